// The first text layer's q|k|v projection once per vocabulary id (meant_qkv_embed_fwd_by_id), the forward half of qkv_by_id.hip.
//
//   x[t] = table[id[t]]  ->  n[t] = RMSNorm_g(x[t])  ->  pre[t] = W' n[t] + b'  ->  qkv[t] = bf16(rotary_{t mod S}(pre[t]))
// Everything up to pre[t] depends on id[t] alone, so it is computed on the V rows of the table: the norm kernel on the bf16 table
// image, one NT GEMM with unrounded float output (GEMM_EPI_F32_OUT) into P [Vp, 3 H Dh], and a gather over the sorted ids that reads
// a row of P once per run of equal ids and, per token of the run, applies the rotary map of the token's position and rounds once.
// Bit equality with the per-token route (meant_rmsnorm_fwd + meant_qkv_proj_fwd_live on the streaming kernel) is the contract: the
// same norm kernel on the same bf16 rows, the same GEMM kernel family with the same K order, acc + bias formed once in fp32, and the
// rotary arithmetic of the streaming kernel's epilogue -- rot_apply8 with the two products of a pair rounded separately, which is
// what that kernel's build does; contraction is off for this file so that the shared source means the same here.
#pragma clang fp contract(off)
#include "common.h"
#include "internal.h"

#define FBYID_REQ(c, ...) MEANT_REQUIRE(c, MEANT_ERR_ARG, __VA_ARGS__)

namespace {

#include "seg_sum.h"               // SEG sorted entries per wave (a stretch), and the cut of a row into column blocks
constexpr int PANEL = 256;         // rows of a key-padding panel (meant_kv_live_rows)

// The gather, the mirror image of qkv_seg_kernel: a wave walks a stretch of SEG sorted entries; grid.y cuts the 3 H Dh columns into
// blocks of at most 64 8-column chunks, one per lane, so the four rotated pairs of a chunk stay in one lane; the cut falls on multiples
// of 8 chunks (gather_col_blocks), so every block's stores cover whole 128-byte lines of a row of qkv.  The k | v chunks (columns >= D)
// of a token in a dead panel are not written (the caller zeroes those panels).
// What a token needs -- its id, its row of qkv, its offset into the rotary tables, its panel's flag -- is formed once per lane for 64
// entries, a block ahead, and broadcast.  The rows travel in two register sets of GATHER_G tokens: while one is rotated, rounded and
// stored (16 bytes per lane), the other is on its way, and the set after it is requested before the first one's stores are issued:
// the memory counter retires in order, so a load behind a store would wait for that store.  For the same reason the last loads of
// a set are issued by every lane every time (a lane that rotates nothing repeats the block's first rotated chunk): the number of
// loads behind a set is then known when it is waited for.
//   ROT (a block with rotated chunks: q and k)  a run of equal ids reads its row of P once; the rotary table rows per token
//   otherwise (v)                               the row of P per token: the repeats of a run are cache hits, and no load hangs on a branch
constexpr int GATHER_G = 2;        // 124 registers, four waves per SIMD; 4 tokens per set: 220 and two, and measured slower
struct GatherBlock { int id, ord, off, kv_ok; };       // 64 sorted entries, one per lane
template <bool ROT>
struct GatherSet;
template <>
struct GatherSet<true> { Vec8<float> r[GATHER_G], A[GATHER_G], B[GATHER_G]; int ord[GATHER_G]; bool st[GATHER_G]; };
template <>
struct GatherSet<false> { Vec8<float> r[GATHER_G]; int ord[GATHER_G]; bool st[GATHER_G]; };
inline SegColBlocks gather_col_blocks(int64_t width) {
  const SegColBlocks cb = seg_col_blocks(width, 1);
  const int cut = (cb.cb_chunks + 7) & ~7;               // <= 64: seg_col_blocks gives at most 64 chunks to a block
  return {(int)ceil_div(width >> 3, cut), cut};
}

// has: the lane has a chunk, at column col (a lane without one mirrors the first and stores nothing); rot_on: the chunk is rotated,
// by the table rows tabA / tabB + the token's offset (a lane that rotates nothing: the block's first rotated chunk's)
template <bool ROT>
__device__ __forceinline__ void gather_walk(const float* __restrict__ P, const int64_t* __restrict__ sorted_ids, const int64_t* __restrict__ order,
                                            const uint8_t* __restrict__ live, const float* __restrict__ tabA, const float* __restrict__ tabB,
                                            bf16* __restrict__ qkv, int64_t n, int N3, int R, int S, int64_t V, int64_t j0, int64_t j1, int col,
                                            bool has, bool kv, bool rot_on) {
  const int lane = threadIdx.x & 63;
  int cur = -1;
  Vec8<float> row{};

  // Ids and row numbers are below 2^31 both (the launcher checks n and V); anything that is no id of the table or no row of qkv
  // becomes -1 and is skipped.  Past the end: the last entry again.  The panel's flag follows once the row numbers have arrived.
  auto entries = [&](int64_t jb) {
    const int64_t jl = jb + lane < j1 ? jb + lane : j1 - 1;
    const long long id64 = sorted_ids[jl], ord64 = order[jl];
    GatherBlock b;
    b.id = id64 >= 0 && id64 < V ? (int)id64 : -1;
    b.ord = ord64 >= 0 && ord64 < n ? (int)ord64 : -1;
    b.off = b.ord >= 0 ? (b.ord % S) * R : 0;           // the token's rows of the rotary tables
    b.kv_ok = 1;
    return b;
  };
  auto flags = [&](const GatherBlock& b) { return !live || (b.ord >= 0 && live[b.ord / PANEL] != 0) ? 1 : 0; };
  // the tokens [t0, t0 + GATHER_G) of a block; those past cnt repeat the last one and store nothing
  auto request = [&](const GatherBlock& b, int t0, int cnt, GatherSet<ROT>& g) {
#pragma unroll
    for (int u = 0; u < GATHER_G; ++u) {
      const int t = t0 + u < cnt ? t0 + u : (cnt ? cnt - 1 : 0);
      const int id = __builtin_amdgcn_readlane(b.id, t);
      const int ord = __builtin_amdgcn_readlane(b.ord, t);
      g.ord[u] = ord;
      g.st[u] = t0 + u < cnt && id >= 0 && ord >= 0 && has && (!kv || __builtin_amdgcn_readlane(b.kv_ok, t) != 0);
      if constexpr (ROT) {
        if (id != cur) {                                // wave-uniform
          cur = id;
          if (id >= 0) row = load8<float>(P + (int64_t)id * N3 + col);
        }
        g.r[u] = row;
        const int o = __builtin_amdgcn_readlane(b.off, t);
        g.A[u] = load8<float>(tabA + o);
        g.B[u] = load8<float>(tabB + o);
      } else {
        g.r[u] = load8<float>(P + (int64_t)(id >= 0 ? id : 0) * N3 + col);
      }
    }
  };
  auto store = [&](const GatherSet<ROT>& g) {
#pragma unroll
    for (int u = 0; u < GATHER_G; ++u) {
      if (!g.st[u]) continue;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = g.r[u].get(e);
      if constexpr (ROT) {
        if (rot_on) rot_apply8(v, g.A[u].lo, g.A[u].hi, g.B[u].lo, g.B[u].hi);
      }
      Vec8<bf16> o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o.set(e, v[e]);
      store8s<bf16>(qkv + (int64_t)g.ord[u] * N3 + col, o);
    }
  };

  GatherSet<ROT> ga, gb;
  GatherBlock blk = entries(j0), nxt = entries(j0 + 64);
  blk.kv_ok = flags(blk);
  request(blk, 0, (int)(j1 - j0 < 64 ? j1 - j0 : 64), ga);
  for (int64_t jb = j0; jb < j1; jb += 64) {
    const int cnt = (int)(j1 - jb < 64 ? j1 - jb : 64);
    const int ncnt = jb + 64 < j1 ? (int)(j1 - jb - 64 < 64 ? j1 - jb - 64 : 64) : 0;     // past the end: nothing is stored
    const GatherBlock after = entries(jb + 128);
    nxt.kv_ok = flags(nxt);
    for (int t0 = 0; t0 < cnt; t0 += 2 * GATHER_G) {
      request(blk, t0 + GATHER_G, cnt, gb);
      store(ga);
      const bool last = t0 + 2 * GATHER_G >= cnt;      // the set after the second one opens the next block
      const GatherBlock from{last ? nxt.id : blk.id, last ? nxt.ord : blk.ord, last ? nxt.off : blk.off, last ? nxt.kv_ok : blk.kv_ok};
      request(from, last ? 0 : t0 + 2 * GATHER_G, last ? ncnt : cnt, ga);
      store(gb);
    }
    blk = nxt;
    nxt = after;
  }
}

__global__ __launch_bounds__(256) void qkv_gather_kernel(const float* __restrict__ P, const int64_t* __restrict__ sorted_ids,
                                                          const int64_t* __restrict__ order, const uint8_t* __restrict__ live,
                                                          const float* __restrict__ qa, const float* __restrict__ qb,
                                                          const float* __restrict__ ka, const float* __restrict__ kb, bf16* __restrict__ qkv,
                                                          int64_t n, int N3, int D, int Dh, int R, int S, int64_t V, int cb_chunks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = seg_uniform64((int64_t)blockIdx.x * 4 + wave);         // a wave's stretch: the same in every lane
  const int64_t j0 = s * SEG;
  if (j0 >= n) return;
  const int64_t j1 = j0 + SEG < n ? j0 + SEG : n;
  const int c0 = blockIdx.y * cb_chunks;
  const int left = (N3 >> 3) - c0;
  const int nch = left < cb_chunks ? left : cb_chunks;
  const bool has = lane < nch;
  const int col = (c0 + (has ? lane : 0)) * 8;          // a lane without a chunk mirrors the first one and stores nothing
  const int sec = col / D;
  const int c = (col - sec * D) % Dh;
  const bool rot_on = qa != nullptr && sec < 2 && c < R;
  const bool kv = sec >= 1;
  // the block's first rotated chunk, for the lanes that rotate nothing; none: the block takes the walk without tables
  const unsigned long long rot_lanes = __ballot(rot_on);
  if (rot_lanes == 0) {
    gather_walk<false>(P, sorted_ids, order, live, nullptr, nullptr, qkv, n, N3, R, S, V, j0, j1, col, has, kv, false);
    return;
  }
  const int first = __builtin_ctzll(rot_lanes);
  const int rsec = __builtin_amdgcn_readlane(sec, first), rc = __builtin_amdgcn_readlane(c, first);
  const float* const tabA = (rot_on ? (sec == 1 ? ka : qa) + c : (rsec == 1 ? ka : qa) + rc);
  const float* const tabB = (rot_on ? (sec == 1 ? kb : qb) + c : (rsec == 1 ? kb : qb) + rc);
  gather_walk<true>(P, sorted_ids, order, live, tabA, tabB, qkv, n, N3, R, S, V, j0, j1, col, has, kv, rot_on);
}

struct FwdByIdWs { size_t ntab, rinv, p, live, total; };
FwdByIdWs fwd_byid_layout(int64_t n, int64_t d, int64_t N3, int64_t V) {
  FwdByIdWs w;
  const int64_t Vp = vpad_rows(V);
  size_t off = 0;
  const auto take = [&off](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
  w.ntab = take((size_t)Vp * d * sizeof(bf16));
  w.rinv = take((size_t)V * sizeof(float));
  w.p = take((size_t)Vp * N3 * sizeof(float));
  w.live = take((size_t)ceil_div(n, PANEL));
  w.total = off;
  return w;
}

bool fwd_byid_shape_ok(int64_t n, int64_t d, int64_t N3, int64_t V) {
  return n > 0 && d > 0 && N3 > 0 && V > 0 && n < (1ll << 31) && V < (1ll << 31) && d % 8 == 0 && N3 % 24 == 0 && N3 < (1ll << 22) && d < (1ll << 22);
}

// a product the route stands for, as the launcher of the NT GEMM would see it
GemmBf16Args shape_args(int64_t M, int64_t N, int64_t K) { return gemm_bf16_nt_args(nullptr, K, nullptr, nullptr, N, M, N, K); }

}  // namespace

extern "C" size_t meant_qkv_embed_fwd_by_id_ws(int64_t n, int64_t d, int64_t N3, int64_t V) {
  return fwd_byid_shape_ok(n, d, N3, V) ? fwd_byid_layout(n, d, N3, V).total : 0;
}

// The shape rule: the table product and the per-token product it replaces must both come from the streaming kernel.  (The one-tile
// kernels need not sum in the same order, and their build contracts the rotary pair into FMAs where the streaming kernel's rounds
// the products separately.)  meant_qkv_proj_fwd_live runs the streaming kernel -- as one launch or as its q and k|v launches --
// exactly where the whole [n, 3 H Dh] product would.
extern "C" int meant_qkv_embed_fwd_by_id_ok(int64_t n, int64_t d, int64_t N3, int64_t V) {
  if (!fwd_byid_shape_ok(n, d, N3, V) || N3 % 3 != 0 || (N3 / 3) % 256 != 0 || n % 256 != 0) return 0;
  if (meant_num_cus() <= 0) return 0;                  // no current device: the launcher's rule counts its compute units
  const int64_t Vp = vpad_rows(V);
  return gemm_bf16_nt_streams(shape_args(n, N3, d)) && gemm_bf16_nt_streams(shape_args(Vp, N3, d)) ? 1 : 0;
}

extern "C" int meant_qkv_embed_fwd_by_id(const void* table_bf16, const float* gain, float eps, const void* w_bf16, const float* bias,
                                         const int64_t* sorted_ids, const int64_t* order, const void* kv_lists, const float* qa,
                                         const float* qb, const float* ka, const float* kb, void* qkv, int64_t n, int64_t S, int64_t d,
                                         int H, int Dh, int R, int64_t V, void* workspace, size_t workspace_bytes, void* stream) {
  FBYID_REQ(table_bf16 && gain && w_bf16 && sorted_ids && order && qkv && workspace && H > 0 && Dh > 0 && S > 0, "qkv_embed_fwd_by_id: bad argument");
  const int64_t D = (int64_t)H * Dh, N3 = 3 * D;
  MEANT_REQUIRE(fwd_byid_shape_ok(n, d, N3, V) && n % S == 0 && S < (1ll << 22) && Dh % 8 == 0, MEANT_ERR_UNSUPPORTED,
                "qkv_embed_fwd_by_id: n=%lld S=%lld d=%lld H=%d Dh=%d V=%lld: n, V < 2^31, n %% S == 0, d %% 8 == 0, Dh %% 8 == 0", (long long)n,
                (long long)S, (long long)d, H, Dh, (long long)V);
  const bool rot = qa != nullptr;
  FBYID_REQ(!rot || (qb && ka && kb && R > 0 && R % 8 == 0 && R <= Dh), "qkv_embed_fwd_by_id: bad rotary tables (rot_dim %% 8 == 0)");
  MEANT_REQUIRE(meant_qkv_embed_fwd_by_id_ok(n, d, N3, V), MEANT_ERR_UNSUPPORTED,
                "qkv_embed_fwd_by_id: the streaming NT kernel must take both the [n, H Dh] and the [V, 3 H Dh] product (n=%lld d=%lld N3=%lld V=%lld)",
                (long long)n, (long long)d, (long long)N3, (long long)V);
  const FwdByIdWs w = fwd_byid_layout(n, d, N3, V);
  MEANT_REQUIRE(workspace_bytes >= w.total, MEANT_ERR_WORKSPACE, "qkv_embed_fwd_by_id: workspace of %zu bytes needed, %zu given", w.total,
                workspace_bytes);
  FBYID_REQ(meant_aligned16(workspace) && meant_aligned16(table_bf16) && meant_aligned16(w_bf16) && meant_aligned16(qkv) &&
                (!rot || (meant_aligned16(qa) && meant_aligned16(qb) && meant_aligned16(ka) && meant_aligned16(kb))),
            "qkv_embed_fwd_by_id: 16-byte alignment");
  const bool listed = kv_lists != nullptr;
  FBYID_REQ(!listed || S % PANEL == 0, "qkv_embed_fwd_by_id: key-padding lists need S %% 256 == 0");
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)workspace;
  bf16* ntab = (bf16*)(base + w.ntab);
  float *rinv = (float*)(base + w.rinv), *P = (float*)(base + w.p);
  uint8_t* live = listed ? (uint8_t*)(base + w.live) : nullptr;
  const int64_t Vp = vpad_rows(V), nst = ceil_div(n, SEG), nblk = n / 64, npan = n / PANEL;

  // 1. the norm on the table image, zero-padded to whole 256-row panels
  // The norm's launcher packs 1, 2 or 4 rows into a wave where the row count divides (norm.hip, norm_route), and the packed and the
  // one-row kernels need not add a row's squares in the same order.  The per-token rows are a multiple of 256; so that the table's
  // rows run on the kernel those take, they go as a multiple of four, and a table that is none gets its last four rows in a second
  // launch, which writes the rows both launches cover a second time with the same bits.
  const int64_t V4 = V & ~(int64_t)3;
  int rc = meant_rmsnorm_fwd(table_bf16, gain, ntab, rinv, V4, d, eps, 0.f, 0, MEANT_BF16, stream);
  if (!rc && V4 < V)
    rc = meant_rmsnorm_fwd((const bf16*)table_bf16 + (V - 4) * d, gain, ntab + (V - 4) * d, rinv + (V - 4), 4, d, eps, 0.f, 0, MEANT_BF16, stream);
  if (rc) return rc;
  hipError_t e = hipSuccess;
  if (Vp > V) e = hipMemsetAsync(ntab + V * d, 0, (size_t)(Vp - V) * d * sizeof(bf16), st);
  if (e == hipSuccess && listed) e = hipMemsetAsync(live, 0, (size_t)npan, st);
  MEANT_REQUIRE(e == hipSuccess, MEANT_ERR_LAUNCH, "qkv_embed_fwd_by_id: clearing the workspace failed: %s", hipGetErrorString(e));
  // 2. P = Ntab W'^T + b', unrounded
  GemmBf16Args a{};
  a.A = ntab; a.lda = d; a.B = (const bf16*)w_bf16; a.ldb = d; a.C = (bf16*)P; a.ldc = N3;
  a.M = Vp; a.N = N3; a.K = d; a.bias = bias; a.epilogue = GEMM_EPI_F32_OUT;
  rc = gemm_bf16_nt_launch(a, st);
  if (rc) return rc;
  // 3. the gather
  const int* const lists = (const int*)kv_lists;
  if (listed) rc = live_flags_launch(lists + MEANT_KV_LIST_HDR + nblk, lists + 1, live, npan, st);
  if (rc) return rc;
  const SegColBlocks cb = gather_col_blocks(N3);
  hipLaunchKernelGGL(qkv_gather_kernel, dim3((unsigned)ceil_div(nst, 4), (unsigned)cb.ncb), dim3(256), 0, st, (const float*)P, sorted_ids, order,
                     (const uint8_t*)live, qa, qb, ka, kb, (bf16*)qkv, n, (int)N3, (int)D, Dh, rot ? R : 0, (int)S, V, cb.cb_chunks);
  MEANT_LAUNCH_CHECK("qkv_embed_fwd_by_id: gather");
  meant_route_hit(ROUTE_QKV_FWD_BY_ID);
  // the k | v columns of dead panels: zeros, as meant_qkv_proj_fwd_live leaves them
  if (listed) return zero_panels_launch((bf16*)qkv + D, N3, 2 * D, lists + MEANT_KV_LIST_HDR + nblk + npan, lists + 2, npan, st);
  return MEANT_OK;
}
