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
// blocks of at most 64 8-column chunks, one per lane, so the four rotated pairs of a chunk stay in one lane.  A run of equal ids
// reads its row of P once.  Four tokens are in flight: their rows (where the id changes) and rotary table rows are requested
// before the first is rotated, rounded and stored, 16 bytes per lane.  The k | v chunks (columns >= D) of a token in a dead panel
// are not written (the caller zeroes those panels).
__global__ __launch_bounds__(256) void qkv_gather_kernel(const float* __restrict__ P, const int64_t* __restrict__ sorted_ids,
                                                          const int64_t* __restrict__ order, const uint8_t* __restrict__ live,
                                                          const float* __restrict__ qa, const float* __restrict__ qb,
                                                          const float* __restrict__ ka, const float* __restrict__ kb, bf16* __restrict__ qkv,
                                                          int64_t n, int N3, int D, int Dh, int R, int S, int64_t V, int cb_chunks) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * 4 + wave;
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
  const float* const tabA = (sec == 1 ? ka : qa) + (rot_on ? c : 0);
  const float* const tabB = (sec == 1 ? kb : qb) + (rot_on ? c : 0);
  long long cur = -1;
  Vec8<float> row{};

  for (int64_t jb = j0; jb < j1; jb += 64) {
    const int64_t jl = jb + lane < j1 ? jb + lane : j1 - 1;
    const long long id64 = sorted_ids[jl], ord64 = order[jl];
    // below 2^31 both (the launcher checks n and V); anything that is no id of the table or no row of qkv becomes -1 and is skipped
    const int my_id = id64 >= 0 && id64 < V ? (int)id64 : -1;
    const int my_ord = ord64 >= 0 && ord64 < n ? (int)ord64 : -1;
    const int cnt = (int)(j1 - jb < 64 ? j1 - jb : 64);
    for (int t0 = 0; t0 < cnt; t0 += 4) {
      Vec8<float> r4[4], A4[4], B4[4];
      int ord4[4];
      bool st4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = t0 + u < cnt ? t0 + u : cnt - 1;
        const int id = __builtin_amdgcn_readlane(my_id, t);
        const int ord = __builtin_amdgcn_readlane(my_ord, t);
        if (id != cur) {                                  // wave-uniform
          cur = id;
          if (id >= 0) row = load8<float>(P + (int64_t)id * N3 + col);
        }
        r4[u] = row;
        ord4[u] = ord;
        const bool tok = t0 + u < cnt && id >= 0 && ord >= 0;
        const bool kv_ok = !live || (tok && live[ord / PANEL] != 0);
        st4[u] = tok && has && (!kv || kv_ok);
        A4[u] = Vec8<float>{};
        B4[u] = Vec8<float>{};
        if (st4[u] && rot_on) {
          const int o = (ord % S) * R;
          A4[u] = load8<float>(tabA + o);
          B4[u] = load8<float>(tabB + o);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (!st4[u]) continue;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = r4[u].get(e);
        if (rot_on) rot_apply8(v, A4[u].lo, A4[u].hi, B4[u].lo, B4[u].hi);
        Vec8<bf16> o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.set(e, v[e]);
        store8s<bf16>(qkv + (int64_t)ord4[u] * N3 + col, o);
      }
    }
  }
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
  const SegColBlocks cb = seg_col_blocks(N3, 1);
  hipLaunchKernelGGL(qkv_gather_kernel, dim3((unsigned)ceil_div(nst, 4), (unsigned)cb.ncb), dim3(256), 0, st, (const float*)P, sorted_ids, order,
                     (const uint8_t*)live, qa, qb, ka, kb, (bf16*)qkv, n, (int)N3, (int)D, Dh, rot ? R : 0, (int)S, V, cb.cb_chunks);
  MEANT_LAUNCH_CHECK("qkv_embed_fwd_by_id: gather");
  meant_route_hit(ROUTE_QKV_FWD_BY_ID);
  // the k | v columns of dead panels: zeros, as meant_qkv_proj_fwd_live leaves them
  if (listed) return zero_panels_launch((bf16*)qkv + D, N3, 2 * D, lists + MEANT_KV_LIST_HDR + nblk + npan, lists + 2, npan, st);
  return MEANT_OK;
}
