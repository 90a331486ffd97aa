// The first text layer's backward once per vocabulary id (meant_qkv_embed_bwd_by_id).
//
//   x[t] = table[id[t]]  ->  n[t] = RMSNorm_g(x[t])  ->  qkv_pre[t] = W' n[t] + b'
// depends on id[t] alone, and its backward is linear in the incoming gradients for fixed x.  So with
//   D[v] = sum of dqkv[t] over the tokens t that carry id v          (qkv_seg_kernel: the walk and the two cross-run passes of seg_sum.h)
// the gradients are table-sized products through the library's own launchers:
//   dW' += D^T Ntab,  db' += colsum(dqkv),  dNtab = D W',  (dXtab, dgain) = RMSNorm backward of (dNtab, table image),
//   dtable[v] += dXtab[v]  (+ the residual gradient summed by id as meant_embedding_bwd_* sum it).
// A bf16 tensor of V rows rounds the summed gradient of an id that holds many tokens once and coherently, where the per-token route
// rounds each token's gradient on its own and the roundings average out.  So D goes to the GEMMs as two images, hi = bf16(D) and
// lo = bf16(D - hi), dNtab comes back as two images (the second is what the first one's rounding dropped, through the GEMM's
// "minus a tensor" epilogue), and the norm backward and dXtab are fp32: table-sized work, a few passes over V rows.
#include "common.h"
#include "internal.h"

#define BYID_REQ(c, ...) MEANT_REQUIRE(c, MEANT_ERR_ARG, __VA_ARGS__)

namespace {

#include "seg_sum.h"               // SEG sorted entries per wave (a stretch); the walk and the crossing-run passes

// flags[list[i]] = 1 for i < *count, on a zeroed array: the live 64-row blocks here, the live 256-row panels of the by-id forward
__global__ __launch_bounds__(256) void live_flags_kernel(const int* __restrict__ list, const int* __restrict__ count, uint8_t* __restrict__ flags,
                                                          int64_t len) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= len || i >= *count) return;
  const int b = list[i];
  if (b >= 0 && b < len) flags[b] = 1;
}

// The segmented sum: seg_walk (seg_sum.h) over a stretch of SEG sorted entries, as emb_seg_kernel (embedding.hip) runs it.  grid.y
// cuts the 3 H Dh columns into blocks of at most 128 8-column chunks (a lane owns two).  A run inside the stretch is final: its
// hi | lo images are stored.  The runs that cross the stretch's ends leave fp32 partial sums in part[stretch][0] (came in from the
// left) / [1] (leaves to the right) for seg_cross_kernel / seg_long_kernel (seg_sum.h, with the hi | lo store).
// cpart[stretch][:] = the column sums of the stretch's rows, for the bias gradient.
// The rows policy: the k | v chunks (columns >= Dq) of a row in a dead 64-row block are never read: they are zeros.
struct QkvLiveRows {
  const uint8_t* live_blocks; bool kv[2];
  __device__ __forceinline__ bool live(int64_t ord) const { return !live_blocks || live_blocks[ord >> 6] != 0; }
  __device__ __forceinline__ bool reads(int k, bool row_live) const { return !kv[k] || row_live; }
};
__global__ __launch_bounds__(256) void qkv_seg_kernel(const bf16* __restrict__ dqkv, const int64_t* __restrict__ sorted_ids,
                                                       const int64_t* __restrict__ order, const uint8_t* __restrict__ live,
                                                       bf16* __restrict__ Dhi, bf16* __restrict__ Dlo, float* __restrict__ part,
                                                       float* __restrict__ cpart, int64_t n, int64_t N3, int64_t Dq, int64_t V,
                                                       int cb_chunks) {
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t j0 = s * SEG;
  if (j0 >= n) return;
  const int64_t j1 = j0 + SEG < n ? j0 + SEG : n;
  const SegCols c = seg_cols(N3, cb_chunks);
  const QkvLiveRows rows{live, {c.col[0] >= Dq, c.col[1] >= Dq}};
  const SegSlotSink<SegStoreHiLo> sink{{Dhi, Dlo}, part + s * 2 * N3, N3};
  seg_walk<true>(dqkv, N3, sorted_ids, order, n, V, j0, j1, c, rows, sink, cpart + s * N3);
}

// db[col] += the sum over the stretches of cpart[stretch][col]: 16 equal pieces of the stretch axis summed in order by 16 threads of
// 4 columns each, the pieces added as a fixed binary tree
__global__ __launch_bounds__(256) void qkv_colsum_kernel(const float* __restrict__ cpart, float* __restrict__ db, int64_t nst, int64_t N3) {
  __shared__ f32x4 red[16][16];
  const int tid = threadIdx.x, p = tid >> 4;
  const int64_t col = (int64_t)blockIdx.x * 64 + (tid & 15) * 4;
  const bool active = col < N3;
  const int64_t piece = (nst + 15) / 16, k0 = p * piece, k1 = k0 + piece < nst ? k0 + piece : nst;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (active)
    for (int64_t k = k0; k < k1; ++k) acc += *reinterpret_cast<const f32x4*>(cpart + k * N3 + col);
  red[p][tid & 15] = acc;
  __syncthreads();
#pragma unroll
  for (int h = 8; h > 0; h >>= 1) {
    if (p < h) red[p][tid & 15] += red[p + h][tid & 15];
    __syncthreads();
  }
  if (p == 0 && active) {
    f32x4* dst = reinterpret_cast<f32x4*>(db + col);
    *dst = *dst + red[0][tid & 15];
  }
}

// fp32 operands of the norm backward: dn = the two images of dNtab added, x = the table image widened; and ones[Vp] for the GEMM epilogue
__global__ __launch_bounds__(256) void widen_kernel(const bf16* __restrict__ dn_a, const bf16* __restrict__ dn_r, const bf16* __restrict__ table,
                                                     float* __restrict__ dn, float* __restrict__ x, int64_t chunks) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * 256) {
    const int64_t off = c * 8;
    const Vec8<bf16> a = load8<bf16>(dn_a + off), r = load8<bf16>(dn_r + off), t = load8<bf16>(table + off);
    Vec8<float> v, w;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v.set(e, a.get(e) + r.get(e));
      w.set(e, t.get(e));
    }
    store8<float>(dn + off, v);
    store8<float>(x + off, w);
  }
}
__global__ __launch_bounds__(256) void ones_kernel(float* __restrict__ p, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = 1.f;
}

// dtable[v, :] += dxtab[v, :] for the rows v of [id_lo, id_hi)
__global__ __launch_bounds__(256) void table_add_kernel(const float* __restrict__ dxtab, float* __restrict__ dtable, int64_t first, int64_t chunks) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * 256) {
    const int64_t off = first + c * 8;
    const Vec8<float> g = load8<float>(dxtab + off);
    Vec8<float> v = load8<float>(dtable + off);
#pragma unroll
    for (int e = 0; e < 8; ++e) v.set(e, v.get(e) + g.get(e));
    store8<float>(dtable + off, v);
  }
}

// the workspace: what survives from the shared stage to the table stages first
struct ByIdWs { size_t dxtab, dhi, dlo, ntab, rinv, dnlo, dna, dnr, ones, dn32, x32, part, cpart, longk, live, sub, sub_bytes, total; };
ByIdWs byid_layout(int64_t n, int64_t d, int64_t N3, int64_t V) {
  ByIdWs w;
  const int64_t Vp = vpad_rows(V), nst = ceil_div(n, SEG);
  size_t off = 0;
  const auto take = [&off](size_t bytes) { const size_t o = off; off += align256(bytes); return o; };
  w.dxtab = take((size_t)V * d * sizeof(float));
  w.dhi = take((size_t)Vp * N3 * sizeof(bf16));
  w.dlo = take((size_t)Vp * N3 * sizeof(bf16));
  w.ntab = take((size_t)Vp * d * sizeof(bf16));
  w.rinv = take((size_t)V * sizeof(float));
  w.dnlo = take((size_t)Vp * d * sizeof(bf16));
  w.dna = take((size_t)Vp * d * sizeof(bf16));
  w.dnr = take((size_t)Vp * d * sizeof(bf16));
  w.ones = take((size_t)Vp * sizeof(float));
  w.dn32 = take((size_t)V * d * sizeof(float));
  w.x32 = take((size_t)V * d * sizeof(float));
  w.part = take((size_t)nst * 2 * N3 * sizeof(float));
  w.cpart = take((size_t)nst * N3 * sizeof(float));
  w.longk = take((size_t)nst * sizeof(int));
  w.live = take((size_t)ceil_div(n, 64));
  // one region for the launchers' own workspaces, which are used one after the other: the ordered dW partials (option
  // "deterministic"), the norm backward's column partials, the residual gradient's segmented sum
  size_t sub = gemm_bf16_tn_ws(Vp, N3, d);
  const size_t nb = meant_rmsnorm_bwd_ws(V, d), sb = meant_embedding_bwd_seg_ws(n, d);
  if (nb > sub) sub = nb;
  if (sb > sub) sub = sb;
  w.sub_bytes = sub;
  w.sub = take(sub);
  w.total = off;
  return w;
}

bool byid_shape_ok(int64_t n, int64_t d, int64_t N3, int64_t V) {
  return n > 0 && d > 0 && N3 > 0 && V > 0 && n < (1ll << 31) && V < (1ll << 31) && d % 8 == 0 && N3 % 192 == 0 && N3 < (1ll << 22) &&
         d < (1ll << 22);
}

}  // namespace

int live_flags_launch(const int* list, const int* count, uint8_t* flags, int64_t len, hipStream_t stream) {
  hipLaunchKernelGGL(live_flags_kernel, dim3((unsigned)ceil_div(len, 256)), dim3(256), 0, stream, list, count, flags, len);
  MEANT_LAUNCH_CHECK("live_flags");
  return MEANT_OK;
}

extern "C" size_t meant_qkv_embed_bwd_by_id_ws(int64_t n, int64_t d, int64_t N3, int64_t V) {
  return byid_shape_ok(n, d, N3, V) ? byid_layout(n, d, N3, V).total : 0;
}

extern "C" int meant_qkv_embed_bwd_by_id(const void* dqkv, const void* dres, const int64_t* sorted_ids, const int64_t* order,
                                         const void* table_bf16, const float* gain, float eps, const void* wT, const void* kv_lists,
                                         float* dw, float* db, float* dgain, float* dtable, int64_t n, int64_t d, int64_t N3, int64_t V,
                                         int64_t id_lo, int64_t id_hi, int stage, void* workspace, size_t workspace_bytes, void* stream) {
  BYID_REQ(sorted_ids && order && dtable && workspace && (stage & ~(MEANT_BY_ID_SHARED | MEANT_BY_ID_TABLE)) == 0 && stage != 0,
           "qkv_embed_bwd_by_id: bad argument");
  MEANT_REQUIRE(byid_shape_ok(n, d, N3, V), MEANT_ERR_UNSUPPORTED,
                "qkv_embed_bwd_by_id: n=%lld d=%lld N3=%lld V=%lld: n, V < 2^31, d %% 8 == 0, N3 = 3 H Dh with H Dh %% 64 == 0", (long long)n,
                (long long)d, (long long)N3, (long long)V);
  BYID_REQ(0 <= id_lo && id_lo <= id_hi && id_hi <= V, "qkv_embed_bwd_by_id: bad id range");
  const ByIdWs w = byid_layout(n, d, N3, V);
  MEANT_REQUIRE(workspace_bytes >= w.total, MEANT_ERR_WORKSPACE, "qkv_embed_bwd_by_id: workspace of %zu bytes needed, %zu given", w.total,
                workspace_bytes);
  BYID_REQ(meant_aligned16(workspace) && meant_aligned16(dtable) && (!dres || meant_aligned16(dres)), "qkv_embed_bwd_by_id: 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  char* base = (char*)workspace;
  float* dxtab = (float*)(base + w.dxtab);
  const int64_t Vp = vpad_rows(V), nst = ceil_div(n, SEG);
  int rc;

  if (stage & MEANT_BY_ID_SHARED) {
    BYID_REQ(dqkv && table_bf16 && gain && wT && dw && db && dgain, "qkv_embed_bwd_by_id: null pointer");
    BYID_REQ(meant_aligned16(dqkv) && meant_aligned16(table_bf16) && meant_aligned16(wT) && meant_aligned16(db),
             "qkv_embed_bwd_by_id: 16-byte alignment");
    bf16 *Dhi = (bf16*)(base + w.dhi), *Dlo = (bf16*)(base + w.dlo), *ntab = (bf16*)(base + w.ntab);
    bf16 *dnlo = (bf16*)(base + w.dnlo), *dna = (bf16*)(base + w.dna), *dnr = (bf16*)(base + w.dnr);
    float *ones = (float*)(base + w.ones), *dn32 = (float*)(base + w.dn32), *x32 = (float*)(base + w.x32);
    float *rinv = (float*)(base + w.rinv), *part = (float*)(base + w.part), *cpart = (float*)(base + w.cpart);
    int* longk = (int*)(base + w.longk);
    uint8_t* live = nullptr;
    // rows of ids that never occur, and the padding rows: zeros (hi and lo are neighbours in the workspace)
    hipError_t e = hipMemsetAsync(Dhi, 0, w.ntab - w.dhi, st);
    if (e == hipSuccess && Vp > V) e = hipMemsetAsync(ntab + V * d, 0, (size_t)(Vp - V) * d * sizeof(bf16), st);
    if (e == hipSuccess && kv_lists) {
      live = (uint8_t*)(base + w.live);
      e = hipMemsetAsync(live, 0, (size_t)ceil_div(n, 64), st);
    }
    MEANT_REQUIRE(e == hipSuccess, MEANT_ERR_LAUNCH, "qkv_embed_bwd_by_id: clearing the workspace failed: %s", hipGetErrorString(e));
    if (live) {
      const int64_t nblk = n / 64;                       // the lists cover whole 64-row blocks: S % 256 == 0
      BYID_REQ(n % 64 == 0, "qkv_embed_bwd_by_id: key-padding lists need n %% 64 == 0");
      rc = live_flags_launch((const int*)kv_lists + MEANT_KV_LIST_HDR, (const int*)kv_lists, live, nblk, st);
      if (rc) return rc;
    }
    const SegColBlocks cb = seg_col_blocks(N3, 2);
    hipLaunchKernelGGL(qkv_seg_kernel, dim3((unsigned)ceil_div(nst, 4), (unsigned)cb.ncb), dim3(256), 0, st, (const bf16*)dqkv, sorted_ids, order,
                       (const uint8_t*)live, Dhi, Dlo, part, cpart, n, N3, N3 / 3, V, cb.cb_chunks);
    seg_cross_launch(SegStoreHiLo{Dhi, Dlo}, sorted_ids, (const float*)part, longk, n, N3, V, st);
    hipLaunchKernelGGL(qkv_colsum_kernel, dim3((unsigned)ceil_div(N3, 64)), dim3(256), 0, st, (const float*)cpart, db, nst, N3);
    MEANT_LAUNCH_CHECK("qkv_embed_bwd_by_id: segmented sum");
    // table-sized work
    rc = meant_rmsnorm_fwd(table_bf16, gain, ntab, rinv, V, d, eps, 0.f, 0, MEANT_BF16, stream);
    if (rc) return rc;
    void* sub = base + w.sub;
    rc = gemm_bf16_tn_launch(Dhi, N3, ntab, d, dw, nullptr, Vp, N3, d, sub, w.sub_bytes, st);
    if (!rc) rc = gemm_bf16_tn_launch(Dlo, N3, ntab, d, dw, nullptr, Vp, N3, d, sub, w.sub_bytes, st);
    if (rc) return rc;
    GemmBf16Args a{};
    a.A = Dlo; a.lda = N3; a.B = (const bf16*)wT; a.ldb = N3; a.C = dnlo; a.ldc = d;
    a.M = Vp; a.N = d; a.K = N3;
    rc = gemm_bf16_nt_launch(a, st);
    if (rc) return rc;
    a.A = Dhi; a.C = dna; a.residual = dnlo; a.ldr = d;
    rc = gemm_bf16_nt_launch(a, st);
    if (rc) return rc;
    // the second image of dNtab: the same product minus the first image, rounded
    hipLaunchKernelGGL(ones_kernel, dim3((unsigned)ceil_div(Vp, 256)), dim3(256), 0, st, ones, Vp);
    a.C = dnr; a.sub = dna; a.ldsub = d; a.sub_coef = ones;
    rc = gemm_bf16_nt_launch(a, st);
    if (rc) return rc;
    {
      const int64_t chunks = V * d / 8;
      int64_t nb = ceil_div(chunks, 256);
      if (nb > 8192) nb = 8192;
      hipLaunchKernelGGL(widen_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const bf16*)dna, (const bf16*)dnr, (const bf16*)table_bf16, dn32, x32, chunks);
      MEANT_LAUNCH_CHECK("qkv_embed_bwd_by_id: widen");
    }
    rc = meant_rmsnorm_bwd(dn32, x32, gain, rinv, dxtab, dgain, V, d, eps, 0.f, 0, nullptr, nullptr, MEANT_F32, sub, w.sub_bytes, stream);
    if (rc) return rc;
    meant_route_hit(ROUTE_QKV_BY_ID);
  }

  if ((stage & MEANT_BY_ID_TABLE) && id_lo < id_hi) {
    if (dres) {                                          // the residual gradient, summed by id as the embedding's own backward sums it
      if (d <= 1024)
        rc = meant_embedding_bwd_sorted_range(dres, sorted_ids, order, dtable, n, d, V, id_lo, id_hi, MEANT_BF16, stream);
      else
        rc = meant_embedding_bwd_seg(dres, sorted_ids, order, dtable, n, d, V, id_lo, id_hi, MEANT_BF16, base + w.sub, w.sub_bytes, stream);
      if (rc) return rc;
    }
    const int64_t chunks = (id_hi - id_lo) * d / 8;
    int64_t nb = ceil_div(chunks, 256);
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(table_add_kernel, dim3((unsigned)nb), dim3(256), 0, st, (const float*)dxtab, dtable, id_lo * d, chunks);
    MEANT_LAUNCH_CHECK("qkv_embed_bwd_by_id: table rows");
  }
  return MEANT_OK;
}
