// Internal (non-exported) interfaces between the translation units of libmeant_hip.so.
#pragma once
#include "common.h"

// Generic strided batched fp32 GEMM on the f32 MFMA (exact fp32 products, v_mfma_f32_32x32x2_f32):
//   C(b1,b2)[m,n] = act(alpha * sum_k A(m,k) B(k,n) + bias[n]) (+ residual(m,n)) (+ C if accumulate)
struct GemmF32Args {
  const void* A; const void* B; void* C;
  int in_dtype = MEANT_F32;   // storage of A and B (bf16 operands are widened to f32 in LDS: slow, exact, any shape)
  int out_dtype = MEANT_F32;  // storage of C, residual, preact
  int64_t M, N, K, nb1, nb2;
  int64_t sA[4];  // b1, b2, m, k
  int64_t sB[4];  // b1, b2, k, n
  int64_t sC[4];  // b1, b2, m, n
  float alpha;
  int accumulate;
  const float* bias;        // [N] or null
  const void* residual;     // same strides as C, or null
  void* preact;             // same strides as C, or null (value before the activation)
  int epilogue;             // meant_epilogue flags
  int ksplit = 0;           // 0: never split K; -1: the launcher may split K over several workgroups per tile (float atomics)
};
int gemm_f32_launch(const GemmF32Args& a, hipStream_t stream);
// its arguments for row-major operands (api.hip): C[M,N] = A B^T ("NT"), or, tn, C[M,N] += A^T B in float
GemmF32Args f32_rowmajor(bool tn, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                         int storage);

// rotate 8 consecutive columns (4 pairs) with table rows A[0..7], B[0..7]: the rotary epilogue of the NT GEMMs (gemm_bf16.hip) and
// the by-id forward's gather (qkv_fwd_by_id.hip), which must give the bits of the streaming GEMM's epilogue.  That kernel's build
// rounds the two products of a pair separately (packed multiplies, then one subtract / add); the gather's translation unit turns
// contraction off so that the same source is the same arithmetic there.
__device__ __forceinline__ void rot_apply8(float (&v)[8], const f32x4& a0, const f32x4& a1, const f32x4& b0, const f32x4& b1) {
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    const float t0 = v[e], t1 = v[e + 1];
    const float A0 = e < 4 ? a0[e] : a1[e - 4], A1 = e < 4 ? a0[e + 1] : a1[e - 3];
    const float B0 = e < 4 ? b0[e] : b1[e - 4], B1 = e < 4 ? b0[e + 1] : b1[e - 3];
    v[e] = t0 * A0 - t1 * B0;
    v[e + 1] = t1 * A1 + t0 * B1;
  }
}

// bf16 MFMA GEMMs (gemm_bf16.hip).  All operands K-contiguous ("NT"): C[M,N] = A[M,K] B[N,K]^T.
// An `epilogue` bit of the library's own, beside the meant_epilogue flags of the header: C is `float` [M, ldc] (ldc in floats, the pointer
// handed over as bf16*) and takes acc + bias UNROUNDED -- the value every bf16 mode rounds.  No rotary, activation, residual, preact or
// extended operand goes with it (gemm_bf16_nt_launch rejects them).
enum { GEMM_EPI_F32_OUT = 1 << 8 };
struct GemmBf16Args {
  const bf16* A; int64_t lda;
  const bf16* B; int64_t ldb;
  bf16* C; int64_t ldc;
  int64_t M, N, K;
  const float* bias;        // [N] or null
  const bf16* residual; int64_t ldr;
  bf16* preact;             // ldc stride, or null
  int epilogue;
  // optional rotary epilogue of the fused QKV projection (null rot_qa = off): tables float [S, R]
  const float* rot_qa; const float* rot_qb; const float* rot_ka; const float* rot_kb;
  int rot_S, rot_D, rot_Dh, rot_R;
  // "extended" epilogue (an RMSNorm folded into this Linear, see meant_linear_fwd_rowscale / meant_linear_bwd_dx_norm):
  //   C = act(row_scale[m] * acc + bias) + residual - sub_coef[m] * sub[m, n] + bres_scale * bres[m / bres_rows, n]   (every part optional)
  const float* row_scale = nullptr;          // [M]
  const bf16* sub = nullptr; int64_t ldsub = 0;
  const float* sub_coef = nullptr;           // [M]
  const float* bres = nullptr;               // float [M / bres_rows, N]: one row per group of bres_rows consecutive output rows
  int bres_rows = 1; float bres_scale = 1.f; //   (the gradient of a sequence mean, broadcast over the sequence's tokens)
  // rotary epilogue over a PART of the q|k|v row: column n of this launch is column col0 + n of the row (B, bias and C are the caller's,
  // already offset), and, streaming kernel only, the 256-row panels panel_list[0 .. *panel_count) alone (device memory, in the walk order
  // of meant_kv_live_rows; null = all panels).  gemm_bf16_nt_launch rejects a list on any other route.
  int col0 = 0;
  const int* panel_list = nullptr; const int* panel_count = nullptr;
};
// the plain product C[M,N] = A[M,K] B[N,K]^T with B dense (row stride K); the caller adds bias and the epilogue's operands
inline GemmBf16Args gemm_bf16_nt_args(const void* A, int64_t lda, const void* B, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K) {
  GemmBf16Args a{};
  a.A = (const bf16*)A; a.lda = lda; a.B = (const bf16*)B; a.ldb = K; a.C = (bf16*)C; a.ldc = ldc;
  a.M = M; a.N = N; a.K = K;
  return a;
}
int gemm_bf16_nt_launch(const GemmBf16Args& a, hipStream_t stream);
bool gemm_bf16_nt_streams(const GemmBf16Args& a);   // the launch takes the streaming kernel over whole 256-row panels (what a panel list needs)
// the MFMA kernels can take these operands: 16-byte aligned, row strides multiples of 8; K >= 8 and K % 8 == 0 (NT), N >= 8 and K >= 8 (TN).
// Anything else is for the exact f32 engine (gemm_f32_launch).
bool gemm_bf16_nt_ok(const void* A, int64_t lda, const void* B, int64_t ldb, int64_t K);
bool gemm_bf16_tn_ok(const void* dY, int64_t lddy, const void* X, int64_t ldx, int64_t N, int64_t K);
int zero_panels_launch(bf16* C, int64_t ldc, int64_t cols, const int* panels, const int* count, int64_t npan, hipStream_t stream);
// flags[list[i]] = 1 for i < *count (device memory; one list of the key-padding lists and its count), on a zeroed array of `len` bytes
// (qkv_by_id.hip; the 64-row blocks of the by-id backward, the 256-row panels of the by-id forward)
int live_flags_launch(const int* list, const int* count, uint8_t* flags, int64_t len, hipStream_t stream);
// the by-id routes' table-sized GEMMs take V rows rounded up to whole 256-row panels
constexpr int VPAD = 256;
static inline int64_t vpad_rows(int64_t V) { return ceil_div(V, VPAD) * VPAD; }
// dW[N,K] (float, +=) = dY[M,N]^T X[M,K], reduction over the token axis M; dbias[N] += colsum(dY)
// ws: partial-sum workspace of gemm_bf16_tn_ws(M, N, K) bytes, used (and required) only with the `deterministic` option
int gemm_bf16_tn_launch(const bf16* dY, int64_t lddy, const bf16* X, int64_t ldx, float* dW, float* dbias,
                        int64_t M, int64_t N, int64_t K, void* ws, size_t ws_bytes, hipStream_t stream);
size_t gemm_bf16_tn_ws(int64_t M, int64_t N, int64_t K);
// the same reduction over the 64-row blocks rows[0 .. *rows_count) of the token axis only (ascending block indices, count read on the
// device); every row of dY outside the listed blocks must be zero
int gemm_bf16_tn_rows_launch(const bf16* dY, int64_t lddy, const bf16* X, int64_t ldx, float* dW, float* dbias, const int* rows,
                             const int* rows_count, int64_t M, int64_t N, int64_t K, void* ws, size_t ws_bytes, hipStream_t stream);

// column sums: out[N] (+)= sum_m x[m, n]
int colsum_launch(const void* x, int64_t ldx, float* out, int64_t M, int64_t N, int dtype, int accumulate, hipStream_t stream);

// attention cores
int attn_f32_fwd(const float* qkv, float* o, float* lse, const float* key_mask, int64_t G, int64_t S, int H, int Dh,
                 float scale, int causal, void* ws, size_t ws_bytes, hipStream_t stream, float drop_p = 0.f, uint64_t seed = 0);
int attn_f32_bwd(const float* qkv, const float* o, const float* dout, const float* lse, const float* key_mask, float* dqkv,
                 int64_t G, int64_t S, int H, int Dh, float scale, int causal, void* ws, size_t ws_bytes, hipStream_t stream, float drop_p = 0.f,
                 uint64_t seed = 0);
// dropout on the score matrix (meant/xPosAttention.py:59): the materialised fp32 core for both dtypes (bf16 through fp32 copies in `ws`)
size_t attn_drop_ws(int64_t G, int64_t S, int H, int Dh, int dtype);
int attn_drop_bf16(bool backward, const bf16* qkv, const bf16* o, const bf16* dout, bf16* o_out, float* lse, const float* key_mask, bf16* dqkv,
                   int64_t G, int64_t S, int H, int Dh, float scale, int causal, float drop_p, uint64_t seed, void* ws, size_t ws_bytes,
                   hipStream_t stream);
size_t attn_f32_ws(int64_t G, int64_t S, int H, int Dh);
int attn_bf16_fwd(const bf16* qkv, bf16* o, float* lse, const float* key_mask, int64_t G, int64_t S, int H, int Dh,
                  float scale, int causal, void* ws, size_t ws_bytes, hipStream_t stream);
// rot: (qa, qb, ka, kb) float [S, R] or all-null: when given, the adjoint of the rotary map is applied to dq and dk
struct RotTables { const float* qa; const float* qb; const float* ka; const float* kb; int R; };
int attn_bf16_bwd(const bf16* qkv, const bf16* o, const bf16* dout, const float* lse, const float* key_mask, bf16* dqkv,
                  int64_t G, int64_t S, int H, int Dh, float scale, int causal, RotTables rot, void* ws, size_t ws_bytes,
                  hipStream_t stream);
size_t attn_bf16_ws(int64_t G, int64_t S, int H, int Dh);
size_t attn_bf16_fwd_ws(int64_t G, int64_t S, int H, int Dh);
// live 64-row blocks and 256-row panels of the [G * S] token rows under a key mask, by the attention kernels' own "skip this key tile" rule
size_t kv_live_rows_bytes(int64_t G, int64_t S);
int kv_live_rows_launch(const float* key_mask, int64_t G, int64_t S, int causal, int* lists, hipStream_t stream);
// S <= 16: one wave per (group, head) (attn_short.hip); same layouts, statistics and semantics, no workspace
bool attn_short_ok(int64_t S, int Dh);
int attn_short_fwd(const bf16* qkv, bf16* o, float* lse, const float* key_mask, int64_t G, int64_t S, int H, int Dh, float scale,
                   int causal, hipStream_t stream);
int attn_short_bwd(const bf16* qkv, const bf16* dout, const float* lse, const float* key_mask, bf16* dqkv, int64_t G, int64_t S, int H,
                   int Dh, float scale, int causal, RotTables rot, hipStream_t stream);
// single-pass backward (attn_bwd1.hip): Dh = 64, S <= 256 or causal S <= 512; bias2 / flags / masks as prepared by attn_bf16_bwd
bool attn_bwd1_ok(int64_t S, int Dh, int causal);
size_t attn_bwd1_ws(int64_t G, int64_t S, int H, int Dh);
int attn_bwd1_launch(const bf16* qkv, const bf16* o, const bf16* dout, const float* lse, const float* bias2, const int* flags,
                     const uint64_t* masks, bf16* dqkv, void* ws1, int64_t G, int64_t S, int H, float scale, int causal, RotTables rot,
                     hipStream_t stream);

// the radix sort of embedding.hip over caller-made 32-bit keys with a 32-bit value each (all four digits): keys_out ascending,
// equal keys in input order.  Not in place.  ws: sort_u32_ws(n) bytes, 4-byte aligned.  0 < n < 2^31.
size_t sort_u32_ws(int64_t n);
int sort_u32_launch(const uint32_t* keys, const uint32_t* vals, int64_t n, uint32_t* keys_out, uint32_t* vals_out, void* ws,
                    size_t ws_bytes, hipStream_t stream);

#ifdef __HIPCC__
// inclusive scan over the 256 threads of a workgroup, of sums or (MAX) of maxima; *total = the workgroup's result.  `wsum` is 4 words
// of LDS; two barriers.
template <bool MAX>
__device__ __forceinline__ uint32_t block_scan_incl_op(uint32_t x, uint32_t* wsum, uint32_t* total) {
  const auto op = [](uint32_t a, uint32_t b) { return MAX ? (a > b ? a : b) : a + b; };
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = __shfl_up(x, o, 64);
    if (lane >= o) x = op(x, y);
  }
  __syncthreads();                                    // the previous call's readers are done with wsum
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  uint32_t pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t s = wsum[w];
    if (w < wave) pre = op(pre, s);
    tot = op(tot, s);
  }
  *total = tot;
  return op(x, pre);
}
__device__ __forceinline__ uint32_t block_scan_incl(uint32_t x, uint32_t* wsum, uint32_t* total) { return block_scan_incl_op<false>(x, wsum, total); }
__device__ __forceinline__ uint32_t block_scan_incl_max(uint32_t x, uint32_t* wsum, uint32_t* total) { return block_scan_incl_op<true>(x, wsum, total); }
#endif
