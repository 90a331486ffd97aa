// Cross-entropy of probabilities against class-probability ("soft") targets: the VQA loop's loss (vqa.py:173,209 calls
// nn.CrossEntropyLoss()(out, target) on the Sigmoid output with the float [B, C] answer weights of utils/custom_datasets.py:214-218,
// 0.3 / 0.6 / 0.9 / 1.0 on up to a handful of the 3129 answers; a row may be all zero and need not sum to 1).
//   * meant_ce_probs_soft -- row_loss[b] = sum_c t[b,c] (logsumexp(p[b,:]) - p[b,c]), loss = mean_b, d loss / d p = (T_b softmax - t) / B
// Evaluated in the shift-invariant form, per row:
//   mx = max_c p_c;  s = sum_c exp(p_c - mx);  T = sum_c t_c;  D = sum_c t_c (mx - p_c)
//   row = T log(s) + D;  d_c = (T exp(p_c - mx) / s - t_c) / B
// (exp(p - lse) and T lse - sum t p both cancel against the size of p: with probabilities + 1000 they lose everything).
// Two forms, both with the row in registers (probs and target read once, the gradient written once), by dword loads: lane i of a
// row's group takes columns i, i + G, i + 2G, ... (a wave's 256 contiguous bytes coalesce wherever the row starts; rows of 3129
// floats start off the 16-byte grid), and nothing at or beyond column C is addressed:
//   wave  (C <= 1024): a wave per row, four rows per workgroup, reductions by butterflies only
//   block (C >  1024): a 256-thread workgroup per row, the waves' partial results combined through LDS in wave order.  Up to
//                      C = 4096 the row is in registers; above, a first pass keeps a running (max, s, T, D) per thread, the
//                      threads' quadruples are merged, and a second read of the row writes the gradient.
// Determinism: no atomics.  Every sum has an order fixed by (C, form); a second launch of ONE workgroup adds the B row losses in an
// order fixed by B (in double) and OVERWRITES loss[0].  The `deterministic` option has nothing to switch.
#include "common.h"
#include "ce_rows.h"

namespace {

constexpr int CS_THREADS = 256;
constexpr int CS_NR = 16;                              // columns per lane held in registers
constexpr int CS_WAVE_MAXC = 64 * CS_NR;               // 1024: the cut between the wave and the block form
constexpr int CS_REG_MAXC = CS_THREADS * CS_NR;        // 4096: the block form keeps the row in registers up to here
constexpr int CS_UNROLL = 4;                           // streaming pass: columns per thread and step

// ---- the row in registers: G = 64 (C <= 1024, a wave per row) or G = 256 (C <= 4096, a workgroup per row) ------------------------
template <typename TT, int G>
__global__ __launch_bounds__(CS_THREADS) void ce_soft_reg_kernel(const float* __restrict__ probs, int64_t ldp, const TT* __restrict__ target,
                                                                  int64_t ldt, float* __restrict__ row_loss, float* __restrict__ dprobs,
                                                                  int64_t ldd, int64_t B, int C, float inv_b) {
  __shared__ float red[4 * 3];
  constexpr int ROWS = CS_THREADS / G;                 // rows per workgroup
  const int i0 = threadIdx.x % G;                      // this thread's first column
  const int64_t row = (int64_t)blockIdx.x * ROWS + threadIdx.x / G;
  if (row >= B) return;                                // G == 64: a whole wave; G == 256: never (the grid is B)
  const float* p = probs + row * ldp;
  const TT* t = target + row * ldt;
  float pv[CS_NR], tv[CS_NR];
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < CS_NR; ++u) {
    const int j = i0 + u * G;
    const bool in = j < C;
    pv[u] = in ? p[j] : -INFINITY;                     // exp(-inf - mx) = 0: a column beyond C adds nothing
    tv[u] = in ? to_f(t[j]) : 0.f;
    mx = fmaxf(mx, pv[u]);
  }
  mx = group_max<G>(mx, red);
  float acc[3] = {0.f, 0.f, 0.f};                      // s, T, D
#pragma unroll
  for (int u = 0; u < CS_NR; ++u) {
    const bool in = i0 + u * G < C;
    const float e = expf(pv[u] - mx);
    acc[0] += e;
    acc[1] += tv[u];
    acc[2] += in ? tv[u] * (mx - pv[u]) : 0.f;         // 0 * inf otherwise
    pv[u] = e;
  }
  group_sum<G, 3>(acc, red);
  const float s = acc[0], T = acc[1], D = acc[2];
  if (i0 == 0) row_loss[row] = T * logf(s) + D;
  if (dprobs) {
    float* d = dprobs + row * ldd;
    const float ts = T / s;
#pragma unroll
    for (int u = 0; u < CS_NR; ++u) {
      const int j = i0 + u * G;
      if (j < C) d[j] = (ts * pv[u] - tv[u]) * inv_b;
    }
  }
}

// ---- C > 4096: a workgroup per row, two reads of the row ------------------------------------------------------------------------
// a thread's running quadruple over the columns it has seen: m their maximum, s = sum exp(p - m), T = sum t, D = sum t (m - p);
// raising m to mn scales s by exp(m - mn) and adds T (mn - m) to D
struct CsRun { float m, s, T, D; };
__device__ __forceinline__ void cs_raise(CsRun& r, float mn) {
  if (mn > r.m) {                                      // also false for a NaN: it then reaches s through exp(p - m)
    if (r.m != -INFINITY) { r.s *= expf(r.m - mn); r.D += r.T * (mn - r.m); }     // nothing seen yet: s = T = D = 0 stay
    r.m = mn;
  }
}

template <typename TT>
__global__ __launch_bounds__(CS_THREADS) void ce_soft_stream_kernel(const float* __restrict__ probs, int64_t ldp, const TT* __restrict__ target,
                                                                     int64_t ldt, float* __restrict__ row_loss, float* __restrict__ dprobs,
                                                                     int64_t ldd, int C, float inv_b) {
  __shared__ float red[4 * 3];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float* p = probs + row * ldp;
  const TT* t = target + row * ldt;
  CsRun r = {-INFINITY, 0.f, 0.f, 0.f};
  int j = tid;
  for (; j + (CS_UNROLL - 1) * CS_THREADS < C; j += CS_UNROLL * CS_THREADS) {      // four loads of each operand in flight
    float pv[CS_UNROLL], tv[CS_UNROLL];
#pragma unroll
    for (int u = 0; u < CS_UNROLL; ++u) { pv[u] = p[j + u * CS_THREADS]; tv[u] = to_f(t[j + u * CS_THREADS]); }
    cs_raise(r, fmaxf(fmaxf(pv[0], pv[1]), fmaxf(pv[2], pv[3])));
#pragma unroll
    for (int u = 0; u < CS_UNROLL; ++u) { r.s += expf(pv[u] - r.m); r.T += tv[u]; r.D += tv[u] * (r.m - pv[u]); }
  }
  for (; j < C; j += CS_THREADS) {
    const float pv = p[j], tv = to_f(t[j]);
    cs_raise(r, pv);
    r.s += expf(pv - r.m); r.T += tv; r.D += tv * (r.m - pv);
  }
  // C > 4096: every thread has seen at least 16 columns, r.m is one of them
  const float mx = group_max<CS_THREADS>(r.m, red);
  cs_raise(r, mx);
  float acc[3] = {r.s, r.T, r.D};
  group_sum<CS_THREADS, 3>(acc, red);
  const float s = acc[0], T = acc[1], D = acc[2];
  if (tid == 0) row_loss[row] = T * logf(s) + D;
  if (dprobs) {
    float* d = dprobs + row * ldd;
    const float ts = T / s;
    for (j = tid; j < C; j += CS_THREADS) d[j] = (ts * expf(p[j] - mx) - to_f(t[j])) * inv_b;
  }
}

// ---- loss[0] = (sum_b row_loss[b]) / B: one workgroup, thread i adds rows i, i + 256, ... in double, then a fixed tree -------------
__global__ __launch_bounds__(CS_THREADS) void ce_soft_finish_kernel(const float* __restrict__ row_loss, int64_t B, float* __restrict__ loss) {
  __shared__ double part[CS_THREADS];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int64_t b = tid; b < B; b += CS_THREADS) a += (double)row_loss[b];
  part[tid] = a;
  __syncthreads();
#pragma unroll
  for (int o = CS_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)(part[0] / (double)B);
}

bool cs_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

template <typename TT>
void cs_launch(const float* probs, int64_t ldp, const TT* target, int64_t ldt, float* row_loss, float* dprobs, int64_t ldd, int64_t B, int C,
               unsigned grid, hipStream_t st) {
  const float inv_b = 1.0f / (float)B;
  if (C <= CS_WAVE_MAXC)
    hipLaunchKernelGGL((ce_soft_reg_kernel<TT, 64>), dim3(grid), dim3(CS_THREADS), 0, st, probs, ldp, target, ldt, row_loss, dprobs, ldd, B, C, inv_b);
  else if (C <= CS_REG_MAXC)
    hipLaunchKernelGGL((ce_soft_reg_kernel<TT, CS_THREADS>), dim3(grid), dim3(CS_THREADS), 0, st, probs, ldp, target, ldt, row_loss, dprobs, ldd, B,
                       C, inv_b);
  else
    hipLaunchKernelGGL(ce_soft_stream_kernel<TT>, dim3(grid), dim3(CS_THREADS), 0, st, probs, ldp, target, ldt, row_loss, dprobs, ldd, C, inv_b);
}

}  // namespace

extern "C" int meant_ce_probs_soft(const float* probs, int64_t ldp, const void* target, int64_t ldt, int target_dtype, float* row_loss,
                                   float* loss, float* dprobs, int64_t ldd, int64_t B, int64_t C, void* stream) {
  MEANT_REQUIRE(probs && target && row_loss && loss, MEANT_ERR_ARG, "ce_probs_soft: null probs / target / row_loss / loss");
  MEANT_REQUIRE(B > 0 && C > 0 && ldp >= C && ldt >= C && (!dprobs || ldd >= C), MEANT_ERR_ARG,
                "ce_probs_soft: bad argument (B=%lld <= 0, C=%lld <= 0, or one of ldp=%lld, ldt=%lld, ldd=%lld below C)", (long long)B, (long long)C,
                (long long)ldp, (long long)ldt, (long long)ldd);
  MEANT_REQUIRE(target_dtype == MEANT_F32 || target_dtype == MEANT_BF16, MEANT_ERR_ARG, "ce_probs_soft: unknown target dtype %d", target_dtype);
  MEANT_REQUIRE(cs_aligned(probs, 4) && cs_aligned(target, target_dtype == MEANT_F32 ? 4 : 2) && cs_aligned(row_loss, 4) && cs_aligned(loss, 4) &&
                    cs_aligned(dprobs, 4),
                MEANT_ERR_ARG, "ce_probs_soft: operands must be aligned to their element size");
  MEANT_REQUIRE(dprobs != probs, MEANT_ERR_ARG, "ce_probs_soft: dprobs must not alias probs");
  const bool wave = C <= CS_WAVE_MAXC;
  const int64_t grid = wave ? ceil_div(B, CS_THREADS / 64) : B;
  // the kernels index a row's columns in 32 bits, a step of CS_UNROLL * CS_THREADS ahead
  MEANT_REQUIRE(C <= INT32_MAX - CS_UNROLL * CS_THREADS && grid <= INT32_MAX, MEANT_ERR_UNSUPPORTED,
                "ce_probs_soft: B=%lld rows of C=%lld columns need more than 2^31 - 1 workgroups (or columns)", (long long)B, (long long)C);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_DTYPE(target_dtype, TT, cs_launch<TT>(probs, ldp, (const TT*)target, ldt, row_loss, dprobs, ldd, B, (int)C, (unsigned)grid, st));
  MEANT_LAUNCH_CHECK(wave ? "ce_probs_soft (wave)" : "ce_probs_soft (block)");
  hipLaunchKernelGGL(ce_soft_finish_kernel, dim3(1), dim3(CS_THREADS), 0, st, (const float*)row_loss, B, loss);
  MEANT_LAUNCH_CHECK("ce_probs_soft (finish)");
  meant_route_hit(wave ? ROUTE_CE_SOFT_WAVE : ROUTE_CE_SOFT_BLOCK);
  return MEANT_OK;
}
