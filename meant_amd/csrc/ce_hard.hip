// Hard-label cross-entropy with class weights, label smoothing and ignore_index: torch's F.cross_entropy(x, y, weight=w,
// label_smoothing=eps, ignore_index=) for integer targets.  With W = sum_c w_c (w_c = 1 and W = C without weights), a row counts iff
// y != ignore_index && 0 <= y < C, and for a row that counts
//   row_loss = (1 - eps) w_y (-logp_y) + (eps / C) sum_c w_c (-logp_c),   row_w = w_y
//   d row_loss / d x_j = (1 - eps) w_y (p_j - [j == y]) + (eps / C) (W p_j - w_j)
//   loss = sum row_loss / sum row_w  (0 when the denominator is 0)
// Evaluated in the shift-invariant form: M = max_c x_c, S = sum_c exp(x_c - M), -logp_c = log S + (M - x_c), so the smoothing term
// is W log S + D with D = sum_c w_c (M - x_c); no term grows with a shift of the row.  With a = (1 - eps) w_y, b = eps / C and
// A = a + b W the gradient is A exp(x_j - M) / S - (a [j == y] + b w_j).
// A row that does not count is never read, no address is formed from its target, and it gets exact zeros.  A -inf logit is a masked
// column at eps == 0; with eps > 0 it is outside the contract (torch gives inf or NaN there): the kernels take a path without D then.
//   * meant_ce_probs_hard       -- f32 rows [B, ldp] (the class head's Sigmoid output): loss rows and the unnormalised gradient in one
//                                  launch, in the two forms of ce_soft.hip with the target row synthesised from (y, w, eps)
//   * meant_softmax_ce_hard_fwd / _bwd -- f32 / bf16 logits [T, ld >= V] of the vocabulary GEMM, 16-byte loads, one read each
//   * meant_ce_hard_reduce      -- one workgroup: the sums of row_loss and row_w in double in an order fixed by T, the counts of the
//                                  three kinds of rows, loss and 1 / denominator into a device block
// Determinism: no atomics; every sum has an order fixed by the shape.  The `deterministic` option has nothing to switch.
#include "common.h"
#include "ce_rows.h"

namespace {

constexpr int CH_THREADS = 256;
constexpr int CH_NR = 16;                              // columns per lane held in registers
constexpr int CH_WAVE_MAXC = 64 * CH_NR;               // 1024: the cut between the wave and the block form
constexpr int CH_REG_MAXC = CH_THREADS * CH_NR;        // 4096: the block form keeps the row in registers up to here
constexpr int CH_UNROLL = 4;                           // streaming pass: columns per thread and step

__device__ __forceinline__ bool ch_counts(int64_t y, int64_t C, int64_t ignore_index) { return y != ignore_index && y >= 0 && y < C; }

// a thread's running quadruple over the columns it has seen: m their maximum, s = sum exp(x - m), and with SMOOTH W = sum w,
// D = sum w (m - x).  Raising m to mn scales s by exp(m - mn) and adds W (mn - m) to D.  A -inf column adds nothing: s is only
// ever rescaled from a finite maximum, and exp(-inf - 0) = 0 stands in for exp(-inf - -inf) while nothing finite has been seen.
template <bool SMOOTH, bool FAST>
struct ChRun {
  float m = -INFINITY, s = 0.f, W = 0.f, D = 0.f;
  static __device__ __forceinline__ float ex(float v) { return FAST ? __expf(v) : expf(v); }
  __device__ __forceinline__ void raise(float mn) {
    if (mn > m) {                                      // also false for a NaN: it then reaches s through exp(x - m)
      if (m != -INFINITY) {
        s *= ex(m - mn);
        if (SMOOTH) D += W * (mn - m);
      }
      m = mn;
    }
  }
  __device__ __forceinline__ void add(float x, float w) {   // after raise(>= x)
    s += ex(x - (m == -INFINITY ? 0.f : m));
    if (SMOOTH) { W += w; D += w * (m - x); }
  }
  // the workgroup's quadruple, in every thread: all raise to the common maximum, then plain sums in a fixed order
  __device__ __forceinline__ void merge_block(float* red) {
    raise(group_max<CH_THREADS>(m, red));
    float acc[SMOOTH ? 3 : 1];
    acc[0] = s;
    if (SMOOTH) { acc[1] = W; acc[2] = D; }
    group_sum<CH_THREADS, SMOOTH ? 3 : 1>(acc, red);
    s = acc[0];
    if (SMOOTH) { W = acc[1]; D = acc[2]; }
  }
};

// what a row's statistics make of (y, w, eps): the loss and the two coefficients of the gradient
struct ChRow { float loss, A, a; };
template <bool SMOOTH>
__device__ __forceinline__ ChRow ch_row(float M, float logS, float W, float D, float xy, float wy, float eps, float b) {
  ChRow r;
  r.a = (1.f - eps) * wy;
  r.loss = r.a * (logS + (M - xy));
  r.A = r.a;
  if (SMOOTH) { r.loss += b * (W * logS + D); r.A += b * W; }
  return r;
}

// ---- class-head form, the row in registers: G = 64 (C <= 1024, a wave per row) or G = 256 (C <= 4096, a workgroup per row) -------
template <int G, bool SMOOTH>
__global__ __launch_bounds__(CH_THREADS) void ce_hard_reg_kernel(const float* __restrict__ probs, int64_t ldp, const int64_t* __restrict__ target,
                                                                  const float* __restrict__ weight, float eps, int64_t ignore_index,
                                                                  float* __restrict__ row_loss, float* __restrict__ row_w,
                                                                  float* __restrict__ dprobs, int64_t ldd, int64_t B, int C) {
  __shared__ float red[4 * 3];
  constexpr int ROWS = CH_THREADS / G;                 // rows per workgroup
  constexpr int NA = SMOOTH ? 3 : 1;
  const int i0 = threadIdx.x % G;                      // this thread's first column
  const int64_t row = (int64_t)blockIdx.x * ROWS + threadIdx.x / G;
  if (row >= B) return;                                // G == 64: a whole wave; G == 256: never (the grid is B)
  const int64_t y = target[row];
  if (!ch_counts(y, C, ignore_index)) {                // the row's whole group (G == 256: the workgroup, before any barrier)
    if (i0 == 0) { row_loss[row] = 0.f; row_w[row] = 0.f; }
    if (dprobs)
      for (int j = i0; j < C; j += G) dprobs[row * ldd + j] = 0.f;
    return;
  }
  const float* p = probs + row * ldp;
  float pv[CH_NR], wv[SMOOTH ? CH_NR : 1];
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < CH_NR; ++u) {
    const int j = i0 + u * G;
    const bool in = j < C;
    pv[u] = in ? p[j] : -INFINITY;                     // exp(-inf - mx) = 0: a column beyond C adds nothing
    if (SMOOTH) wv[u] = in ? (weight ? weight[j] : 1.f) : 0.f;
    mx = fmaxf(mx, pv[u]);
  }
  mx = group_max<G>(mx, red);
  float acc[NA] = {};                                  // s, W, D
#pragma unroll
  for (int u = 0; u < CH_NR; ++u) {
    const bool in = i0 + u * G < C;
    const float e = expf(pv[u] - mx);
    acc[0] += e;
    if (SMOOTH) {
      acc[1] += wv[u];
      acc[2] += in ? wv[u] * (mx - pv[u]) : 0.f;       // 0 * inf otherwise
    }
    pv[u] = e;
  }
  group_sum<G, NA>(acc, red);
  const float s = acc[0], b = SMOOTH ? eps / (float)C : 0.f;
  const float wy = weight ? weight[y] : 1.f;
  const ChRow r = ch_row<SMOOTH>(mx, logf(s), acc[SMOOTH ? 1 : 0], acc[SMOOTH ? 2 : 0], p[y], wy, eps, b);
  if (i0 == 0) { row_loss[row] = r.loss; row_w[row] = wy; }
  if (dprobs) {
    float* d = dprobs + row * ldd;
    const float As = r.A / s;
#pragma unroll
    for (int u = 0; u < CH_NR; ++u) {
      const int j = i0 + u * G;
      if (j < C) d[j] = As * pv[u] - ((j == y ? r.a : 0.f) + (SMOOTH ? b * wv[u] : 0.f));
    }
  }
}

// ---- class-head form, C > 4096: a workgroup per row, two reads of the row ----------------------------------------------------------
template <bool SMOOTH>
__global__ __launch_bounds__(CH_THREADS) void ce_hard_stream_kernel(const float* __restrict__ probs, int64_t ldp, const int64_t* __restrict__ target,
                                                                     const float* __restrict__ weight, float eps, int64_t ignore_index,
                                                                     float* __restrict__ row_loss, float* __restrict__ row_w,
                                                                     float* __restrict__ dprobs, int64_t ldd, int C) {
  __shared__ float red[4 * 3];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t y = target[row];
  if (!ch_counts(y, C, ignore_index)) {
    if (tid == 0) { row_loss[row] = 0.f; row_w[row] = 0.f; }
    if (dprobs)
      for (int j = tid; j < C; j += CH_THREADS) dprobs[row * ldd + j] = 0.f;
    return;
  }
  const float* p = probs + row * ldp;
  ChRun<SMOOTH, false> r;
  int j = tid;
  for (; j + (CH_UNROLL - 1) * CH_THREADS < C; j += CH_UNROLL * CH_THREADS) {      // four loads of each operand in flight
    float pv[CH_UNROLL], wv[CH_UNROLL];
#pragma unroll
    for (int u = 0; u < CH_UNROLL; ++u) {
      pv[u] = p[j + u * CH_THREADS];
      wv[u] = SMOOTH && weight ? weight[j + u * CH_THREADS] : 1.f;
    }
    r.raise(fmaxf(fmaxf(pv[0], pv[1]), fmaxf(pv[2], pv[3])));
#pragma unroll
    for (int u = 0; u < CH_UNROLL; ++u) r.add(pv[u], wv[u]);
  }
  for (; j < C; j += CH_THREADS) {
    const float pv = p[j];
    r.raise(pv);
    r.add(pv, SMOOTH && weight ? weight[j] : 1.f);
  }
  r.merge_block(red);
  const float b = SMOOTH ? eps / (float)C : 0.f;
  const float wy = weight ? weight[y] : 1.f;
  const ChRow q = ch_row<SMOOTH>(r.m, logf(r.s), r.W, r.D, p[y], wy, eps, b);
  if (tid == 0) { row_loss[row] = q.loss; row_w[row] = wy; }
  if (dprobs) {
    float* d = dprobs + row * ldd;
    const float As = q.A / r.s;
    for (j = tid; j < C; j += CH_THREADS)
      d[j] = As * expf(p[j] - r.m) - ((j == y ? q.a : 0.f) + (SMOOTH ? b * (weight ? weight[j] : 1.f) : 0.f));
  }
}

// ---- large-vocabulary form: a workgroup per row, 16-byte loads, the row read once forward and once backward ------------------------
// stat [T, 4] = (M, log S, A, a) of a row that counts, zeros otherwise
template <typename T, bool SMOOTH>
__global__ __launch_bounds__(CH_THREADS) void ce_hard_vocab_fwd_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ target,
                                                                        const float* __restrict__ weight, float eps, int V,
                                                                        int64_t ignore_index, float* __restrict__ row_loss,
                                                                        float* __restrict__ row_w, float* __restrict__ stat) {
  __shared__ float red[4 * 3];
  const int tid = threadIdx.x;
  const int64_t row = blockIdx.x;
  const int64_t y = target[row];
  if (!ch_counts(y, V, ignore_index)) {
    if (tid == 0) {
      row_loss[row] = 0.f; row_w[row] = 0.f;
      *reinterpret_cast<f32x4*>(stat + 4 * row) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }
  const T* x = logits + row * ld;
  ChRun<SMOOTH, true> r;
  const int nchunk = V >> 3;
  for (int c = tid; c < nchunk; c += CH_THREADS) {
    const Vec8<T> v = load8<T>(x + c * 8);
    Vec8<float> w;
    if (SMOOTH && weight) w = load8<float>(weight + c * 8);
    float cm = v.get(0);
#pragma unroll
    for (int i = 1; i < 8; ++i) cm = fmaxf(cm, v.get(i));
    r.raise(cm);
#pragma unroll
    for (int i = 0; i < 8; ++i) r.add(v.get(i), SMOOTH && weight ? w.get(i) : 1.f);
  }
  for (int j = (nchunk << 3) + tid; j < V; j += CH_THREADS) {   // ragged tail (V = 64001)
    const float xv = to_f(x[j]);
    r.raise(xv);
    r.add(xv, SMOOTH && weight ? weight[j] : 1.f);
  }
  r.merge_block(red);
  if (tid == 0) {
    const float logS = logf(r.s);                      // once per row: the accurate form costs nothing
    const float wy = weight ? weight[y] : 1.f;
    const ChRow q = ch_row<SMOOTH>(r.m, logS, r.W, r.D, to_f(x[y]), wy, eps, SMOOTH ? eps / (float)V : 0.f);
    row_loss[row] = q.loss;
    row_w[row] = wy;
    *reinterpret_cast<f32x4*>(stat + 4 * row) = f32x4{r.m, logS, q.A, q.a};
  }
}

// WCOL: a weight per column enters the gradient (eps > 0 with weights); otherwise the smoothing term subtracts the constant b
template <typename T, bool WCOL>
__global__ __launch_bounds__(CH_THREADS) void ce_hard_vocab_bwd_kernel(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ target,
                                                                        const float* __restrict__ weight, float b, const float* __restrict__ stat,
                                                                        int V, int64_t ignore_index, const float* __restrict__ gscale,
                                                                        T* __restrict__ dlogits) {
  const int64_t row = blockIdx.x;
  const T* x = logits + row * ld;
  T* dx = dlogits + row * ld;
  const int tid = threadIdx.x;
  const int64_t y = target[row];
  const int nchunk_ld = (int)(ld >> 3);                // ld % 8 == 0 (checked by the launcher): covers the padding too
  if (!ch_counts(y, V, ignore_index)) {                // the whole workgroup: zeros, whatever the row holds (it is not read)
    Vec8<T> z;
#pragma unroll
    for (int i = 0; i < 8; ++i) z.set(i, 0.f);
    for (int c = tid; c < nchunk_ld; c += CH_THREADS) store8<T>(dx + c * 8, z);
    return;
  }
  const float g = gscale[0];
  const float LOG2E = 1.4426950408889634f;
  const f32x4 st = *reinterpret_cast<const f32x4*>(stat + 4 * row);
  const float M = st[0], nl2S = -st[1] * LOG2E, A = st[2], a = st[3];
  for (int c = tid; c < nchunk_ld; c += CH_THREADS) {
    const Vec8<T> v = load8<T>(x + c * 8);
    Vec8<T> o;
    if (c * 8 + 8 <= V) {                              // a whole chunk of the vocabulary: all but the last one or two of a row
      Vec8<float> w;
      if (WCOL) w = load8<float>(weight + c * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float sub = (c * 8 + i == y ? a : 0.f) + (WCOL ? b * w.get(i) : b);
        o.set(i, (A * __builtin_amdgcn_exp2f(fmaf(v.get(i) - M, LOG2E, nl2S)) - sub) * g);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int j = c * 8 + i;
        float d = 0.f;
        if (j < V) {
          const float sub = (j == y ? a : 0.f) + (WCOL ? b * weight[j] : b);
          d = (A * __builtin_amdgcn_exp2f(fmaf(v.get(i) - M, LOG2E, nl2S)) - sub) * g;
        }
        o.set(i, d);                                   // the padding: zeros at any gscale and any content
      }
    }
    store8<T>(dx + c * 8, o);
  }
}

// ---- the reduction: one workgroup, thread i takes rows i, i + 256, ... in double, then a fixed tree ---------------------------------
struct ChStats { float loss, gscale; double num, den; int64_t n_counted, n_ignored, n_invalid; };
static_assert(sizeof(ChStats) == MEANT_CE_STATS_BYTES, "the layout include/meant_hip.h documents");

__global__ __launch_bounds__(CH_THREADS) void ce_hard_reduce_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_w,
                                                                     const int64_t* __restrict__ target, int64_t T, int64_t C,
                                                                     int64_t ignore_index, ChStats* __restrict__ stats) {
  __shared__ double part[2][CH_THREADS];
  __shared__ int64_t cnt[3][CH_THREADS];
  const int tid = threadIdx.x;
  double num = 0.0, den = 0.0;
  int64_t n[3] = {0, 0, 0};
  for (int64_t t = tid; t < T; t += CH_THREADS) {
    const int64_t y = target[t];
    if (ch_counts(y, C, ignore_index)) {               // the other rows hold zeros; they are not trusted to
      num += (double)row_loss[t];
      den += (double)row_w[t];
      n[0] += 1;
    } else {
      n[y == ignore_index ? 1 : 2] += 1;
    }
  }
  part[0][tid] = num; part[1][tid] = den;
#pragma unroll
  for (int k = 0; k < 3; ++k) cnt[k][tid] = n[k];
  __syncthreads();
#pragma unroll
  for (int o = CH_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      part[0][tid] += part[0][tid + o]; part[1][tid] += part[1][tid + o];
#pragma unroll
      for (int k = 0; k < 3; ++k) cnt[k][tid] += cnt[k][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double N = part[0][0], Dn = part[1][0];
    ChStats s;
    s.loss = Dn == 0.0 ? 0.f : (float)(N / Dn);
    s.gscale = Dn == 0.0 ? 0.f : (float)(1.0 / Dn);
    s.num = N; s.den = Dn;
    s.n_counted = cnt[0][0]; s.n_ignored = cnt[1][0]; s.n_invalid = cnt[2][0];
    *stats = s;
  }
}

bool ch_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
bool ch_eps_ok(float eps) { return eps >= 0.f && eps <= 1.f; }      // false for a NaN

int ch_reduce(const float* row_loss, const float* row_w, const int64_t* target, int64_t T, int64_t C, int64_t ignore_index, void* stats,
              hipStream_t st) {
  hipLaunchKernelGGL(ce_hard_reduce_kernel, dim3(1), dim3(CH_THREADS), 0, st, row_loss, row_w, target, T, C, ignore_index, (ChStats*)stats);
  MEANT_LAUNCH_CHECK("ce_hard_reduce");
  return MEANT_OK;
}

template <bool SMOOTH>
void ch_launch_probs(const float* probs, int64_t ldp, const int64_t* target, const float* weight, float eps, int64_t ignore_index,
                     float* row_loss, float* row_w, float* dprobs, int64_t ldd, int64_t B, int C, unsigned grid, hipStream_t st) {
  if (C <= CH_WAVE_MAXC)
    hipLaunchKernelGGL((ce_hard_reg_kernel<64, SMOOTH>), dim3(grid), dim3(CH_THREADS), 0, st, probs, ldp, target, weight, eps, ignore_index,
                       row_loss, row_w, dprobs, ldd, B, C);
  else if (C <= CH_REG_MAXC)
    hipLaunchKernelGGL((ce_hard_reg_kernel<CH_THREADS, SMOOTH>), dim3(grid), dim3(CH_THREADS), 0, st, probs, ldp, target, weight, eps,
                       ignore_index, row_loss, row_w, dprobs, ldd, B, C);
  else
    hipLaunchKernelGGL(ce_hard_stream_kernel<SMOOTH>, dim3(grid), dim3(CH_THREADS), 0, st, probs, ldp, target, weight, eps, ignore_index,
                       row_loss, row_w, dprobs, ldd, C);
}

}  // namespace

extern "C" int meant_ce_hard_reduce(const float* row_loss, const float* row_w, const int64_t* target, int64_t T, int64_t C,
                                    int64_t ignore_index, void* stats, void* stream) {
  MEANT_REQUIRE(stats && T >= 0 && C > 0 && (T == 0 || (row_loss && row_w && target)), MEANT_ERR_ARG,
                "ce_hard_reduce: null row_loss / row_w / target / stats, T=%lld < 0 or C=%lld <= 0", (long long)T, (long long)C);
  MEANT_REQUIRE(ch_aligned(row_loss, 4) && ch_aligned(row_w, 4) && ch_aligned(target, 8) && ch_aligned(stats, 8), MEANT_ERR_ARG,
                "ce_hard_reduce: operands must be aligned to their element size (stats: 8 bytes)");
  return ch_reduce(row_loss, row_w, target, T, C, ignore_index, stats, (hipStream_t)stream);
}

extern "C" int meant_ce_probs_hard(const float* probs, int64_t ldp, const int64_t* target, const float* weight, float eps,
                                   int64_t ignore_index, float* row_loss, float* row_w, float* dprobs, int64_t ldd, int64_t B, int64_t C,
                                   void* stats, void* stream) {
  MEANT_REQUIRE(probs && target && row_loss && row_w && stats, MEANT_ERR_ARG, "ce_probs_hard: null probs / target / row_loss / row_w / stats");
  MEANT_REQUIRE(B > 0 && C > 0 && ldp >= C && (!dprobs || ldd >= C), MEANT_ERR_ARG,
                "ce_probs_hard: bad argument (B=%lld <= 0, C=%lld <= 0, or one of ldp=%lld, ldd=%lld below C)", (long long)B, (long long)C,
                (long long)ldp, (long long)ldd);
  MEANT_REQUIRE(ch_eps_ok(eps), MEANT_ERR_ARG, "ce_probs_hard: label smoothing %g outside [0, 1]", (double)eps);
  MEANT_REQUIRE(ch_aligned(probs, 4) && ch_aligned(weight, 4) && ch_aligned(row_loss, 4) && ch_aligned(row_w, 4) && ch_aligned(dprobs, 4) &&
                    ch_aligned(target, 8) && ch_aligned(stats, 8),
                MEANT_ERR_ARG, "ce_probs_hard: operands must be aligned to their element size (stats: 8 bytes)");
  MEANT_REQUIRE(dprobs != probs && row_loss != row_w, MEANT_ERR_ARG, "ce_probs_hard: dprobs must not alias probs, nor row_w row_loss");
  const bool wave = C <= CH_WAVE_MAXC;
  const int64_t grid = wave ? ceil_div(B, CH_THREADS / 64) : B;
  // the kernels index a row's columns in 32 bits, a step of CH_UNROLL * CH_THREADS ahead
  MEANT_REQUIRE(C <= INT32_MAX - CH_UNROLL * CH_THREADS && grid <= INT32_MAX, MEANT_ERR_UNSUPPORTED,
                "ce_probs_hard: B=%lld rows of C=%lld columns need more than 2^31 - 1 workgroups (or columns)", (long long)B, (long long)C);
  hipStream_t st = (hipStream_t)stream;
  if (eps > 0.f)
    ch_launch_probs<true>(probs, ldp, target, weight, eps, ignore_index, row_loss, row_w, dprobs, ldd, B, (int)C, (unsigned)grid, st);
  else
    ch_launch_probs<false>(probs, ldp, target, weight, eps, ignore_index, row_loss, row_w, dprobs, ldd, B, (int)C, (unsigned)grid, st);
  MEANT_LAUNCH_CHECK(wave ? "ce_probs_hard (wave)" : "ce_probs_hard (block)");
  const int rc = ch_reduce(row_loss, row_w, target, B, C, ignore_index, stats, st);
  if (rc) return rc;
  meant_route_hit(wave ? ROUTE_CE_HARD_WAVE : ROUTE_CE_HARD_BLOCK);
  return MEANT_OK;
}

extern "C" int meant_softmax_ce_hard_fwd(const void* logits, int64_t ld, const int64_t* target, const float* weight, float eps, int64_t T,
                                         int64_t V, int64_t ignore_index, float* row_loss, float* row_w, float* stat, void* stats, int dtype,
                                         void* stream) {
  MEANT_REQUIRE(logits && target && row_loss && row_w && stat && stats, MEANT_ERR_ARG, "softmax_ce_hard_fwd: null pointer");
  MEANT_REQUIRE(T >= 0 && V > 0 && V < (1LL << 31) && ld >= V && ld % 8 == 0, MEANT_ERR_ARG,
                "softmax_ce_hard_fwd: need T >= 0, 0 < V <= ld, ld %% 8 == 0 (T=%lld, V=%lld, ld=%lld)", (long long)T, (long long)V, (long long)ld);
  MEANT_REQUIRE(ch_eps_ok(eps), MEANT_ERR_ARG, "softmax_ce_hard_fwd: label smoothing %g outside [0, 1]", (double)eps);
  MEANT_REQUIRE(dtype == MEANT_F32 || dtype == MEANT_BF16, MEANT_ERR_ARG, "softmax_ce_hard_fwd: unknown dtype %d", dtype);
  MEANT_REQUIRE(meant_aligned16(logits) && meant_aligned16(weight) && meant_aligned16(stat) && ch_aligned(row_loss, 4) && ch_aligned(row_w, 4) &&
                    ch_aligned(target, 8) && ch_aligned(stats, 8),
                MEANT_ERR_ARG, "softmax_ce_hard_fwd: logits, weight and stat 16-byte aligned, stats 8, the others to their element size");
  MEANT_REQUIRE(row_loss != row_w, MEANT_ERR_ARG, "softmax_ce_hard_fwd: row_w must not alias row_loss");
  MEANT_REQUIRE(T <= INT32_MAX, MEANT_ERR_UNSUPPORTED, "softmax_ce_hard_fwd: T=%lld rows need more than 2^31 - 1 workgroups", (long long)T);
  hipStream_t st = (hipStream_t)stream;
  if (T > 0) {
    DISPATCH_DTYPE(dtype, Tt, {
      if (eps > 0.f)
        hipLaunchKernelGGL((ce_hard_vocab_fwd_kernel<Tt, true>), dim3((unsigned)T), dim3(CH_THREADS), 0, st, (const Tt*)logits, ld, target, weight,
                           eps, (int)V, ignore_index, row_loss, row_w, stat);
      else
        hipLaunchKernelGGL((ce_hard_vocab_fwd_kernel<Tt, false>), dim3((unsigned)T), dim3(CH_THREADS), 0, st, (const Tt*)logits, ld, target, weight,
                           eps, (int)V, ignore_index, row_loss, row_w, stat);
    });
    MEANT_LAUNCH_CHECK("softmax_ce_hard_fwd");
    meant_route_hit(ROUTE_CE_HARD_VOCAB);
  }
  return ch_reduce(row_loss, row_w, target, T, V, ignore_index, stats, st);
}

extern "C" int meant_softmax_ce_hard_bwd(const void* logits, int64_t ld, const int64_t* target, const float* weight, float eps,
                                         const float* stat, int64_t T, int64_t V, int64_t ignore_index, const float* gscale, void* dlogits,
                                         int dtype, void* stream) {
  MEANT_REQUIRE(logits && target && stat && gscale && dlogits, MEANT_ERR_ARG, "softmax_ce_hard_bwd: null pointer");
  MEANT_REQUIRE(T >= 0 && V > 0 && V < (1LL << 31) && ld >= V && ld % 8 == 0, MEANT_ERR_ARG,
                "softmax_ce_hard_bwd: need T >= 0, 0 < V <= ld, ld %% 8 == 0 (T=%lld, V=%lld, ld=%lld)", (long long)T, (long long)V, (long long)ld);
  MEANT_REQUIRE(ch_eps_ok(eps), MEANT_ERR_ARG, "softmax_ce_hard_bwd: label smoothing %g outside [0, 1]", (double)eps);
  MEANT_REQUIRE(dtype == MEANT_F32 || dtype == MEANT_BF16, MEANT_ERR_ARG, "softmax_ce_hard_bwd: unknown dtype %d", dtype);
  MEANT_REQUIRE(meant_aligned16(logits) && meant_aligned16(dlogits) && meant_aligned16(weight) && meant_aligned16(stat) && ch_aligned(gscale, 4) &&
                    ch_aligned(target, 8),
                MEANT_ERR_ARG, "softmax_ce_hard_bwd: logits, dlogits, weight and stat 16-byte aligned, the others to their element size");
  MEANT_REQUIRE(T <= INT32_MAX, MEANT_ERR_UNSUPPORTED, "softmax_ce_hard_bwd: T=%lld rows need more than 2^31 - 1 workgroups", (long long)T);
  if (T == 0) return MEANT_OK;
  const float b = eps > 0.f ? eps / (float)V : 0.f;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_DTYPE(dtype, Tt, {
    if (eps > 0.f && weight)
      hipLaunchKernelGGL((ce_hard_vocab_bwd_kernel<Tt, true>), dim3((unsigned)T), dim3(CH_THREADS), 0, st, (const Tt*)logits, ld, target, weight, b,
                         stat, (int)V, ignore_index, gscale, (Tt*)dlogits);
    else
      hipLaunchKernelGGL((ce_hard_vocab_bwd_kernel<Tt, false>), dim3((unsigned)T), dim3(CH_THREADS), 0, st, (const Tt*)logits, ld, target, weight, b,
                         stat, (int)V, ignore_index, gscale, (Tt*)dlogits);
  });
  MEANT_LAUNCH_CHECK("softmax_ce_hard_bwd");
  return MEANT_OK;
}
