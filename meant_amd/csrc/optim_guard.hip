// Guarded optimizer tail (in_loop_train.py:232-239 under GradScaler, :548-550): gradient statistics, the skip decision, the step
// count and the loss scale in one 64-byte state block ON THE DEVICE (layout: include/meant_hip.h), three kinds of launches over the
// flat fp32 buckets of the gradient reducer and no host read:
//   * meant_grad_stats_f32 -- sum of the finite squares (double) and count of the non-finite elements of a bucket, two launches,
//                             no atomics: a span of consecutive elements per partial, then one workgroup adds the partials in an
//                             order fixed by n.  HBM-bound: 4 B per parameter.
//   * meant_optim_step_f32 -- unscale + clip + Adam / AdamW over a bucket, skipped as a whole when the step holds a non-finite
//                             gradient; bias corrections from the device's own step count.  HBM-bound: 28 B per parameter.
//   * meant_optim_finish   -- one thread: counts the step as taken or skipped and moves the loss scale (torch's _amp_update_scale_).
#include "common.h"

namespace {

constexpr int OG_THREADS = 256;
constexpr int64_t OG_SPAN = 4096;            // elements per partial while n <= OG_SPAN * OG_PARTS_MAX
constexpr int64_t OG_PARTS_MAX = 65536;      // beyond, the span grows in steps of OG_SPAN so that the partials stay within this
constexpr int OG_GRID_CAP = 2048;            // workgroups per launch (8 per CU); a workgroup strides over spans, one partial each

struct OptimState {                          // include/meant_hip.h, "state block"
  double sumsq;
  int64_t nonfinite, steps, skipped;
  float scale;
  int32_t growth_tracker;
  float last_norm;
  int32_t last_skipped;
  int32_t reserved[4];
};
static_assert(sizeof(OptimState) == MEANT_OPTIM_STATE_BYTES, "state block layout");

// span length and number of partials: functions of n alone
inline int64_t og_span(int64_t n) { return OG_SPAN * (n <= OG_SPAN * OG_PARTS_MAX ? 1 : ceil_div(n, OG_SPAN * OG_PARTS_MAX)); }

__device__ __forceinline__ void og_acc(float x, double& s, uint32_t& c) {
  const bool fin = (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u;
  const double d = (double)(fin ? x : 0.f);             // the square of a float is exact in double: overflow is not a case
  s += d * d;
  c += fin ? 0u : 1u;
}

__global__ __launch_bounds__(OG_THREADS) void grad_stats_kernel(const float* __restrict__ g, int64_t n, int64_t span, int64_t nparts,
                                                                double* __restrict__ part_sum, uint32_t* __restrict__ part_cnt) {
  __shared__ double wsum[OG_THREADS / 64];
  __shared__ uint32_t wcnt[OG_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t part = blockIdx.x; part < nparts; part += gridDim.x) {      // wave-uniform: every lane reaches the shuffles and barriers
    const int64_t lo = part * span;
    const int64_t len = (n - lo < span) ? n - lo : span;
    const float* __restrict__ x = g + lo;                                  // lo % 4096 == 0: as aligned as g
    const int64_t nv = len >> 2;
    double s = 0.0;
    uint32_t c = 0;
#pragma unroll 4
    for (int64_t i = tid; i < nv; i += OG_THREADS) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(x + i * 4);
      og_acc(v[0], s, c); og_acc(v[1], s, c); og_acc(v[2], s, c); og_acc(v[3], s, c);
    }
    for (int64_t i = (nv << 2) + tid; i < len; i += OG_THREADS) og_acc(x[i], s, c);     // the n % 4 elements of the last span
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); c += __shfl_xor(c, o, 64); }
    if (lane == 0) { wsum[wave] = s; wcnt[wave] = c; }
    __syncthreads();
    if (tid == 0) {
      part_sum[part] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
      part_cnt[part] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
    }
    __syncthreads();                                                       // wsum / wcnt are reused by the next span
  }
}

// one workgroup: thread t adds the partials [t * per, (t + 1) * per) in index order, then neighbours pair up in index order
__global__ __launch_bounds__(OG_THREADS) void grad_stats_finish_kernel(const double* __restrict__ part_sum, const uint32_t* __restrict__ part_cnt,
                                                                       int64_t nparts, int first, OptimState* __restrict__ st) {
  __shared__ double ps[OG_THREADS];
  __shared__ int64_t pc[OG_THREADS];
  const int tid = threadIdx.x;
  const int64_t per = (nparts + OG_THREADS - 1) / OG_THREADS;
  const int64_t lo = tid * per, hi = lo + per < nparts ? lo + per : nparts;
  double s = 0.0;
  int64_t c = 0;
  for (int64_t k = lo; k < hi; ++k) { s += part_sum[k]; c += (int64_t)part_cnt[k]; }
  ps[tid] = s; pc[tid] = c;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < OG_THREADS; o <<= 1) {
    if ((tid & (2 * o - 1)) == 0) { ps[tid] += ps[tid + o]; pc[tid] += pc[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    if (first) { st->sumsq = ps[0]; st->nonfinite = pc[0]; }
    else { st->sumsq += ps[0]; st->nonfinite += pc[0]; }
  }
}

__device__ __forceinline__ double og_ipow(double b, int64_t t) {          // b^t, t >= 1, by squaring: ~2 log2(t) multiplies
  double r = 1.0;
  while (t) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

// what a step's update needs of the state block: the two factors of the gradient, lr / bc1 and 1 / sqrt(bc2)
struct StepConsts { float f0, f1, step, isb2; int skip; };
__device__ __forceinline__ StepConsts og_step_consts(const OptimState* __restrict__ st, float lr, float b1, float b2, float max_norm,
                                                     int clip_scaled) {
  StepConsts k;
  k.skip = st->nonfinite != 0;
  const int64_t t = st->steps + 1;
  const float bc1 = (float)(1.0 - og_ipow((double)b1, t)), bc2 = (float)(1.0 - og_ipow((double)b2, t));
  const float scale = st->scale == 0.f ? 1.f : st->scale;
  const float inv = 1.f / scale;
  float c = 1.f;
  if (max_norm > 0.f) {
    const double norm = clip_scaled ? sqrt(st->sumsq) : sqrt(st->sumsq) * (double)fabsf(inv);
    const double cd = (double)max_norm / (norm + 1e-6);
    c = cd < 1.0 ? (float)cd : 1.f;
  }
  k.f0 = clip_scaled ? c : inv;
  k.f1 = clip_scaled ? inv : c;
  k.step = lr / bc1;
  k.isb2 = rsqrtf(bc2);
  return k;
}

// KIND MEANT_OPTIM_ADAMW: the arithmetic of adamw_kernel (optim.hip).  MEANT_OPTIM_ADAM: torch.optim.Adam, weight decay as L2
// added to the gradient.  The gradient is read as (g * c) * inv with clip_scaled (clip what backward left, then unscale: the
// reference's order) and as (g * inv) * c without (unscale, then clip): the roundings of the two torch passes, in their order.
template <int KIND>
__global__ __launch_bounds__(OG_THREADS) void optim_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps,
                                                                float wd, float max_norm, int clip_scaled,
                                                                const OptimState* __restrict__ st) {
  // wave-uniform, from scalar loads: once per wave.  Measured against one thread per workgroup computing them for the other waves
  // through LDS, and against a grid of 4096: no difference beyond what separates two processes running the same build
  const StepConsts sc = og_step_consts(st, lr, b1, b2, max_norm, clip_scaled);
  if (sc.skip) return;                                // the whole step is skipped: nothing is stored
  const float f0 = sc.f0, f1 = sc.f1, step = sc.step, isb2 = sc.isb2, decay = KIND == MEANT_OPTIM_ADAMW ? 1.f - lr * wd : 1.f;
  const int64_t nv = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    f32x4 pv = *reinterpret_cast<f32x4*>(p + i * 4), mv = *reinterpret_cast<f32x4*>(m + i * 4), vv = *reinterpret_cast<f32x4*>(v + i * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i * 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float gk = (gv[k] * f0) * f1;
      if (KIND == MEANT_OPTIM_ADAM) gk += wd * pv[k];
      mv[k] = b1 * mv[k] + (1.f - b1) * gk;
      vv[k] = b2 * vv[k] + (1.f - b2) * gk * gk;
      pv[k] = pv[k] * decay - step * mv[k] / (sqrtf(vv[k]) * isb2 + eps);
    }
    *reinterpret_cast<f32x4*>(p + i * 4) = pv;
    *reinterpret_cast<f32x4*>(m + i * 4) = mv;
    *reinterpret_cast<f32x4*>(v + i * 4) = vv;
  }
  for (int64_t i = (nv << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float pk = p[i];
    float gk = (g[i] * f0) * f1;
    if (KIND == MEANT_OPTIM_ADAM) gk += wd * pk;
    const float mk = b1 * m[i] + (1.f - b1) * gk, vk = b2 * v[i] + (1.f - b2) * gk * gk;
    m[i] = mk; v[i] = vk;
    p[i] = pk * decay - step * mk / (sqrtf(vk) * isb2 + eps);
  }
}

__global__ void optim_finish_kernel(OptimState* __restrict__ st, float growth, float backoff, int interval, int dynamic) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float scale = st->scale == 0.f ? 1.f : st->scale;
  if (st->nonfinite != 0) {
    st->skipped += 1;
    st->last_skipped = 1;
    if (dynamic) { st->scale = scale * backoff; st->growth_tracker = 0; }
    return;
  }
  st->steps += 1;
  st->last_skipped = 0;
  st->last_norm = (float)(sqrt(st->sumsq) / (double)fabsf(scale));
  if (dynamic) {
    const int32_t tr = st->growth_tracker + 1;
    if (tr == interval) {
      const float grown = scale * growth;
      if ((__builtin_bit_cast(uint32_t, grown) & 0x7f800000u) != 0x7f800000u) st->scale = grown;
      st->growth_tracker = 0;
    } else {
      st->growth_tracker = tr;
    }
  }
}

inline bool og_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" size_t meant_grad_stats_ws(int64_t n) {
  if (n <= 0) return 0;
  int64_t parts = ceil_div(n, OG_SPAN);
  if (parts > OG_PARTS_MAX) parts = OG_PARTS_MAX;
  return (size_t)((parts * 12 + 15) / 16 * 16);        // a double and a uint32 per partial
}

extern "C" int meant_grad_stats_f32(const float* g, int64_t n, void* state, int first, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  MEANT_REQUIRE(g && state && n >= 0, MEANT_ERR_ARG, "grad_stats_f32: null pointer or n < 0");
  MEANT_REQUIRE(meant_aligned16(g) && og_aligned8(state), MEANT_ERR_ARG, "grad_stats_f32: g needs 16-byte, state 8-byte alignment");
  if (n == 0) return MEANT_OK;
  const size_t need = meant_grad_stats_ws(n);
  MEANT_REQUIRE(workspace && meant_aligned16(workspace), MEANT_ERR_ARG, "grad_stats_f32: null or misaligned workspace");
  MEANT_REQUIRE(workspace_bytes >= need, MEANT_ERR_WORKSPACE, "grad_stats_f32: workspace of %zu bytes needed, %zu given", need,
                workspace_bytes);
  const int64_t span = og_span(n), nparts = ceil_div(n, span);            // nparts <= OG_PARTS_MAX, and nparts * 12 <= need
  double* part_sum = (double*)workspace;
  uint32_t* part_cnt = (uint32_t*)(part_sum + nparts);
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)(nparts < OG_GRID_CAP ? nparts : OG_GRID_CAP);
  hipLaunchKernelGGL(grad_stats_kernel, dim3(grid), dim3(OG_THREADS), 0, st, g, n, span, nparts, part_sum, part_cnt);
  MEANT_LAUNCH_CHECK("grad_stats_f32");
  hipLaunchKernelGGL(grad_stats_finish_kernel, dim3(1), dim3(OG_THREADS), 0, st, (const double*)part_sum, (const uint32_t*)part_cnt, nparts,
                     first, (OptimState*)state);
  MEANT_LAUNCH_CHECK("grad_stats_f32 (finish)");
  meant_route_hit(ROUTE_GRAD_STATS);
  return MEANT_OK;
}

extern "C" int meant_optim_step_f32(float* p, const float* g, float* m, float* v, int64_t n, int kind, float lr, float beta1, float beta2,
                                    float eps, float weight_decay, float max_norm, int clip_scaled, const void* state, void* stream) {
  MEANT_REQUIRE(p && g && m && v && state && n >= 0, MEANT_ERR_ARG, "optim_step_f32: null pointer or n < 0");
  MEANT_REQUIRE(kind == MEANT_OPTIM_ADAMW || kind == MEANT_OPTIM_ADAM, MEANT_ERR_ARG, "optim_step_f32: unknown kind %d", kind);
  MEANT_REQUIRE(meant_aligned16(p) && meant_aligned16(g) && meant_aligned16(m) && meant_aligned16(v) && og_aligned8(state), MEANT_ERR_ARG,
                "optim_step_f32: p, g, m, v need 16-byte, state 8-byte alignment");
  if (n == 0) return MEANT_OK;
  int64_t nb = ceil_div(n, OG_THREADS * 4);
  if (nb > OG_GRID_CAP) nb = OG_GRID_CAP;
  const OptimState* st = (const OptimState*)state;
  if (kind == MEANT_OPTIM_ADAMW)
    hipLaunchKernelGGL(optim_step_kernel<MEANT_OPTIM_ADAMW>, dim3((unsigned)nb), dim3(OG_THREADS), 0, (hipStream_t)stream, p, g, m, v, n, lr,
                       beta1, beta2, eps, weight_decay, max_norm, clip_scaled, st);
  else
    hipLaunchKernelGGL(optim_step_kernel<MEANT_OPTIM_ADAM>, dim3((unsigned)nb), dim3(OG_THREADS), 0, (hipStream_t)stream, p, g, m, v, n, lr,
                       beta1, beta2, eps, weight_decay, max_norm, clip_scaled, st);
  MEANT_LAUNCH_CHECK("optim_step_f32");
  meant_route_hit(ROUTE_OPTIM_STEP);
  return MEANT_OK;
}

extern "C" int meant_optim_finish(void* state, float growth_factor, float backoff_factor, int growth_interval, int dynamic, void* stream) {
  MEANT_REQUIRE(state && og_aligned8(state), MEANT_ERR_ARG, "optim_finish: null or misaligned state");
  MEANT_REQUIRE(!dynamic || growth_interval >= 1, MEANT_ERR_ARG, "optim_finish: growth_interval must be >= 1");
  hipLaunchKernelGGL(optim_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (OptimState*)state, growth_factor, backoff_factor,
                     growth_interval, dynamic);
  MEANT_LAUNCH_CHECK("optim_finish");
  return MEANT_OK;
}
