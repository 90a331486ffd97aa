// Learned softmax pooling of the token axis (src/meant/meant_tweet.py:173,259-261; src/meant/meant_timesformer.py:274,336-338):
//   lang_prep = Linear(d, d) -> LayerNorm(d) -> GELU -> Linear(d, 1) -> Softmax over the sequence;  pooled = sum_s w_s x_s.
// The first Linear is a GEMM the library has.  Behind it, forward:
//   ln_gelu_dot_fwd   score[t] = gelu(LayerNorm(h[t])) . w2 + b2 with the row in registers (the row kernels of norm.hip are the model:
//                     one wave per row for d % 8 == 0 and d <= 2048, the workgroup on a row otherwise); n and a are never written;
//   softmax_pool_fwd  per sequence the softmax of S scores (every column slab of a sequence recomputes it: S floats) and the weighted
//                     sum over the token rows, laid out as the mean-pool (elementwise.hip, K8) with a weight per row.
// Backward:
//   softmax_pool_bwd  one wave per token row: dx = w dout and the row dot r = x . dout from the one read of x; then a kernel over the
//                     [G, S] floats alone turns the dots into dscore = w (r - sum_t w_t r_t);
//   ln_gelu_dot_bwd   n and a recomputed from h and (mean, rstd); dh = LayerNorm backward of dscore w2 gelu'(n); the column sums
//                     dgamma, dbeta, dw2 as norm.hip makes dgamma / dbeta: a partial row per workgroup, reduced in a fixed order.
// HBM-bound streaming kernels; fp32 math on T storage; ordered sums, no atomics: two runs give the same bits.
#include <initializer_list>
#include <type_traits>

#include "internal.h"

namespace {

constexpr int SP_THREADS = 256;        // 4 waves
constexpr int SP_MAXC = 4;             // chunks of 8 per lane kept in registers, one wave per row -> d <= 2048
constexpr int SP_WIDE_SLICE = 8192;    // elements of a row the workgroup keeps in registers at a time
constexpr int SP_MAX_BLOCKS = 1024;    // of the row kernels: bounds the backward's partial rows

// GELU by tier, as norm.hip evaluates it: libm erf in the fp32 tier, the rational erfc (|error| 7.5e-8 in Phi) in the bf16 tier
template <typename T> __device__ __forceinline__ float gelu_t(float x);
template <> __device__ __forceinline__ float gelu_t<float>(float x) { return gelu_erf(x); }
template <> __device__ __forceinline__ float gelu_t<bf16>(float x) { return gelu_erf_fast(x); }
// gelu(x) and gelu'(x) from one Phi(x): a = x Phi, a' = Phi + x pdf
template <typename T> __device__ __forceinline__ void gelu_both(float x, float& a, float& da);
template <> __device__ __forceinline__ void gelu_both<float>(float x, float& a, float& da) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
  const float pdf = 0.39894228040143268f * __expf(-0.5f * x * x);
  a = x * cdf;
  da = cdf + x * pdf;
}
template <> __device__ __forceinline__ void gelu_both<bf16>(float x, float& a, float& da) {
  const float phi = gelu_phi_fast(x);
  const float e = __builtin_amdgcn_exp2f(-0.72134752044448170f * x * x);        // exp(-x^2 / 2)
  a = x * phi;
  da = fmaf(x * 0.39894228040143268f, e, phi);
}

// sum / maximum over the workgroup, the same value in every thread (red: 4 floats of LDS); the four waves combine in wave order
__device__ __forceinline__ float sp_block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}
__device__ __forceinline__ float sp_block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return s;
}

// the threads that own a row of the two ln_gelu_dot kernels: a wave (TEAM = 64) or the workgroup (TEAM = 256), as in norm.hip
template <int TEAM> struct SpTeam {
  static_assert(TEAM == 64 || TEAM == SP_THREADS, "a wave or the workgroup");
  static constexpr int PER_BLOCK = SP_THREADS / TEAM;
  static constexpr int SLICE = TEAM == 64 ? SP_MAXC * 512 : SP_WIDE_SLICE;
  static constexpr int BWD_LDS = TEAM == 64 ? PER_BLOCK * 512 : 4;
  static __device__ __forceinline__ int team() { return TEAM == 64 ? (int)threadIdx.x >> 6 : 0; }
  static __device__ __forceinline__ int member() { return TEAM == 64 ? (int)threadIdx.x & 63 : (int)threadIdx.x; }
  static __device__ __forceinline__ int slices(int d) { return TEAM == 64 ? 1 : (d + SLICE - 1) / SLICE; }
  static __device__ __forceinline__ float sum(float v, float* red) {
    if constexpr (TEAM == 64) return wave_sum(v);
    else return sp_block_sum(v, red);
  }
};
template <int V, int TEAM> constexpr int SP_CPT = SpTeam<TEAM>::SLICE / (TEAM * V);
// first column of chunk c of slice s of this thread: member m owns chunks m, m + TEAM, ... of V elements
template <int V, int TEAM> __device__ __forceinline__ int sp_col(int s, int c) {
  return s * SpTeam<TEAM>::SLICE + (SpTeam<TEAM>::member() + c * TEAM) * V;
}
template <typename T, int V> __device__ __forceinline__ void sp_load(const T* p, float (&f)[V]) {
  if constexpr (V == 8) {
    const Vec8<T> v = load8<T>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = v.get(i);
  } else f[0] = to_f(p[0]);
}
template <typename T, int V> __device__ __forceinline__ void sp_store(T* p, const float (&f)[V]) {
  if constexpr (V == 8) {
    Vec8<T> o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o.set(i, f[i]);
    store8<T>(p, o);
  } else p[0] = from_f<T>(f[0]);
}
template <int V> __device__ __forceinline__ void sp_param(const float* p, float (&f)[V]) {
  if constexpr (V == 8) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[i] = a[i]; f[i + 4] = b[i]; }
  } else f[0] = p[0];
}
// chunk c of a workgroup's partial row from its teams' register sums over their rows; called by all threads.  TEAM = 64: the four
// waves' sums added in wave order through LDS (red: [4][512] floats)
template <int V, int TEAM>
__device__ __forceinline__ void sp_partial_row(float* prow, int c, const float (&acc)[V], int d, float* red) {
  using Tm = SpTeam<TEAM>;
  const int col = sp_col<V, TEAM>(0, c);
  if constexpr (TEAM == 64) {
    const int m = Tm::member() * V;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < V; ++i) red[Tm::team() * 512 + m + i] = acc[i];
    __syncthreads();
    if (Tm::team() == 0 && col < d) {
#pragma unroll
      for (int i = 0; i < V; ++i) prow[col + i] = red[m + i] + red[512 + m + i] + red[1024 + m + i] + red[1536 + m + i];
    }
  } else if (col < d) {
#pragma unroll
    for (int i = 0; i < V; ++i) prow[col + i] = acc[i];
  }
}

// ------------------------------------------------------------------------------------------------
// score[row] = sum_j gelu(((h_j - mean) rstd) gamma_j + beta_j) w2_j + b2; stats[row] = (mean, rstd), the variance about the mean in
// a pass of its own over the registers (a row longer than one slice is read again per pass, expected from L2)
template <typename T, int V, int TEAM>
__global__ __launch_bounds__(SP_THREADS) void ln_gelu_dot_fwd_kernel(const T* __restrict__ h, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, const float* __restrict__ w2,
                                                                      const float* __restrict__ b2, float* __restrict__ score,
                                                                      float* __restrict__ stats, int64_t rows, int d, float eps) {
  using Tm = SpTeam<TEAM>;
  __shared__ float red[4];
  constexpr int CPT = SP_CPT<V, TEAM>;
  const int ns = Tm::slices(d);
  const float shift = b2 ? b2[0] : 0.f;
  for (int64_t row = (int64_t)blockIdx.x * Tm::PER_BLOCK + Tm::team(); row < rows; row += (int64_t)gridDim.x * Tm::PER_BLOCK) {
    const T* hr = h + row * d;
    float v[CPT][V];
    float sm = 0.f;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = sp_col<V, TEAM>(s, c);
        if (col < d) {
          sp_load<T, V>(hr + col, v[c]);
#pragma unroll
          for (int i = 0; i < V; ++i) sm += v[c][i];
        }
      }
    }
    const float mean = Tm::sum(sm, red) / (float)d;
    float q = 0.f;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = sp_col<V, TEAM>(s, c);
        if (col < d) {
          if (ns > 1) sp_load<T, V>(hr + col, v[c]);
#pragma unroll
          for (int i = 0; i < V; ++i) { const float t = v[c][i] - mean; q += t * t; }
        }
      }
    }
    const float rstd = rsqrtf(Tm::sum(q, red) / (float)d + eps);
    float dot = 0.f;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = sp_col<V, TEAM>(s, c);
        if (col < d) {
          if (ns > 1) sp_load<T, V>(hr + col, v[c]);
          float g[V], b[V], u[V];
          sp_param<V>(gamma + col, g);
          sp_param<V>(beta + col, b);
          sp_param<V>(w2 + col, u);
#pragma unroll
          for (int i = 0; i < V; ++i) dot += gelu_t<T>((v[c][i] - mean) * rstd * g[i] + b[i]) * u[i];
        }
      }
    }
    dot = Tm::sum(dot, red);
    if (Tm::member() == 0) {
      score[row] = dot + shift;
      stats[row * 2] = mean;
      stats[row * 2 + 1] = rstd;
    }
  }
}

// one chunk of the backward's inputs: x-hat, dn = ds w2 gelu'(n), gamma dn, ds a
template <typename T, int V>
__device__ __forceinline__ void lgd_bwd_in(const T* h, const float* gamma, const float* beta, const float* w2, int64_t off, int col, float mean,
                                           float rstd, float ds, float (&xh)[V], float (&dn)[V], float (&gd)[V], float (&wa)[V]) {
  float hv[V], g[V], b[V], u[V];
  sp_load<T, V>(h + off + col, hv);
  sp_param<V>(gamma + col, g);
  sp_param<V>(beta + col, b);
  sp_param<V>(w2 + col, u);
#pragma unroll
  for (int i = 0; i < V; ++i) {
    xh[i] = (hv[i] - mean) * rstd;
    float a, da;
    gelu_both<T>(xh[i] * g[i] + b[i], a, da);
    dn[i] = ds * u[i] * da;
    gd[i] = dn[i] * g[i];
    wa[i] = ds * a;
  }
}

// dh = rstd (gamma dn - mean_j(gamma dn) - xhat mean_j(gamma dn xhat)); per-block partial rows of dgamma = sum dn xhat, dbeta = sum dn and
// dw2 = sum ds a in partial[3][gridDim][d].  A one-slice row keeps the three sums in registers till the end (sp_partial_row); a longer row
// keeps them in the block's own partial rows (each column read and written by one thread only)
template <typename T, int V, int TEAM>
__global__ __launch_bounds__(SP_THREADS) void ln_gelu_dot_bwd_kernel(const float* __restrict__ dscore, const T* __restrict__ h,
                                                                      const float* __restrict__ stats, const float* __restrict__ gamma,
                                                                      const float* __restrict__ beta, const float* __restrict__ w2,
                                                                      T* __restrict__ dh, float* __restrict__ partial, int64_t rows, int d) {
  using Tm = SpTeam<TEAM>;
  __shared__ float red[Tm::BWD_LDS];
  constexpr int CPT = SP_CPT<V, TEAM>;
  const int ns = Tm::slices(d);
  const bool resident = ns == 1;
  float* grow = partial + (int64_t)blockIdx.x * d;
  float* brow = partial + ((int64_t)gridDim.x + blockIdx.x) * d;
  float* wrow = partial + (2 * (int64_t)gridDim.x + blockIdx.x) * d;
  float ga[CPT][V], ba[CPT][V], wacc[CPT][V];
#pragma unroll
  for (int c = 0; c < CPT; ++c)
#pragma unroll
    for (int i = 0; i < V; ++i) { ga[c][i] = 0.f; ba[c][i] = 0.f; wacc[c][i] = 0.f; }
  if (!resident) {
    for (int s = 0; s < ns; ++s)
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = sp_col<V, TEAM>(s, c);
        if (col < d) {
#pragma unroll
          for (int i = 0; i < V; ++i) { grow[col + i] = 0.f; brow[col + i] = 0.f; wrow[col + i] = 0.f; }
        }
      }
  }
  for (int64_t row = (int64_t)blockIdx.x * Tm::PER_BLOCK + Tm::team(); row < rows; row += (int64_t)gridDim.x * Tm::PER_BLOCK) {
    const int64_t off = row * d;
    const float mean = stats[row * 2], rstd = stats[row * 2 + 1], ds = dscore[row];
    float xh[CPT][V], gd[CPT][V];
    float s1 = 0.f, s2 = 0.f;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = sp_col<V, TEAM>(s, c);
        if (col < d) {
          float dn[V], wa[V];
          lgd_bwd_in<T, V>(h, gamma, beta, w2, off, col, mean, rstd, ds, xh[c], dn, gd[c], wa);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            s1 += gd[c][i];
            s2 += gd[c][i] * xh[c][i];
            if (resident) { ga[c][i] += dn[i] * xh[c][i]; ba[c][i] += dn[i]; wacc[c][i] += wa[i]; }
            else { grow[col + i] += dn[i] * xh[c][i]; brow[col + i] += dn[i]; wrow[col + i] += wa[i]; }
          }
        }
      }
    }
    s1 = Tm::sum(s1, red) / (float)d;
    s2 = Tm::sum(s2, red) / (float)d;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = sp_col<V, TEAM>(s, c);
        if (col < d) {
          if (!resident) {
            float dn[V], wa[V];
            lgd_bwd_in<T, V>(h, gamma, beta, w2, off, col, mean, rstd, ds, xh[c], dn, gd[c], wa);
          }
          float o[V];
#pragma unroll
          for (int i = 0; i < V; ++i) o[i] = rstd * (gd[c][i] - s1 - xh[c][i] * s2);
          sp_store<T, V>(dh + off + col, o);
        }
      }
    }
  }
  if (resident) {
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      sp_partial_row<V, TEAM>(grow, c, ga[c], d, red);
      sp_partial_row<V, TEAM>(brow, c, ba[c], d, red);
      sp_partial_row<V, TEAM>(wrow, c, wacc[c], d, red);
    }
  }
}

// out_p[j] = sum_b partial[p][b][j] in a fixed order, p = blockIdx.y of three planes.  A workgroup takes 16 columns; its 16 row lanes
// stride the partial rows and are combined through LDS in lane order.
constexpr int SP_RED_COLS = 16, SP_RED_LANES = SP_THREADS / SP_RED_COLS;
__global__ __launch_bounds__(SP_THREADS) void sp_colreduce_kernel(const float* __restrict__ partial, float* __restrict__ out0,
                                                                   float* __restrict__ out1, float* __restrict__ out2, int np, int d) {
  __shared__ float red[SP_RED_LANES][SP_RED_COLS];
  const int cl = threadIdx.x % SP_RED_COLS, rl = threadIdx.x / SP_RED_COLS;
  const int j = blockIdx.x * SP_RED_COLS + cl;
  const float* plane = partial + (int64_t)blockIdx.y * np * d;
  float* out = blockIdx.y == 0 ? out0 : blockIdx.y == 1 ? out1 : out2;
  float s = 0.f;
  if (j < d)
    for (int p = rl; p < np; p += SP_RED_LANES) s += plane[(int64_t)p * d + j];
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && j < d) {
    float t = 0.f;
    for (int l = 0; l < SP_RED_LANES; ++l) t += red[l][cl];
    out[j] = t;
  }
}

// ------------------------------------------------------------------------------------------------
// whether position i of a key mask of the header's MASK_* kinds takes part (0 = left out); a null mask keeps everything
__device__ __forceinline__ bool sp_keep(const void* mask, int kind, int64_t i) {
  if (!mask) return true;
  switch (kind) {
    case MEANT_MASK_F32: return ((const float*)mask)[i] != 0.f;
    case MEANT_MASK_BF16: return (float)((const bf16*)mask)[i] != 0.f;
    case MEANT_MASK_I64: return ((const int64_t*)mask)[i] != 0;
    case MEANT_MASK_U8: return ((const unsigned char*)mask)[i] != 0;
    default: return ((const int32_t*)mask)[i] != 0;
  }
}

// block = (g, 256-column slab): 32 chunks x 8 row groups, as the mean-pool.  Every slab of a sequence computes the same softmax
// statistics (m, 1 / l) from the S scores by the same instructions -- the same bits -- and slab 0 writes the weights; a row group
// sums w_s x_s over its rows in ascending order, the 8 row groups are combined in ascending order.  A position the mask leaves out
// has w = 0 and its row of x is not read.
template <typename T, typename TO, bool VEC>
__global__ __launch_bounds__(256) void softmax_pool_fwd_kernel(const T* __restrict__ x, const float* __restrict__ score,
                                                                const void* __restrict__ key_mask, int mask_kind, float* __restrict__ w,
                                                                TO* __restrict__ out, int64_t ld_out, int64_t col_off, int S, int d) {
  __shared__ float red[8][32][9];
  __shared__ float sred[4];
  const int64_t g = blockIdx.x;
  const float* sc = score + g * S;
  float m = -INFINITY;
  for (int s = threadIdx.x; s < S; s += 256)
    if (sp_keep(key_mask, mask_kind, g * S + s)) m = fmaxf(m, sc[s]);
  m = sp_block_max(m, sred);
  float l = 0.f;
  for (int s = threadIdx.x; s < S; s += 256)
    if (sp_keep(key_mask, mask_kind, g * S + s)) l += expf(sc[s] - m);
  l = sp_block_sum(l, sred);
  const float inv = l > 0.f ? 1.0f / l : 0.f;               // every position left out: m = -inf, l = 0, all weights 0
  if (blockIdx.y == 0)
    for (int s = threadIdx.x; s < S; s += 256) w[g * S + s] = sp_keep(key_mask, mask_kind, g * S + s) ? expf(sc[s] - m) * inv : 0.f;
  const int chunk = blockIdx.y * 32 + (threadIdx.x & 31);
  const int rg = threadIdx.x >> 5;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (chunk * 8 < d) {
    const T* base = x + g * (int64_t)S * d + chunk * 8;
    for (int s = rg; s < S; s += 8) {
      if (!sp_keep(key_mask, mask_kind, g * S + s)) continue;
      const float ws = expf(sc[s] - m) * inv;
      const Vec8<T> v = load8n<VEC>(base + (int64_t)s * d, d - chunk * 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = __builtin_fmaf(ws, v.get(k), acc[k]);     // pinned: the same arithmetic in both forms
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) red[rg][threadIdx.x & 31][k] = acc[k];
  __syncthreads();
  if (rg == 0 && chunk * 8 < d) {
    Vec8<TO> o;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) s += red[r][threadIdx.x][k];
      o.set(k, s);
    }
    if (VEC || d - chunk * 8 >= 8) store8n<VEC>(out + g * ld_out + col_off + chunk * 8, o, 8);
    else store8n<VEC>(out + g * ld_out + col_off + chunk * 8, o, d - chunk * 8);
  }
}

// one wave per token row (g, s): dx = w dout, rdot[row] = x . dout (a lane's chunks in order, elements in order, then the butterfly)
template <typename T, typename TO, bool VEC>
__global__ __launch_bounds__(256) void softmax_pool_bwd_rows_kernel(const TO* __restrict__ dout, int64_t ld_out, int64_t col_off,
                                                                     const T* __restrict__ x, const float* __restrict__ w,
                                                                     T* __restrict__ dx, float* __restrict__ rdot, int64_t rows, int S, int d) {
  const int nch = chunks8<VEC>(d);
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    const int64_t g = row / S;
    const float wv = w[row];
    const TO* dr = dout + g * ld_out + col_off;
    float acc = 0.f;
    for (int c = lane; c < nch; c += 64) {
      const int n = d - c * 8;
      const Vec8<T> xv = load8n<VEC, true>(x + row * d + c * 8, n);
      const Vec8<TO> dv = load8n<VEC>(dr + c * 8, n);
      Vec8<T> o;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        acc = __builtin_fmaf(xv.get(k), dv.get(k), acc);     // pinned: left to the compiler, the 16-byte form packs the products and adds them unfused
        o.set(k, wv * dv.get(k));
      }
      store8n<VEC, true>(dx + row * d + c * 8, o, n);
    }
    acc = wave_sum(acc);
    if (lane == 0) rdot[row] = acc;
  }
}

// in place on the row dots: dscore[g, s] = w (r - sum_t w_t r_t), the sum over the positions with w != 0 in a fixed order (a thread's
// positions ascending, the butterfly, the four waves in order); w == 0 gives 0 whatever the row held
__global__ __launch_bounds__(256) void softmax_pool_bwd_score_kernel(const float* __restrict__ w, float* __restrict__ dscore, int S) {
  __shared__ float sred[4];
  const int64_t g = blockIdx.x;
  const float* wg = w + g * S;
  float* rg = dscore + g * S;
  float c = 0.f;
  for (int s = threadIdx.x; s < S; s += 256) {
    const float ws = wg[s];
    if (ws != 0.f) c += ws * rg[s];
  }
  c = sp_block_sum(c, sred);
  for (int s = threadIdx.x; s < S; s += 256) {
    const float ws = wg[s];
    rg[s] = ws != 0.f ? ws * (rg[s] - c) : 0.f;
  }
}

template <typename TS>
__global__ __launch_bounds__(256) void price_cols_kernel(const TS* __restrict__ src, float* __restrict__ out, int64_t ld_out, int64_t col_off,
                                                          int64_t rows, int cols) {
  const int64_t total = rows * cols;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cols;
    out[r * ld_out + col_off + (i - r * cols)] = (float)src[i];
  }
}

// ---- host side ----
inline int sp_blocks(int64_t rows) {
  const int64_t b = ceil_div(rows, 4);
  return (int)(b < 1 ? 1 : (b > SP_MAX_BLOCKS ? SP_MAX_BLOCKS : b));
}
// (V, TEAM) of a row of d elements whose activation pointers allow (vec) 16-byte loads or not: <8, 64>, <8, 256> and <1, 256>
template <int N> using SpInt = std::integral_constant<int, N>;
template <typename F> inline int sp_switch_vt(bool vec, int64_t d, F&& f) {
  return !vec ? f(SpInt<1>{}, SpInt<256>{}) : d <= SP_MAXC * 512 ? f(SpInt<8>{}, SpInt<64>{}) : f(SpInt<8>{}, SpInt<256>{});
}
inline bool sp_dtype_ok(int dtype) { return dtype == MEANT_F32 || dtype == MEANT_BF16; }
// the pool kernels' 16-byte form: as the mean-pool's (d, ld_out and col_off multiples of 8, aligned bases)
inline bool sp_pool_vec(int64_t ld_out, int64_t col_off, int64_t d, std::initializer_list<const void*> ptrs) {
  bool ok = d % 8 == 0 && ld_out % 8 == 0 && col_off % 8 == 0;
  for (const void* p : ptrs) ok = ok && meant_aligned16(p);
  return ok;
}

}  // namespace

#define SP_REQ(c, ...) MEANT_REQUIRE(c, MEANT_ERR_ARG, __VA_ARGS__)

extern "C" int meant_ln_gelu_dot_fwd(const void* h, const float* gamma, const float* beta, const float* w2, const float* b2, float* score,
                                     float* stats, int64_t rows, int64_t d, float eps, int dtype, void* stream) {
  SP_REQ(h && gamma && beta && w2 && score && stats, "ln_gelu_dot_fwd: null pointer");
  SP_REQ(rows > 0 && d > 0 && d < (1LL << 30), "ln_gelu_dot_fwd: bad shape (rows=%lld, d=%lld)", (long long)rows, (long long)d);
  SP_REQ(sp_dtype_ok(dtype), "ln_gelu_dot_fwd: unknown dtype %d", dtype);
  SP_REQ(meant_aligned_elem(h, dtype) && meant_aligned_elem(gamma, MEANT_F32) && meant_aligned_elem(beta, MEANT_F32) &&
             meant_aligned_elem(w2, MEANT_F32) && meant_aligned_elem(score, MEANT_F32) && meant_aligned_elem(stats, MEANT_F32),
         "ln_gelu_dot_fwd: operands must be aligned to their element size");
  const bool vec = d % 8 == 0 && meant_aligned16(h);
  return sp_switch_vt(vec, d, [&](auto v, auto team) -> int {
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((ln_gelu_dot_fwd_kernel<T, v.value, team.value>), dim3(sp_blocks(rows)), dim3(SP_THREADS), 0,
                                                (hipStream_t)stream, (const T*)h, gamma, beta, w2, b2, score, stats, rows, (int)d, eps));
    MEANT_LAUNCH_CHECK("ln_gelu_dot_fwd");
    return MEANT_OK;
  });
}

extern "C" size_t meant_ln_gelu_dot_bwd_ws(int64_t rows, int64_t d) {
  if (rows <= 0 || d <= 0) return 0;
  return (size_t)3 * sp_blocks(rows) * (size_t)d * sizeof(float);
}

extern "C" int meant_ln_gelu_dot_bwd(const float* dscore, const void* h, const float* stats, const float* gamma, const float* beta,
                                     const float* w2, void* dh, float* dgamma, float* dbeta, float* dw2, int64_t rows, int64_t d, int dtype,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  SP_REQ(dscore && h && stats && gamma && beta && w2 && dh && dgamma && dbeta && dw2 && workspace, "ln_gelu_dot_bwd: null pointer");
  SP_REQ(rows > 0 && d > 0 && d < (1LL << 30), "ln_gelu_dot_bwd: bad shape (rows=%lld, d=%lld)", (long long)rows, (long long)d);
  SP_REQ(sp_dtype_ok(dtype), "ln_gelu_dot_bwd: unknown dtype %d", dtype);
  SP_REQ(meant_aligned_elem(h, dtype) && meant_aligned_elem(dh, dtype) && meant_aligned_elem(workspace, MEANT_F32) &&
             meant_aligned_elem(dscore, MEANT_F32) && meant_aligned_elem(stats, MEANT_F32) && meant_aligned_elem(gamma, MEANT_F32) &&
             meant_aligned_elem(beta, MEANT_F32) && meant_aligned_elem(w2, MEANT_F32) && meant_aligned_elem(dgamma, MEANT_F32) &&
             meant_aligned_elem(dbeta, MEANT_F32) && meant_aligned_elem(dw2, MEANT_F32),
         "ln_gelu_dot_bwd: operands must be aligned to their element size");
  MEANT_REQUIRE(workspace_bytes >= meant_ln_gelu_dot_bwd_ws(rows, d), MEANT_ERR_WORKSPACE, "ln_gelu_dot_bwd: workspace too small");
  const bool vec = d % 8 == 0 && meant_aligned16(h) && meant_aligned16(dh);
  const int nb = sp_blocks(rows);
  const int rc = sp_switch_vt(vec, d, [&](auto v, auto team) -> int {
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((ln_gelu_dot_bwd_kernel<T, v.value, team.value>), dim3(nb), dim3(SP_THREADS), 0,
                                                (hipStream_t)stream, dscore, (const T*)h, stats, gamma, beta, w2, (T*)dh, (float*)workspace,
                                                rows, (int)d));
    MEANT_LAUNCH_CHECK("ln_gelu_dot_bwd");
    return MEANT_OK;
  });
  if (rc) return rc;
  hipLaunchKernelGGL(sp_colreduce_kernel, dim3((unsigned)ceil_div(d, (int64_t)SP_RED_COLS), 3), dim3(SP_THREADS), 0, (hipStream_t)stream,
                     (const float*)workspace, dgamma, dbeta, dw2, nb, (int)d);
  MEANT_LAUNCH_CHECK("ln_gelu_dot_bwd: column sums");
  return MEANT_OK;
}

// the three (activation, pooled buffer) storage pairs of the mean-pool
#define SP_POOL_DISPATCH(name, VEC, LAUNCH)                                                                             \
  do {                                                                                                                  \
    if (dtype == MEANT_F32 && out_dtype == MEANT_F32) { using T = float; using TO = float; constexpr bool VEC_ = VEC; LAUNCH; }            \
    else if (dtype == MEANT_BF16 && out_dtype == MEANT_F32) { using T = bf16; using TO = float; constexpr bool VEC_ = VEC; LAUNCH; }       \
    else if (dtype == MEANT_BF16 && out_dtype == MEANT_BF16) { using T = bf16; using TO = bf16; constexpr bool VEC_ = VEC; LAUNCH; }       \
    else { meant_set_error(name ": unsupported dtype combination"); return MEANT_ERR_UNSUPPORTED; }                   \
  } while (0)

extern "C" int meant_softmax_pool_fwd(const void* x, const float* score, const void* key_mask, int mask_kind, float* w, void* out,
                                      int64_t ld_out, int64_t col_off, int64_t G, int64_t S, int64_t d, int dtype, int out_dtype,
                                      void* stream) {
  SP_REQ(x && score && w && out, "softmax_pool_fwd: null pointer");
  SP_REQ(G > 0 && S > 0 && d > 0 && col_off >= 0 && col_off + d <= ld_out, "softmax_pool_fwd: bad shape (G=%lld, S=%lld, d=%lld, col_off=%lld, ld_out=%lld)",
         (long long)G, (long long)S, (long long)d, (long long)col_off, (long long)ld_out);
  SP_REQ(G < 2147483647LL && S < 2147483647LL && d < (1LL << 30), "softmax_pool_fwd: too many groups, rows or columns");
  SP_REQ(sp_dtype_ok(dtype) && sp_dtype_ok(out_dtype), "softmax_pool_fwd: unknown dtype %d / %d", dtype, out_dtype);
  SP_REQ(!key_mask || (mask_kind >= MEANT_MASK_F32 && mask_kind <= MEANT_MASK_I32), "softmax_pool_fwd: unknown mask kind %d", mask_kind);
  const size_t msz = mask_kind == MEANT_MASK_I64 ? 8 : (mask_kind == MEANT_MASK_F32 || mask_kind == MEANT_MASK_I32) ? 4 : mask_kind == MEANT_MASK_BF16 ? 2 : 1;
  SP_REQ(meant_aligned_elem(x, dtype) && meant_aligned_elem(out, out_dtype) && meant_aligned_elem(score, MEANT_F32) && meant_aligned_elem(w, MEANT_F32) &&
             (!key_mask || (reinterpret_cast<uintptr_t>(key_mask) & (msz - 1)) == 0),
         "softmax_pool_fwd: operands must be aligned to their element size");
  const dim3 grid((unsigned)G, (unsigned)ceil_div(d, 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define SP_LAUNCH hipLaunchKernelGGL((softmax_pool_fwd_kernel<T, TO, VEC_>), grid, block, 0, st, (const T*)x, score, key_mask, mask_kind, w, (TO*)out, ld_out, col_off, (int)S, (int)d)
  if (sp_pool_vec(ld_out, col_off, d, {x, out})) SP_POOL_DISPATCH("softmax_pool_fwd", true, SP_LAUNCH);
  else SP_POOL_DISPATCH("softmax_pool_fwd", false, SP_LAUNCH);
#undef SP_LAUNCH
  MEANT_LAUNCH_CHECK("softmax_pool_fwd");
  return MEANT_OK;
}

extern "C" int meant_softmax_pool_bwd(const void* dout, int64_t ld_out, int64_t col_off, const void* x, const float* w, void* dx, float* dscore,
                                      int64_t G, int64_t S, int64_t d, int dtype, int out_dtype, void* stream) {
  SP_REQ(dout && x && w && dx && dscore, "softmax_pool_bwd: null pointer");
  SP_REQ(G > 0 && S > 0 && d > 0 && col_off >= 0 && col_off + d <= ld_out, "softmax_pool_bwd: bad shape (G=%lld, S=%lld, d=%lld, col_off=%lld, ld_out=%lld)",
         (long long)G, (long long)S, (long long)d, (long long)col_off, (long long)ld_out);
  SP_REQ(G < 2147483647LL && S < 2147483647LL && d < (1LL << 30), "softmax_pool_bwd: too many groups, rows or columns");
  SP_REQ(sp_dtype_ok(dtype) && sp_dtype_ok(out_dtype), "softmax_pool_bwd: unknown dtype %d / %d", dtype, out_dtype);
  SP_REQ(meant_aligned_elem(x, dtype) && meant_aligned_elem(dx, dtype) && meant_aligned_elem(dout, out_dtype) && meant_aligned_elem(w, MEANT_F32) &&
             meant_aligned_elem(dscore, MEANT_F32),
         "softmax_pool_bwd: operands must be aligned to their element size");
  const int64_t rows = G * S;
  const int64_t nb = ceil_div(rows, 4);
  const dim3 grid((unsigned)(nb > 8192 ? 8192 : nb)), block(256);
  hipStream_t st = (hipStream_t)stream;
#define SP_LAUNCH hipLaunchKernelGGL((softmax_pool_bwd_rows_kernel<T, TO, VEC_>), grid, block, 0, st, (const TO*)dout, ld_out, col_off, (const T*)x, w, (T*)dx, dscore, rows, (int)S, (int)d)
  if (sp_pool_vec(ld_out, col_off, d, {dout, x, dx})) SP_POOL_DISPATCH("softmax_pool_bwd", true, SP_LAUNCH);
  else SP_POOL_DISPATCH("softmax_pool_bwd", false, SP_LAUNCH);
#undef SP_LAUNCH
  MEANT_LAUNCH_CHECK("softmax_pool_bwd");
  hipLaunchKernelGGL(softmax_pool_bwd_score_kernel, dim3((unsigned)G), block, 0, st, w, dscore, (int)S);
  MEANT_LAUNCH_CHECK("softmax_pool_bwd: scores");
  return MEANT_OK;
}

extern "C" int meant_price_cols(const void* src, int price_dtype, float* out, int64_t ld_out, int64_t col_off, int64_t rows, int64_t cols,
                                void* stream) {
  SP_REQ(src && out, "price_cols: null pointer");
  SP_REQ(rows > 0 && cols > 0 && cols < (1LL << 30) && col_off >= 0 && col_off + cols <= ld_out, "price_cols: bad shape (rows=%lld, cols=%lld, col_off=%lld, ld_out=%lld)",
         (long long)rows, (long long)cols, (long long)col_off, (long long)ld_out);
  SP_REQ(price_dtype >= MEANT_PRICE_F32 && price_dtype <= MEANT_PRICE_F16, "price_cols: unknown price dtype %d", price_dtype);
  const size_t esz = price_dtype == MEANT_PRICE_F64 ? 8 : price_dtype == MEANT_PRICE_F32 ? 4 : 2;
  SP_REQ((reinterpret_cast<uintptr_t>(src) & (esz - 1)) == 0 && meant_aligned_elem(out, MEANT_F32), "price_cols: operands must be aligned to their element size");
  const int64_t nb = ceil_div(rows * cols, 256);
  const dim3 grid((unsigned)(nb > 4096 ? 4096 : nb)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (price_dtype) {
    case MEANT_PRICE_F32: hipLaunchKernelGGL(price_cols_kernel<float>, grid, block, 0, st, (const float*)src, out, ld_out, col_off, rows, (int)cols); break;
    case MEANT_PRICE_BF16: hipLaunchKernelGGL(price_cols_kernel<bf16>, grid, block, 0, st, (const bf16*)src, out, ld_out, col_off, rows, (int)cols); break;
    case MEANT_PRICE_F64: hipLaunchKernelGGL(price_cols_kernel<double>, grid, block, 0, st, (const double*)src, out, ld_out, col_off, rows, (int)cols); break;
    default: hipLaunchKernelGGL(price_cols_kernel<_Float16>, grid, block, 0, st, (const _Float16*)src, out, ld_out, col_off, rows, (int)cols); break;
  }
  MEANT_LAUNCH_CHECK("price_cols");
  return MEANT_OK;
}
