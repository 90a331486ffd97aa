// K1: RMSNorm / LayerNorm forward + backward.  HBM-bound streaming kernels.
//   one 64-lane wavefront per row, 16-byte (8-element bf16 / 2x16-byte f32) loads, the row kept in
//   registers between the reduction and the normalisation (one read + one write per element),
//   butterfly reduction over the wave, gain-gradient partials reduced per block then summed by a strip
//   kernel.  The backward optionally folds in the two elementwise passes that surround it in the encoder:
//   the add of the gradient that arrives through the residual branch sharing x, and the GELU derivative
//   when x = gelu(pre) (meant/meant.py:64,107).
// Reference semantics: utils/rms_norm.py:40-57 (eps added to the RMS, outside the sqrt).
#include <type_traits>
#include "internal.h"

namespace {

constexpr int MAXC = 4;               // chunks of 8 per lane kept in registers -> d <= 2048
constexpr int NORM_THREADS = 256;     // 4 waves = 4 rows in flight per block
constexpr int NORM_MAX_BLOCKS = 1024;
constexpr int NORM_PACKED_BLOCKS = 2048;

// exact libm erf in the fp32 tier, the rational erfc (|error| 7.5e-8 in Phi) in the bf16 tier
template <typename T> __device__ __forceinline__ float gelu_grad_t(float x);
template <> __device__ __forceinline__ float gelu_grad_t<float>(float x) { return gelu_erf_grad(x); }
template <> __device__ __forceinline__ float gelu_grad_t<bf16>(float x) { return gelu_erf_grad_fast(x); }

// Phi(x) for every bf16 x with 2^-10 <= |x| < 8 (common.h: phi_slot); each workgroup of a gelu-on-load kernel copies it to LDS
__device__ const float g_phi_tab[2 * PHI_N] = {
#include "phi_table.inc"
};
template <typename T> constexpr bool PHI_TABLE = sizeof(T) == 2;          // bf16 tier only: an fp32 pre-activation has no small domain
// Forward only.  In the backward (two waves per SIMD, nothing to cover the LDS latency of a 64-lane gather, ~10 clocks of bank
// conflicts each) the table measured 10 % SLOWER than the rational form, and a mix of the two (some elements of every 8 by
// table, the rest by arithmetic, to use both pipes) was slower than the table alone in the forward (tools/probe_norm_pooled3.py).
__device__ __forceinline__ void phi_tab_to_lds(float* dst) {
  for (int j = threadIdx.x; j < (int)(2 * PHI_N); j += NORM_THREADS) dst[j] = g_phi_tab[j];
  __syncthreads();
}


// ------------------------------------------------------------------------------------------------
// Packed-row variants for the widths the encoder uses.  One wave takes R consecutive rows as ONE flat run of
// R * d / 8 chunks dealt lane-cyclically, C = R * d / 512 chunks per lane, every lane equally loaded
// (d = 768: R = 2, C = 3 -- one wave per row gives half the lanes two chunks and the other half one), all loads of
// a row group issued before the first use, and twice the waves per CU in flight.
template <typename T, int C>
__global__ __launch_bounds__(NORM_THREADS) void rmsnorm_fwd_packed_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                                           T* __restrict__ y, float* __restrict__ rinv_out,
                                                                           int64_t rows, int d, int R, float eps, float drop_p,
                                                                           uint64_t seed) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = d >> 3;
  const float inv_sqrt_d = rsqrtf((float)d);
  int rsel[C], col[C];                                 // which of the R rows / which column a lane's chunk c belongs to
  f32x4 g0[C], g1[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int k = lane + 64 * c;
    rsel[c] = k / nchunk;
    col[c] = (k - rsel[c] * nchunk) * 8;
    g0[c] = *reinterpret_cast<const f32x4*>(scale + col[c]);
    g1[c] = *reinterpret_cast<const f32x4*>(scale + col[c] + 4);
  }
  const int64_t ngroups = rows / R;
  for (int64_t grp = (int64_t)blockIdx.x * 4 + wave; grp < ngroups; grp += (int64_t)gridDim.x * 4) {
    const int64_t row0 = grp * R;
    const T* xr = x + row0 * d;
    Vec8<T> v[C];
    float ss[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = load8s<T>(xr + (lane + 64 * c) * 8);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      ss[c] = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float f = v[c].get(i); ss[c] += f * f; }
    }
    float rr[C];
#pragma unroll
    for (int c = 0; c < C; ++c) rr[c] = 0.f;
    for (int r = 0; r < R; ++r) {                      // R <= 4 segmented sums
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) s += rsel[c] == r ? ss[c] : 0.f;
      s = wave_sum_dpp(s);
      const float rv = rms_rinv(s, inv_sqrt_d, eps);
      if (lane == 0) rinv_out[row0 + r] = rv;
#pragma unroll
      for (int c = 0; c < C; ++c) rr[c] = rsel[c] == r ? rv : rr[c];
    }
    T* yr = y + row0 * d;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float km[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
      if (drop_p > 0.f) keep_scale8(drop_p, seed, (uint64_t)(row0 + rsel[c]) * d + col[c], km);
      Vec8<T> o;
#pragma unroll
      for (int i = 0; i < 8; ++i) o.set(i, (i < 4 ? g0[c][i] : g1[c][i - 4]) * (v[c].get(i) * rr[c]) * km[i]);
      store8s<T>(yr + (lane + 64 * c) * 8, o);
    }
  }
}

// statistics only: rinv[row] = 1 / (||x_row|| / sqrt(d) + eps), nothing else written (the normalisation itself rides the
// consumer GEMM's epilogue as a per-row factor: meant_linear_fwd_rowscale).  One read of x.
template <typename T, int C>
__global__ __launch_bounds__(NORM_THREADS) void rmsnorm_stats_packed_kernel(const T* __restrict__ x, float* __restrict__ rinv_out,
                                                                             int64_t rows, int d, int R, float eps) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nchunk = d >> 3;
  const float inv_sqrt_d = rsqrtf((float)d);
  int rsel[C];
#pragma unroll
  for (int c = 0; c < C; ++c) rsel[c] = (lane + 64 * c) / nchunk;
  const int64_t ngroups = rows / R;
  for (int64_t grp = (int64_t)blockIdx.x * 4 + wave; grp < ngroups; grp += (int64_t)gridDim.x * 4) {
    const int64_t row0 = grp * R;
    const T* xr = x + row0 * d;
    Vec8<T> v[C];
    float ss[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = load8<T>(xr + (lane + 64 * c) * 8);       // x stays cacheable: the consumer GEMM reads it next
#pragma unroll
    for (int c = 0; c < C; ++c) {
      ss[c] = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) { const float f = v[c].get(i); ss[c] += f * f; }
    }
    for (int r = 0; r < R; ++r) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) s += rsel[c] == r ? ss[c] : 0.f;
      s = wave_sum_dpp(s);
      if (lane == 0) rinv_out[row0 + r] = rms_rinv(s, inv_sqrt_d, eps);
    }
  }
}

// Pooled form: the consumer of this norm (POOL = 1) or of its input (POOL = 2) is the sequence mean-pool (meant/meant.py:231).
// pooled[g, :] (float) = mean over the `group_rows` rows of group g of y (POOL = 1: y itself is not written at all -- it has
// no other reader once the stack's last Linear is evaluated on the pooled features) or of x (POOL = 2: the residual
// operand).  A workgroup owns whole groups: its four waves split a group's rows into four contiguous runs, keep column
// sums in registers, and combine them through LDS in a fixed order -- no atomics, so the forward stays bit-reproducible.
// group_rows is a multiple of R (a wave's step never straddles a group).
// GELU_IN: x holds the PRE-activation h of the Linear + GELU that feeds this norm (meant/meant.py:63-64, :106-107); the
// activation gelu(h), rounded to the storage type as the GEMM epilogue would have stored it, is formed on load, so that
// tensor is never written or read.
template <typename T, int C, int POOL, bool GELU_IN>
__global__ __launch_bounds__(NORM_THREADS) void rmsnorm_fwd_pooled_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                                           T* __restrict__ y, float* __restrict__ rinv_out,
                                                                           int64_t ngroups, int d, int R, float eps, float drop_p,
                                                                           uint64_t seed, float* __restrict__ pooled, int group_rows) {
  __shared__ float red[4][C * 64 * 8];                 // per wave: the column sums of its C * 64 chunks
  __shared__ float phi_s[(GELU_IN && PHI_TABLE<T>) ? 2 * PHI_N : 1];
  if constexpr (GELU_IN && PHI_TABLE<T>) phi_tab_to_lds(phi_s);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nchunk = d >> 3;
  const float inv_sqrt_d = rsqrtf((float)d);
  int rsel[C], col[C];
  f32x4 g0[C], g1[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int k = lane + 64 * c;
    rsel[c] = k / nchunk;
    col[c] = (k - rsel[c] * nchunk) * 8;
    g0[c] = *reinterpret_cast<const f32x4*>(scale + col[c]);
    g1[c] = *reinterpret_cast<const f32x4*>(scale + col[c] + 4);
  }
  const int steps = group_rows / R;                    // steps of R rows per group
  const int per = (steps + 3) / 4;
  const int s_lo = wave * per, s_hi = s_lo + per < steps ? s_lo + per : steps;
  const float inv_group = 1.0f / (float)group_rows;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    float psum[C][8];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int i = 0; i < 8; ++i) psum[c][i] = 0.f;
    for (int st = s_lo; st < s_hi; ++st) {
      const int64_t row0 = g * group_rows + (int64_t)st * R;
      const T* xr = x + row0 * d;
      Vec8<T> v[C];
      float ss[C];
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = load8s<T>(xr + (lane + 64 * c) * 8);
      if (GELU_IN) {
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            if constexpr (PHI_TABLE<T>) v[c].set(i, v[c].get(i) * phi_s[phi_slot(v[c].raw(i))]);
            else v[c].set(i, gelu_erf_fast(v[c].get(i)));
          }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        ss[c] = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float f = v[c].get(i); ss[c] += f * f; }
      }
      float rr[C];
#pragma unroll
      for (int c = 0; c < C; ++c) rr[c] = 0.f;
      for (int r = 0; r < R; ++r) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += rsel[c] == r ? ss[c] : 0.f;
        s = wave_sum_dpp(s);
        const float rv = rms_rinv(s, inv_sqrt_d, eps);
        if (lane == 0) rinv_out[row0 + r] = rv;
#pragma unroll
        for (int c = 0; c < C; ++c) rr[c] = rsel[c] == r ? rv : rr[c];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float km[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
        if (drop_p > 0.f) keep_scale8(drop_p, seed, (uint64_t)(row0 + rsel[c]) * d + col[c], km);
        Vec8<T> o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o.set(i, (i < 4 ? g0[c][i] : g1[c][i - 4]) * (v[c].get(i) * rr[c]) * km[i]);
        if (POOL == 1) {
          // the mean is taken over the values the literal path would have stored, i.e. after rounding to the activation type
#pragma unroll
          for (int i = 0; i < 8; ++i) psum[c][i] += o.get(i);
        } else {
          if (y) store8s<T>(y + row0 * d + (lane + 64 * c) * 8, o);     // y == NULL: statistics + means of x only
#pragma unroll
          for (int i = 0; i < 8; ++i) psum[c][i] += v[c].get(i);
        }
      }
    }
    // fixed-order combine: chunk k = lane + 64 c of wave w holds column (k mod nchunk) * 8 of row k / nchunk
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int i = 0; i < 8; ++i) red[wave][(lane + 64 * c) * 8 + i] = psum[c][i];
    __syncthreads();
    for (int j = threadIdx.x; j < d; j += NORM_THREADS) {
      float s = 0.f;
      for (int w = 0; w < 4; ++w)
        for (int r = 0; r < R; ++r) s += red[w][r * d + j];
      pooled[g * d + j] = s * inv_group;
    }
    __syncthreads();
  }
}

// BC bit 0: dy is the gradient of the POOLED features, float [groups, d]: row r receives dy_g[r / group_rows] / group_rows
// (the backward of POOL = 1 above -- no [tokens, d] broadcast is ever materialised); bit 1: the same for dres (POOL = 2).
// BC bit 2: x is not stored at all -- it is gelu(gelu_pre), formed on load (the forward's GELU_IN)
// CHAIN: the result dpre (gradient of the pre-activation gelu_pre = r_up (x_up W'^T) + b_up of a Linear whose input norm rides
// its GEMM as a per-row factor, meant_linear_fwd_rowscale) is what three more things are made of, all in this pass:
//   dx            <- r_up[row] * dpre : the A operand of BOTH backward GEMMs of that Linear (dW' = (r dpre)^T x_up, and
//                    (r dpre) W' = the first term of d x_up);
//   kcoef[row]    <- rowdot(dpre, pre - b_up) r_up^2 / ((1 - eps_up r_up) d_up): the factor of x_up in the norm's own term,
//                    d x_up = (r dpre) W' - kcoef x_up, which the input-gradient GEMM subtracts in its epilogue;
//   partial2[blk] <- column sums of the UNSCALED dpre (the Linear's bias gradient; the scaled tensor cannot give it).
struct NormChain { const float* up_rinv; const float* up_bias; float* kcoef; float* partial2; float up_eps; int up_d; };
template <typename T, int C, int BC, bool CHAIN = false>
__global__ __launch_bounds__(NORM_THREADS, 2) void rmsnorm_bwd_packed_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                           const float* __restrict__ scale,
                                                                           const float* __restrict__ rinv, T* __restrict__ dx,
                                                                           float* __restrict__ partial, int64_t rows, int d, int R,
                                                                           float eps, float drop_p, uint64_t seed,
                                                                           const T* __restrict__ dres, const T* __restrict__ gelu_pre,
                                                                           int group_rows, NormChain ch = NormChain{}) {
  __shared__ float red[4][C * 64 * 8];                 // per wave: the gain-gradient sums of its C * 64 chunks
  __shared__ float gain_s[CHAIN ? C * 64 * 8 : 1];     // CHAIN: the gains live in LDS (24 registers the extra accumulators need)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float inv_group = BC ? 1.0f / (float)group_rows : 0.f;
  const int nchunk = d >> 3;
  int rsel[C], col[C];
  f32x4 g0[CHAIN ? 1 : C], g1[CHAIN ? 1 : C];
  float gacc[C][8];
  if constexpr (CHAIN) {
    for (int j = threadIdx.x; j < d; j += NORM_THREADS) gain_s[j] = scale[j];
    __syncthreads();
  }
  float bacc[CHAIN ? C : 1][8];                       // CHAIN: column sums of the unscaled result
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int k = lane + 64 * c;
    rsel[c] = k / nchunk;
    col[c] = (k - rsel[c] * nchunk) * 8;
    if constexpr (!CHAIN) {
      g0[c] = *reinterpret_cast<const f32x4*>(scale + col[c]);
      g1[c] = *reinterpret_cast<const f32x4*>(scale + col[c] + 4);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) gacc[c][i] = 0.f;
    if constexpr (CHAIN) {
#pragma unroll
      for (int i = 0; i < 8; ++i) bacc[c][i] = 0.f;
    }
  }
  const int64_t ngroups = rows / R;
  for (int64_t grp = (int64_t)blockIdx.x * 4 + wave; grp < ngroups; grp += (int64_t)gridDim.x * 4) {
    const int64_t row0 = grp * R;
    const int64_t off = row0 * d;
    Vec8<T> xv[C], dv[C], rv[C], pv[C];
    Vec8<float> dvg[C], rvg[C];                        // broadcast (pooled) gradients, fp32
    const int64_t pg = BC ? (int64_t)((unsigned)row0 / (unsigned)group_rows) : 0;   // group of this step's rows (32-bit divide: rows < 2^31 is checked)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int64_t o = off + (lane + 64 * c) * 8;
      if (gelu_pre) pv[c] = load8s<T>(gelu_pre + o);
      if (BC & 4) {                                   // x = pre * Phi(pre) is not stored: keep Phi (x and gelu' are both one multiply-add away)
        if constexpr (!CHAIN) {
#pragma unroll
          for (int i = 0; i < 8; ++i) xv[c].set(i, gelu_phi_fast(pv[c].get(i)));
        }
      } else xv[c] = load8s<T>(x + o);
      if (BC & 1) dvg[c] = load8<float>(reinterpret_cast<const float*>(dy) + pg * d + col[c]);
      else dv[c] = load8s<T>(dy + o);
      if (BC & 2) rvg[c] = load8<float>(reinterpret_cast<const float*>(dres) + pg * d + col[c]);
      else if (dres) rv[c] = load8s<T>(dres + o);
    }
    // CHAIN: three more accumulator sets than the plain kernel have to fit the 256 registers of two waves per SIMD, so the
    // chunks are worked on ONE AFTER THE OTHER (scheduling fences): the fp32 temporaries of one chunk at a time
    if constexpr (CHAIN && (BC & 4) != 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) xv[c].set(i, gelu_phi_fast(pv[c].get(i)));
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    float rr[C], cd[C], gd[C][8];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      rr[c] = rinv[row0 + rsel[c]];
      float km[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
      if (drop_p > 0.f) keep_scale8(drop_p, seed, (uint64_t)(row0 + rsel[c]) * d + col[c], km);
      cd[c] = 0.f;
      f32x4 ga0, ga1;
      if constexpr (CHAIN) {
        ga0 = *reinterpret_cast<const f32x4*>(gain_s + col[c]);
        ga1 = *reinterpret_cast<const f32x4*>(gain_s + col[c] + 4);
      } else { ga0 = g0[c]; ga1 = g1[c]; }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float dyi = ((BC & 1) ? dvg[c].get(i) * inv_group : dv[c].get(i)) * km[i];
        const float xi = (BC & 4) ? pv[c].get(i) * xv[c].get(i) : xv[c].get(i);
        gacc[c][i] += dyi * xi * rr[c];
        const float t = (i < 4 ? ga0[i] : ga1[i - 4]) * dyi;
        gd[c][i] = t;
        cd[c] += t * xi;
      }
      if constexpr (CHAIN) __builtin_amdgcn_sched_barrier(0);
    }
    float kk[C];
#pragma unroll
    for (int c = 0; c < C; ++c) kk[c] = 0.f;
    for (int r = 0; r < R; ++r) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < C; ++c) s += rsel[c] == r ? cd[c] : 0.f;
      s = wave_sum_dpp(s);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        if (rsel[c] == r) {
          const float nsd = (__builtin_amdgcn_rcpf(rr[c]) - eps) * (float)d;          // ||x|| * sqrt(d)
          kk[c] = nsd > 0.f ? s * rr[c] * rr[c] * __builtin_amdgcn_rcpf(nsd) : 0.f;
        }
      }
    }
    float rd[CHAIN ? C : 1], ru[CHAIN ? C : 1];
    if constexpr (CHAIN) {
#pragma unroll
      for (int c = 0; c < C; ++c) ru[c] = ch.up_rinv[row0 + rsel[c]];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      Vec8<T> o;
      f32x4 ub0 = {0.f, 0.f, 0.f, 0.f}, ub1 = ub0;
      if constexpr (CHAIN) {
        rd[c] = 0.f;
        ub0 = *reinterpret_cast<const f32x4*>(ch.up_bias + col[c]);
        ub1 = *reinterpret_cast<const f32x4*>(ch.up_bias + col[c] + 4);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xi2 = (BC & 4) ? pv[c].get(i) * xv[c].get(i) : xv[c].get(i);
        float val = rr[c] * gd[c][i] - kk[c] * xi2;
        if (BC & 2) val += rvg[c].get(i) * inv_group;
        else if (dres) val += rv[c].get(i);
        if (BC & 4) {                                   // gelu'(pre) = Phi + pre * pdf(pre), Phi kept from the first pass
          const float pr = pv[c].get(i);
          val *= fmaf(pr * 0.39894228040143268f, __builtin_amdgcn_exp2f(-0.72134752044448170f * pr * pr), xv[c].get(i));
        } else if (gelu_pre) val *= gelu_grad_t<T>(pv[c].get(i));
        if constexpr (CHAIN) {
          bacc[c][i] += val;
          rd[c] += val * (pv[c].get(i) - (i < 4 ? ub0[i] : ub1[i - 4]));
          o.set(i, val * ru[c]);
        } else o.set(i, val);
      }
      if constexpr (CHAIN) {
        store8<T>(dx + off + (lane + 64 * c) * 8, o);       // read twice right away (dW and dX GEMMs): keep it cacheable
        __builtin_amdgcn_sched_barrier(0);
      } else store8s<T>(dx + off + (lane + 64 * c) * 8, o);
    }
    if constexpr (CHAIN) {
      for (int r = 0; r < R; ++r) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) s += rsel[c] == r ? rd[c] : 0.f;
        s = wave_sum_dpp(s);
        if (lane == 0) {
          const float rv1 = ch.up_rinv[row0 + r];
          const float den = (1.0f - ch.up_eps * rv1) * (float)ch.up_d;      // = ||x_up|| sqrt(d) r
          ch.kcoef[row0 + r] = den > 0.f ? s * rv1 * rv1 / den : 0.f;
        }
      }
    }
  }
  __syncthreads();
  // fixed-order combine (no atomics: the gain gradient is bit-reproducible): chunk k = lane + 64 c of wave w holds column
  // (k mod nchunk) * 8 of row k / nchunk of the wave's R-row steps
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int i = 0; i < 8; ++i) red[wave][(lane + 64 * c) * 8 + i] = gacc[c][i];
  __syncthreads();
  for (int j = threadIdx.x; j < d; j += NORM_THREADS) {
    float s = 0.f;
    for (int w = 0; w < 4; ++w)
      for (int r = 0; r < R; ++r) s += red[w][r * d + j];
    partial[(int64_t)blockIdx.x * d + j] = s;
  }
  if constexpr (CHAIN) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int i = 0; i < 8; ++i) red[wave][(lane + 64 * c) * 8 + i] = bacc[c][i];
    __syncthreads();
    for (int j = threadIdx.x; j < d; j += NORM_THREADS) {
      float s = 0.f;
      for (int w = 0; w < 4; ++w)
        for (int r = 0; r < R; ++r) s += red[w][r * d + j];
      ch.partial2[(int64_t)blockIdx.x * d + j] = s;
    }
  }
}

// out[j] (+)= sum_p partial[p, j] in a FIXED order: the last step of every parameter gradient above.  The kernels keep their sums
// ordered (registers, LDS, one partial row per workgroup); colsum_launch, which the Linear bias gradient uses, would add its row
// strips with float atomics from 65 partial rows on, and the bits of dscale / dbias_up / dgamma / dbeta would change from run to run.
// A workgroup takes COLRED_COLS columns; its row lanes stride the partial rows and are combined through LDS in lane order.
constexpr int COLRED_COLS = 16, COLRED_LANES = NORM_THREADS / COLRED_COLS;
__global__ __launch_bounds__(NORM_THREADS) void colreduce_kernel(const float* __restrict__ partial, float* __restrict__ out, int np, int64_t d,
                                                                  int accumulate) {
  __shared__ float red[COLRED_LANES][COLRED_COLS];
  const int cl = threadIdx.x % COLRED_COLS, rl = threadIdx.x / COLRED_COLS;
  const int64_t j = (int64_t)blockIdx.x * COLRED_COLS + cl;
  float s = 0.f;
  if (j < d)
    for (int p = rl; p < np; p += COLRED_LANES) s += partial[(int64_t)p * d + j];
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && j < d) {
    float t = accumulate ? out[j] : 0.f;
    for (int l = 0; l < COLRED_LANES; ++l) t += red[l][cl];
    out[j] = t;
  }
}

// ------------------------------------------------------------------------------------------------
// The unpacked rows: every shape the packed kernels above do not take, RMSNorm (full, partial, offset, dropout) and LayerNorm,
// forward and backward.  One kernel family; a row belongs to a TEAM of threads, of two sizes:
//   TEAM = 64  (NORM_ROW:  d % 8 == 0 and d <= 2048): one wave per row, the workgroup's four waves on four rows at a time;
//   TEAM = 256 (NORM_WIDE: d > 2048, or d % 8 != 0):  the whole workgroup on one row.
// Grid-stride over rows with at most norm_blocks(rows) workgroups (so the backward's per-block partial rows fit
// meant_rmsnorm_bwd_ws).  Member m of a team owns chunks m, m + TEAM, ... of V elements of a row: V = 8 (16-byte loads) when
// d % 8 == 0; V = 1 otherwise -- a row of such a width is not 16-byte aligned, and these shapes take element loads throughout
// (a correctness route, not a tuned one; TEAM = 256 only).  A slice of Team::SLICE elements is WIDE_CPT chunks per member: a row
// of one slice (TEAM = 64: always; TEAM = 256: d <= 8192) stays in registers between the reduction and the write (one read and
// one write per element); a longer row is read again, slice by slice, for each later pass (expected from L2).  Row sums: a
// thread's chunks in order, elements in order, then wave_sum, and for TEAM = 256 a fixed-order combine of the four waves
// through LDS.  The backward's column sums over a workgroup's rows end in its one partial row (partial_row below).
constexpr int WIDE_SLICE = 8192;
constexpr int64_t NORM_MAX_D = 2147483647LL - WIDE_SLICE;   // the column index of a slice chunk stays an int

// sum over the workgroup, the same value in every thread (red: 4 floats of LDS)
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return s;
}

// the threads that own a row: everything the kernel bodies below need to know about the two sizes
template <int TEAM> struct Team {
  static_assert(TEAM == 64 || TEAM == NORM_THREADS, "a wave or the workgroup");
  static constexpr int PER_BLOCK = NORM_THREADS / TEAM;                 // teams, so rows in flight, per workgroup
  static constexpr int SLICE = TEAM == 64 ? MAXC * 512 : WIDE_SLICE;    // MAXC chunks of 8 per member either way
  static constexpr int SUM_LDS = TEAM == 64 ? 1 : 4;                    // floats sum() needs (TEAM = 64: none, the array is never touched)
  static constexpr int BWD_LDS = TEAM == 64 ? PER_BLOCK * 512 : SUM_LDS;   // floats sum() and partial_row() need
  static __device__ __forceinline__ int team() { return TEAM == 64 ? (int)threadIdx.x >> 6 : 0; }
  static __device__ __forceinline__ int member() { return TEAM == 64 ? (int)threadIdx.x & 63 : (int)threadIdx.x; }
  static __device__ __forceinline__ int slices(int d) { return TEAM == 64 ? 1 : (d + SLICE - 1) / SLICE; }   // TEAM = 64: a constant, no slice loop is compiled
  // sum over the team, the same value in every member
  static __device__ __forceinline__ float sum(float v, float* red) {
    if constexpr (TEAM == 64) return wave_sum(v);
    else return block_sum(v, red);
  }
};
template <int V, int TEAM> constexpr int WIDE_CPT = Team<TEAM>::SLICE / (TEAM * V);

// first column of chunk c of slice s of this thread
template <int V, int TEAM> __device__ __forceinline__ int wide_col(int s, int c) {
  return s * Team<TEAM>::SLICE + (Team<TEAM>::member() + c * TEAM) * V;
}

template <typename T, int V> __device__ __forceinline__ void wide_load(const T* p, float (&f)[V]) {
  if constexpr (V == 8) {
    const Vec8<T> v = load8<T>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = v.get(i);
  } else f[0] = to_f(p[0]);
}
template <typename T, int V> __device__ __forceinline__ void wide_store(T* p, const float (&f)[V]) {
  if constexpr (V == 8) {
    Vec8<T> o;
#pragma unroll
    for (int i = 0; i < 8; ++i) o.set(i, f[i]);
    store8<T>(p, o);
  } else p[0] = from_f<T>(f[0]);
}
// V consecutive fp32 parameters (gain, offset, bias)
template <int V> __device__ __forceinline__ void wide_param(const float* p, float (&f)[V]) {
  if constexpr (V == 8) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[i] = a[i]; f[i + 4] = b[i]; }
  } else f[0] = p[0];
}
// keep-multipliers of the V elements from flat index e by the rule of keep_scale8: element e is decided by the draw for
// e >> 3, its part e & 7, whatever the row's width (V = 8: e is a multiple of 8)
template <int V> __device__ __forceinline__ void wide_keep(float p, uint64_t seed, uint64_t e, float (&m)[V]) {
  if (!(p > 0.f)) {
#pragma unroll
    for (int i = 0; i < V; ++i) m[i] = 1.f;
    return;
  }
  float km[8];
  keep_scale8(p, seed, e & ~7ull, km);
  if constexpr (V == 8) {
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = km[i];
  } else {
    const int q = (int)(e & 7);
    float s = km[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) s = q == j ? km[j] : s;      // a select chain, not a dynamic index into a private array
    m[0] = s;
  }
}
// chunk c of a workgroup's partial row `prow` from its teams' register sums `acc` over their (one-slice) rows; called by all threads.
// TEAM = 256: the one team's sums as they are; TEAM = 64: the four waves' sums added in wave order through LDS (red: [4][512] floats)
template <int V, int TEAM>
__device__ __forceinline__ void partial_row(float* prow, int c, const float (&acc)[V], int d, float* red) {
  using Tm = Team<TEAM>;
  const int col = wide_col<V, TEAM>(0, c);
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

// a chunk of a row as it waits in registers between the RMSNorm forward's statistics and its write: floats, but with one wave per row
// in the storage type -- 16 registers fewer in the bf16 tier, which keeps that kernel at six waves per SIMD (75 VGPRs; 102 with floats)
template <typename T, int V, int TEAM> struct RowChunk {
  float f[V];
  __device__ __forceinline__ void load(const T* p) { wide_load<T, V>(p, f); }
  __device__ __forceinline__ float get(int i) const { return f[i]; }
};
template <typename T> struct RowChunk<T, 8, 64> {
  Vec8<T> v;
  __device__ __forceinline__ void load(const T* p) { v = load8<T>(p); }
  __device__ __forceinline__ float get(int i) const { return v.get(i); }
};

// d_part / offset: the partial and the bias form of utils/rms_norm.py:44-57 (RMSNorm(d, p, bias=True)): the statistics are taken over
// the first d_part = int(d p) elements of a row only (d_part == d: the full-width form the MEANT path uses), and `offset` (float [d],
// may be null) is added to the scaled result.  The offset is loaded like the gain (wide_param): read element by element, its
// 8 addresses per chunk were kept in registers across the row loop, 32 VGPRs that cost the bf16 tier two waves per SIMD.
template <typename T, int V, int TEAM>
__global__ __launch_bounds__(NORM_THREADS) void rmsnorm_fwd_wide_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                                         T* __restrict__ y, float* __restrict__ rinv_out, int64_t rows,
                                                                         int d, float eps, float drop_p, uint64_t seed, int d_part,
                                                                         const float* __restrict__ offset) {
  using Tm = Team<TEAM>;
  __shared__ float red[Tm::SUM_LDS];
  constexpr int CPT = WIDE_CPT<V, TEAM>;
  const int ns = Tm::slices(d);
  const float inv_sqrt_d = rsqrtf((float)d_part);
  for (int64_t row = (int64_t)blockIdx.x * Tm::PER_BLOCK + Tm::team(); row < rows; row += (int64_t)gridDim.x * Tm::PER_BLOCK) {
    const T* xr = x + row * d;
    T* yr = y + row * d;
    RowChunk<T, V, TEAM> v[CPT];
    float ss = 0.f;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
          v[c].load(xr + col);
#pragma unroll
          for (int i = 0; i < V; ++i) ss += col + i < d_part ? v[c].get(i) * v[c].get(i) : 0.f;
        }
      }
    }
    ss = Tm::sum(ss, red);
    const float r = 1.0f / (sqrtf(ss) * inv_sqrt_d + eps);
    if (Tm::member() == 0) rinv_out[row] = r;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
          if (ns > 1) v[c].load(xr + col);
          float g[V], km[V], o[V], ofs[V];
          wide_param<V>(scale + col, g);
          if (offset) wide_param<V>(offset + col, ofs);
          wide_keep<V>(drop_p, seed, (uint64_t)row * d + col, km);
#pragma unroll
          for (int i = 0; i < V; ++i) o[i] = g[i] * (v[c].get(i) * r) * km[i] + (offset ? ofs[i] : 0.f);
          wide_store<T, V>(yr + col, o);
        }
      }
    }
  }
}

// one chunk of the RMSNorm backward's inputs: x, the masked dy, and gain * masked dy
template <typename T, int V>
__device__ __forceinline__ void rms_bwd_in(const T* dy, const T* x, const float* scale, int64_t off, int col, float drop_p, uint64_t seed,
                                           float (&xv)[V], float (&dyv)[V], float (&gd)[V]) {
  float g[V], km[V];
  wide_load<T, V>(x + off + col, xv);
  wide_load<T, V>(dy + off + col, dyv);
  wide_param<V>(scale + col, g);
  wide_keep<V>(drop_p, seed, (uint64_t)off + col, km);
#pragma unroll
  for (int i = 0; i < V; ++i) { dyv[i] *= km[i]; gd[i] = g[i] * dyv[i]; }
}

// dx_j = r * g_j dy_j  -  x_j * c * r^2 / (n sqrt(d)),  c = sum_i g_i dy_i x_i,  n sqrt(d) = (1/r - eps) d
// partial form (d_part < d): the statistics see the first d_part elements only, so the second term exists for j < d_part alone and
// n sqrt(d_part) = (1/r - eps) d_part; partial_off (OFF): per-block column sums of dy, the gradient of the offset.
// dres: the gradient that arrives through the residual branch sharing x; gelu_pre: x = gelu(pre), chained through the activation
// in the same pass.  The gain (and offset) gradient sums of a team's rows stay in registers for a one-slice row and end in the
// block's partial row through partial_row; for a longer row they are kept in the block's own partial row itself (each column
// read and written by one thread only, no atomics)
template <typename T, int V, int TEAM, bool OFF>
__global__ __launch_bounds__(NORM_THREADS) void rmsnorm_bwd_wide_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                         const float* __restrict__ scale, const float* __restrict__ rinv,
                                                                         T* __restrict__ dx, float* __restrict__ partial, int64_t rows,
                                                                         int d, float eps, float drop_p, uint64_t seed,
                                                                         const T* __restrict__ dres, const T* __restrict__ gelu_pre,
                                                                         int d_part, float* __restrict__ partial_off) {
  using Tm = Team<TEAM>;
  __shared__ float red[Tm::BWD_LDS];
  constexpr int CPT = WIDE_CPT<V, TEAM>;
  const int ns = Tm::slices(d);
  const bool resident = ns == 1;
  float* prow = partial + (int64_t)blockIdx.x * d;
  float* orow = OFF ? partial_off + (int64_t)blockIdx.x * d : nullptr;
  float gacc[CPT][V], oacc[OFF ? CPT : 1][V];
#pragma unroll
  for (int c = 0; c < CPT; ++c)
#pragma unroll
    for (int i = 0; i < V; ++i) { gacc[c][i] = 0.f; if (OFF) oacc[c][i] = 0.f; }
  if (!resident) {
    for (int s = 0; s < ns; ++s)
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
#pragma unroll
          for (int i = 0; i < V; ++i) { prow[col + i] = 0.f; if (OFF) orow[col + i] = 0.f; }
        }
      }
  }
  for (int64_t row = (int64_t)blockIdx.x * Tm::PER_BLOCK + Tm::team(); row < rows; row += (int64_t)gridDim.x * Tm::PER_BLOCK) {
    const int64_t off = row * d;
    const float r = rinv[row];
    float xv[CPT][V], gd[CPT][V];
    float cdot = 0.f;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
          float dyv[V];
          rms_bwd_in<T, V>(dy, x, scale, off, col, drop_p, seed, xv[c], dyv, gd[c]);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            cdot += gd[c][i] * xv[c][i];
            const float ga = dyv[i] * xv[c][i] * r;
            if (resident) { gacc[c][i] += ga; if (OFF) oacc[c][i] += dyv[i]; }
            else { prow[col + i] += ga; if (OFF) orow[col + i] += dyv[i]; }
          }
        }
      }
    }
    cdot = Tm::sum(cdot, red);
    const float nsd = (1.0f / r - eps) * (float)d_part;     // ||x_part|| * sqrt(d_part)
    const float k = nsd > 0.f ? cdot * r * r / nsd : 0.f;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
          if (!resident) {
            float dyv[V];
            rms_bwd_in<T, V>(dy, x, scale, off, col, drop_p, seed, xv[c], dyv, gd[c]);
          }
          float o[V];
#pragma unroll
          for (int i = 0; i < V; ++i) o[i] = r * gd[c][i] - (col + i < d_part ? k * xv[c][i] : 0.f);
          if (dres) {
            float rv[V];
            wide_load<T, V>(dres + off + col, rv);
#pragma unroll
            for (int i = 0; i < V; ++i) o[i] = from_f<T>(o[i]) + rv[i];       // each folded pass starts from the value its own pass would have read
          }
          if (gelu_pre) {
            float pv[V];
            wide_load<T, V>(gelu_pre + off + col, pv);
#pragma unroll
            for (int i = 0; i < V; ++i) o[i] = from_f<T>(o[i]) * gelu_grad_t<T>(pv[i]);
          }
          wide_store<T, V>(dx + off + col, o);
        }
      }
    }
  }
  if (resident) {
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      partial_row<V, TEAM>(prow, c, gacc[c], d, red);
      if constexpr (OFF) partial_row<V, TEAM>(orow, c, oacc[c], d, red);
    }
  }
}

// stats[row] = (mean, rstd); the variance is taken about the mean in a pass of its own
template <typename T, int V, int TEAM>
__global__ __launch_bounds__(NORM_THREADS) void layernorm_fwd_wide_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                                           const float* __restrict__ beta, T* __restrict__ y,
                                                                           float* __restrict__ stats, int64_t rows, int d, float eps) {
  using Tm = Team<TEAM>;
  __shared__ float red[Tm::SUM_LDS];
  constexpr int CPT = WIDE_CPT<V, TEAM>;
  const int ns = Tm::slices(d);
  for (int64_t row = (int64_t)blockIdx.x * Tm::PER_BLOCK + Tm::team(); row < rows; row += (int64_t)gridDim.x * Tm::PER_BLOCK) {
    const T* xr = x + row * d;
    T* yr = y + row * d;
    float v[CPT][V];
    float sm = 0.f;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
          wide_load<T, V>(xr + col, v[c]);
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
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
          if (ns > 1) wide_load<T, V>(xr + col, v[c]);
#pragma unroll
          for (int i = 0; i < V; ++i) { const float t = v[c][i] - mean; q += t * t; }
        }
      }
    }
    const float rstd = rsqrtf(Tm::sum(q, red) / (float)d + eps);
    if (Tm::member() == 0) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
          if (ns > 1) wide_load<T, V>(xr + col, v[c]);
          float g[V], b[V], o[V];
          wide_param<V>(gamma + col, g);
          wide_param<V>(beta + col, b);
#pragma unroll
          for (int i = 0; i < V; ++i) o[i] = (v[c][i] - mean) * rstd * g[i] + b[i];
          wide_store<T, V>(yr + col, o);
        }
      }
    }
  }
}

// x * y rounded on its own, never contracted into the add that takes it.  The LayerNorm backward's row sums need it: s1 takes
// gamma * dy and s2 takes (gamma dy) * xhat, both products with other readers, and whether the build fuses them into the sums
// depends on how it packs the two chains -- in the TEAM = 64 form it did, one unit in the last place of dx away from the separate
// one-wave-per-row kernel this body replaced (profiles/norm_team_refactor.txt, section 4).  With the two products pinned, dx keeps those
// bits at both team sizes.  The other a * b + c of these kernels (the ga / gacc updates, gd - s1 - xh * s2) are the compiler's to
// contract; they came out the same at both team sizes, and tools/debug_norm_ab.py against the build before is the check that they still do.
__device__ __forceinline__ float mul_rn(float x, float y) {
#pragma clang fp contract(off)
  return x * y;
}

// one chunk of the LayerNorm backward's inputs: x-hat, dy, gamma * dy
template <typename T, int V>
__device__ __forceinline__ void ln_bwd_in(const T* dy, const T* x, const float* gamma, int64_t off, int col, float mean, float rstd,
                                          float (&xh)[V], float (&dyv)[V], float (&gd)[V]) {
  float xv[V], g[V];
  wide_load<T, V>(x + off + col, xv);
  wide_load<T, V>(dy + off + col, dyv);
  wide_param<V>(gamma + col, g);
#pragma unroll
  for (int i = 0; i < V; ++i) { xh[i] = (xv[i] - mean) * rstd; gd[i] = mul_rn(dyv[i], g[i]); }
}

// dgamma / dbeta partials per block written to partial[2][gridDim][d]; gradient sums as in rmsnorm_bwd_wide_kernel
template <typename T, int V, int TEAM>
__global__ __launch_bounds__(NORM_THREADS) void layernorm_bwd_wide_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                                           const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                           T* __restrict__ dx, float* __restrict__ partial, int64_t rows,
                                                                           int d) {
  using Tm = Team<TEAM>;
  __shared__ float red[Tm::BWD_LDS];
  constexpr int CPT = WIDE_CPT<V, TEAM>;
  const int ns = Tm::slices(d);
  const bool resident = ns == 1;
  float* grow = partial + (int64_t)blockIdx.x * d;
  float* brow = partial + ((int64_t)gridDim.x + blockIdx.x) * d;
  float ga[CPT][V], ba[CPT][V];
#pragma unroll
  for (int c = 0; c < CPT; ++c)
#pragma unroll
    for (int i = 0; i < V; ++i) { ga[c][i] = 0.f; ba[c][i] = 0.f; }
  if (!resident) {
    for (int s = 0; s < ns; ++s)
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
#pragma unroll
          for (int i = 0; i < V; ++i) { grow[col + i] = 0.f; brow[col + i] = 0.f; }
        }
      }
  }
  for (int64_t row = (int64_t)blockIdx.x * Tm::PER_BLOCK + Tm::team(); row < rows; row += (int64_t)gridDim.x * Tm::PER_BLOCK) {
    const int64_t off = row * d;
    const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
    float xh[CPT][V], gd[CPT][V];
    float s1 = 0.f, s2 = 0.f;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
          float dyv[V];
          ln_bwd_in<T, V>(dy, x, gamma, off, col, mean, rstd, xh[c], dyv, gd[c]);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            s1 += gd[c][i];
            s2 += mul_rn(gd[c][i], xh[c][i]);
            if (resident) { ga[c][i] += dyv[i] * xh[c][i]; ba[c][i] += dyv[i]; }
            else { grow[col + i] += dyv[i] * xh[c][i]; brow[col + i] += dyv[i]; }
          }
        }
      }
    }
    s1 = Tm::sum(s1, red) / (float)d;
    s2 = Tm::sum(s2, red) / (float)d;
    for (int s = 0; s < ns; ++s) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) {
        const int col = wide_col<V, TEAM>(s, c);
        if (col < d) {
          if (!resident) {
            float dyv[V];
            ln_bwd_in<T, V>(dy, x, gamma, off, col, mean, rstd, xh[c], dyv, gd[c]);
          }
          float o[V];
#pragma unroll
          for (int i = 0; i < V; ++i) o[i] = rstd * (gd[c][i] - s1 - xh[c][i] * s2);
          wide_store<T, V>(dx + off + col, o);
        }
      }
    }
  }
  if (resident) {
#pragma unroll
    for (int c = 0; c < CPT; ++c) {
      partial_row<V, TEAM>(grow, c, ga[c], d, red);
      partial_row<V, TEAM>(brow, c, ba[c], d, red);
    }
  }
}

// ---- host side: one classifier, one launcher per kernel template, the entry points ------------------------------------------
inline int clamp_blocks(int64_t b, int64_t cap) { return (int)(b < 1 ? 1 : (b > cap ? cap : b)); }
inline int packed_blocks(int64_t groups) { return clamp_blocks(ceil_div(groups, 4), NORM_PACKED_BLOCKS); }
// the packed backward kernels hold two workgroups per CU (205 VGPRs): more than 512 workgroups run in rounds, each paying the
// prologue (gain loads) and the epilogue (LDS reduction of the gain gradient, partial row) again -- at the MLM step's 32 k rows
// the 2048-block launch spent two thirds of its 98 us there
inline int packed_blocks_bwd(int64_t groups) { return clamp_blocks(ceil_div(groups, 4), 2 * (int64_t)meant_num_cus()); }
inline int norm_blocks(int64_t rows) { return clamp_blocks(ceil_div(rows, 4), NORM_MAX_BLOCKS); }
inline size_t dtype_bytes(int dtype) { return dtype == MEANT_BF16 ? 2 : 4; }

// Which kernels a shape runs on; the only place that knows the widths.  NORM_ROW and NORM_WIDE are the two team sizes of the one
// unpacked family (the *_wide_kernel templates, switch_vt below).
//   NORM_WIDE:   d % 8 != 0 or d > MAXC * 512 = 2048: TEAM = 256, one workgroup per row, V = 8 elements per load if d % 8 == 0, else V = 1;
//   NORM_PACKED: R = 1, 2 or 4 rows per wave with R * d / 8 = C * 64 chunks, C <= 3 per lane (so d <= 1536), and rows % R == 0;
//   NORM_ROW:    every other d <= 2048: TEAM = 64, one wave per row, V = 8 (also what a packing shape gets from a caller that cannot pack).
enum NormKind { NORM_PACKED, NORM_ROW, NORM_WIDE };
struct NormRoute { NormKind kind; int R, C, V; };
inline NormRoute norm_route(int64_t rows, int64_t d, bool may_pack = true) {
  if (d % 8 != 0 || d > MAXC * 512) return {NORM_WIDE, 0, 0, d % 8 == 0 ? 8 : 1};
  const int nchunk = (int)(d >> 3);
  for (int R = 1; may_pack && rows > 0 && d > 0 && R <= 4; R *= 2)
    if ((R * nchunk) % 64 == 0 && R * nchunk / 64 <= 3 && rows % R == 0) return {NORM_PACKED, R, R * nchunk / 64, 8};
  return {NORM_ROW, 0, 0, 8};
}
// alignment a route's kernels need of a row pointer: 16 bytes for the 8-element loads, the element's own at V = 1
inline bool norm_aligned(const NormRoute& nr, const void* p, size_t elt) {
  return nr.V == 8 ? meant_aligned16(p) : (reinterpret_cast<uintptr_t>(p) % elt) == 0;
}

// compile-time switches over the chunks per lane C of a packed route and over (V, TEAM) of an unpacked one: f(Int<N>{}...) for
// the runtime value; <8, 64>, <8, 256> and <1, 256> are the only (V, TEAM) instantiated
template <int N> using Int = std::integral_constant<int, N>;
template <typename F> inline int switch_c(int C, F&& f) { return C == 1 ? f(Int<1>{}) : C == 2 ? f(Int<2>{}) : f(Int<3>{}); }
template <typename F> inline int switch_vt(const NormRoute& nr, F&& f) {
  return nr.kind == NORM_ROW ? f(Int<8>{}, Int<64>{}) : nr.V == 8 ? f(Int<8>{}, Int<256>{}) : f(Int<1>{}, Int<256>{});
}

// the ordered reductions of per-block partial rows every backward ends with: out1 from `partial`, out2 (if not null) from the plane after it
inline int norm_colsums(const float* partial, int nb, int64_t d, float* out1, float* out2, int accumulate2, void* stream) {
  const dim3 grid((unsigned)ceil_div(d, (int64_t)COLRED_COLS));
  hipLaunchKernelGGL(colreduce_kernel, grid, dim3(NORM_THREADS), 0, (hipStream_t)stream, partial, out1, nb, d, 0);
  if (out2) hipLaunchKernelGGL(colreduce_kernel, grid, dim3(NORM_THREADS), 0, (hipStream_t)stream, partial + (size_t)nb * d, out2, nb, d, accumulate2);
  MEANT_LAUNCH_CHECK("norm_colsums");
  return MEANT_OK;
}

// ---- launchers: each kernel template is named here and nowhere else ----
inline int launched(const char* name) { MEANT_LAUNCH_CHECK(name); return MEANT_OK; }
// the unpacked forward, one wave or one workgroup per row
int launch_fwd_unpacked(const char* name, const NormRoute& nr, const void* x, const float* scale, void* y, float* rinv, int64_t rows, int64_t d,
                        float eps, float drop_p, uint64_t seed, int64_t d_part, const float* offset, int dtype, void* stream) {
  return switch_vt(nr, [&](auto v, auto team) -> int {
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((rmsnorm_fwd_wide_kernel<T, v.value, team.value>), dim3(norm_blocks(rows)), dim3(NORM_THREADS), 0,
                                                (hipStream_t)stream, (const T*)x, scale, (T*)y, rinv, rows, (int)d, eps, drop_p, seed,
                                                (int)d_part, offset));
    return launched(name);
  });
}

int launch_fwd_packed(const char* name, const NormRoute& nr, const void* x, const float* scale, void* y, float* rinv, int64_t rows, int64_t d,
                      float eps, float drop_p, uint64_t seed, int dtype, void* stream) {
  return switch_c(nr.C, [&](auto c) -> int {
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((rmsnorm_fwd_packed_kernel<T, c.value>), dim3(packed_blocks(rows / nr.R)), dim3(NORM_THREADS), 0,
                                                (hipStream_t)stream, (const T*)x, scale, (T*)y, rinv, rows, (int)d, nr.R, eps, drop_p, seed));
    return launched(name);
  });
}

int launch_stats_packed(const char* name, const NormRoute& nr, const void* x, float* rinv, int64_t rows, int64_t d, float eps, int dtype,
                        void* stream) {
  return switch_c(nr.C, [&](auto c) -> int {
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((rmsnorm_stats_packed_kernel<T, c.value>), dim3(packed_blocks(rows / nr.R)), dim3(NORM_THREADS), 0,
                                                (hipStream_t)stream, (const T*)x, rinv, rows, (int)d, nr.R, eps));
    return launched(name);
  });
}

template <int POOL, bool GELU_IN>
int launch_fwd_pooled(const char* name, const NormRoute& nr, const void* x, const float* scale, void* y, float* rinv, float* pooled,
                      int64_t ngroups, int64_t d, int64_t group_rows, float eps, float drop_p, uint64_t seed, int dtype, void* stream) {
  const int nb = (int)(ngroups < NORM_PACKED_BLOCKS ? ngroups : NORM_PACKED_BLOCKS);
  return switch_c(nr.C, [&](auto c) -> int {
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((rmsnorm_fwd_pooled_kernel<T, c.value, POOL, GELU_IN>), dim3(nb), dim3(NORM_THREADS), 0,
                                                (hipStream_t)stream, (const T*)x, scale, (T*)y, rinv, ngroups, (int)d, nr.R, eps, drop_p, seed,
                                                pooled, (int)group_rows));
    return launched(name);
  });
}

// the plain (BC = 0), pooled (BC = 1, 2, 3, 5) and chained (CHAIN with BC = 0 or 5) packed backward on rows / R groups; the callers'
// explicit <BC, CHAIN> are the only instantiations
template <int BC, bool CHAIN>
int launch_bwd_packed(const char* name, const NormRoute& nr, int nbp, const void* dy, const void* x, const float* scale, const float* rinv,
                      void* dx, float* partial, int64_t rows, int64_t d, float eps, float drop_p, uint64_t seed, const void* dres,
                      const void* gelu_pre, int64_t group_rows, const NormChain& ch, int dtype, void* stream) {
  return switch_c(nr.C, [&](auto c) -> int {
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((rmsnorm_bwd_packed_kernel<T, c.value, BC, CHAIN>), dim3(nbp), dim3(NORM_THREADS), 0,
                                                (hipStream_t)stream, (const T*)dy, (const T*)x, scale, rinv, (T*)dx, partial, rows, (int)d, nr.R,
                                                eps, drop_p, seed, (const T*)dres, (const T*)gelu_pre, (int)group_rows, ch));
    return launched(name);
  });
}

// the unpacked backward; partial_off (may be null): the plane of the offset gradient's partial rows
int launch_bwd_unpacked(const char* name, const NormRoute& nr, int nb, const void* dy, const void* x, const float* scale, const float* rinv,
                        void* dx, float* partial, int64_t rows, int64_t d, float eps, float drop_p, uint64_t seed, const void* dres,
                        const void* gelu_pre, int64_t d_part, float* partial_off, int dtype, void* stream) {
  auto launch = [&](auto v, auto team, auto off) -> int {
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((rmsnorm_bwd_wide_kernel<T, v.value, team.value, off.value>), dim3(nb), dim3(NORM_THREADS), 0,
                                                (hipStream_t)stream, (const T*)dy, (const T*)x, scale, rinv, (T*)dx, partial, rows, (int)d, eps,
                                                drop_p, seed, (const T*)dres, (const T*)gelu_pre, (int)d_part, partial_off));
    return launched(name);
  };
  return switch_vt(nr, [&](auto v, auto team) -> int {
    return partial_off ? launch(v, team, std::true_type{}) : launch(v, team, std::false_type{});
  });
}

int launch_ln_fwd(const char* name, const NormRoute& nr, const void* x, const float* gamma, const float* beta, void* y, float* stats,
                  int64_t rows, int64_t d, float eps, int dtype, void* stream) {
  return switch_vt(nr, [&](auto v, auto team) -> int {
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((layernorm_fwd_wide_kernel<T, v.value, team.value>), dim3(norm_blocks(rows)), dim3(NORM_THREADS), 0,
                                                (hipStream_t)stream, (const T*)x, gamma, beta, (T*)y, stats, rows, (int)d, eps));
    return launched(name);
  });
}

int launch_ln_bwd(const char* name, const NormRoute& nr, int nb, const void* dy, const void* x, const float* gamma, const float* stats, void* dx,
                  float* partial, int64_t rows, int64_t d, int dtype, void* stream) {
  return switch_vt(nr, [&](auto v, auto team) -> int {
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((layernorm_bwd_wide_kernel<T, v.value, team.value>), dim3(nb), dim3(NORM_THREADS), 0,
                                                (hipStream_t)stream, (const T*)dy, (const T*)x, gamma, stats, (T*)dx, partial, rows, (int)d));
    return launched(name);
  });
}

// ---- RMSNorm forward / backward, full and partial form.  The full form (d_part = d, no offset) may pack; the partial one never does. ----
int rmsnorm_fwd_any(const char* name, bool may_pack, const void* x, const float* scale, const float* offset, void* y, float* rinv, int64_t rows,
                    int64_t d, int64_t d_part, float eps, float drop_p, uint64_t seed, int dtype, void* stream) {
  MEANT_REQUIRE(x && scale && y && rinv, MEANT_ERR_ARG, "%s: null pointer", name);
  MEANT_REQUIRE(rows >= 0 && d > 0 && d <= NORM_MAX_D && d_part >= 1 && d_part <= d, MEANT_ERR_UNSUPPORTED,
                "%s: unsupported d=%lld, d_part=%lld: need 1 <= d_part <= d", name, (long long)d, (long long)d_part);
  MEANT_REQUIRE(drop_p >= 0.f && drop_p < 1.f, MEANT_ERR_ARG, "%s: drop_p out of range", name);
  const NormRoute nr = norm_route(rows, d, may_pack);
  const size_t eb = dtype_bytes(dtype);
  MEANT_REQUIRE(norm_aligned(nr, x, eb) && norm_aligned(nr, y, eb) && norm_aligned(nr, scale, 4) && (!offset || norm_aligned(nr, offset, 4)),
                MEANT_ERR_ARG, "%s: alignment", name);      // offset: read in 16-byte loads at V = 8, as the gain is
  if (rows == 0) return MEANT_OK;
  if (nr.kind == NORM_PACKED) return launch_fwd_packed(name, nr, x, scale, y, rinv, rows, d, eps, drop_p, seed, dtype, stream);
  return launch_fwd_unpacked(name, nr, x, scale, y, rinv, rows, d, eps, drop_p, seed, d_part, offset, dtype, stream);
}

// dscale (and doffset, if not null) from the per-block partial rows in `workspace` (meant_rmsnorm_bwd_ws bytes)
int rmsnorm_bwd_any(const char* name, bool may_pack, const void* dy, const void* x, const float* scale, const float* rinv, void* dx, float* dscale,
                    float* doffset, int64_t rows, int64_t d, int64_t d_part, float eps, float drop_p, uint64_t seed, const void* dres,
                    const void* gelu_pre, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  MEANT_REQUIRE(dy && x && scale && rinv && dx && dscale && workspace, MEANT_ERR_ARG, "%s: null pointer", name);
  MEANT_REQUIRE(rows > 0 && d > 0 && d <= NORM_MAX_D && d_part >= 1 && d_part <= d, MEANT_ERR_UNSUPPORTED,
                "%s: unsupported d=%lld, d_part=%lld: need 1 <= d_part <= d", name, (long long)d, (long long)d_part);
  MEANT_REQUIRE(workspace_bytes >= meant_rmsnorm_bwd_ws(rows, d), MEANT_ERR_WORKSPACE, "%s: workspace too small", name);
  const NormRoute nr = norm_route(rows, d, may_pack);
  float* part1 = (float*)workspace;
  if (nr.kind == NORM_PACKED) {
    const int nbp = packed_blocks_bwd(rows / nr.R);
    const int rc = launch_bwd_packed<0, false>(name, nr, nbp, dy, x, scale, rinv, dx, part1, rows, d, eps, drop_p, seed, dres, gelu_pre, 1,
                                                NormChain{}, dtype, stream);
    return rc ? rc : norm_colsums(part1, nbp, d, dscale, nullptr, 0, stream);
  }
  const size_t eb = dtype_bytes(dtype);
  MEANT_REQUIRE(nr.kind != NORM_WIDE || (norm_aligned(nr, dy, eb) && norm_aligned(nr, x, eb) && norm_aligned(nr, dx, eb) && norm_aligned(nr, scale, 4) &&
                                         (!dres || norm_aligned(nr, dres, eb)) && (!gelu_pre || norm_aligned(nr, gelu_pre, eb))),
                MEANT_ERR_ARG, "%s: alignment", name);
  const int nb = norm_blocks(rows);
  const int rc = launch_bwd_unpacked(name, nr, nb, dy, x, scale, rinv, dx, part1, rows, d, eps, drop_p, seed, dres, gelu_pre, d_part,
                                     doffset ? part1 + (size_t)nb * d : nullptr, dtype, stream);
  return rc ? rc : norm_colsums(part1, nb, d, dscale, doffset, 0, stream);
}

}  // namespace

extern "C" size_t meant_rmsnorm_bwd_ws(int64_t rows, int64_t d) {
  const int64_t nb = norm_blocks(rows) > packed_blocks(rows) ? norm_blocks(rows) : packed_blocks(rows);
  return (size_t)nb * d * sizeof(float) * 2;
}

extern "C" int meant_rmsnorm_fwd(const void* x, const float* scale, void* y, float* rinv, int64_t rows, int64_t d,
                                 float eps, float drop_p, uint64_t seed, int dtype, void* stream) {
  return rmsnorm_fwd_any("rmsnorm_fwd", true, x, scale, nullptr, y, rinv, rows, d, d, eps, drop_p, seed, dtype, stream);
}

extern "C" int meant_rmsnorm_bwd(const void* dy, const void* x, const float* scale, const float* rinv, void* dx,
                                 float* dscale, int64_t rows, int64_t d, float eps, float drop_p, uint64_t seed,
                                 const void* dres, const void* gelu_pre, int dtype, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  return rmsnorm_bwd_any("rmsnorm_bwd", true, dy, x, scale, rinv, dx, dscale, nullptr, rows, d, d, eps, drop_p, seed, dres, gelu_pre, dtype,
                         workspace, workspace_bytes, stream);
}

// ---- partial / bias forms of the reference class (utils/rms_norm.py:44-57); not used by any MEANT model, generic kernels ----
extern "C" int meant_rmsnorm_partial_fwd(const void* x, const float* scale, const float* offset, void* y, float* rinv, int64_t rows,
                                         int64_t d, int64_t d_part, float eps, int dtype, void* stream) {
  return rmsnorm_fwd_any("rmsnorm_partial_fwd", false, x, scale, offset, y, rinv, rows, d, d_part, eps, 0.f, 0, dtype, stream);
}

extern "C" int meant_rmsnorm_partial_bwd(const void* dy, const void* x, const float* scale, const float* rinv, void* dx, float* dscale,
                                         float* doffset, int64_t rows, int64_t d, int64_t d_part, float eps, int dtype, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  return rmsnorm_bwd_any("rmsnorm_partial_bwd", false, dy, x, scale, rinv, dx, dscale, doffset, rows, d, d_part, eps, 0.f, 0, nullptr, nullptr,
                         dtype, workspace, workspace_bytes, stream);
}

// ---- pooled forms (the norms whose output or input feeds the sequence mean-pool only) ----
extern "C" int meant_rmsnorm_pooled_ok(int64_t rows, int64_t d, int64_t group_rows) {
  if (group_rows <= 0 || rows % group_rows) return 0;
  const NormRoute nr = norm_route(rows, d);
  return nr.kind == NORM_PACKED && group_rows % nr.R == 0;
}

extern "C" int meant_rmsnorm_fwd_pooled(const void* x, const float* scale, void* y, float* rinv, float* pooled, int64_t rows, int64_t d,
                                        int64_t group_rows, int pool_input, int gelu_input, float eps, float drop_p, uint64_t seed,
                                        int dtype, void* stream) {
  const char* name = "rmsnorm_fwd_pooled";
  MEANT_REQUIRE(x && scale && rinv && pooled, MEANT_ERR_ARG, "rmsnorm_fwd_pooled: null pointer");   // y == NULL with pool_input: statistics + means of x only
  MEANT_REQUIRE(!(pool_input && gelu_input), MEANT_ERR_UNSUPPORTED, "rmsnorm_fwd_pooled: gelu_input goes with pool_input == 0");
  MEANT_REQUIRE(meant_rmsnorm_pooled_ok(rows, d, group_rows), MEANT_ERR_UNSUPPORTED,
                "rmsnorm_fwd_pooled: rows=%lld d=%lld group_rows=%lld is not a packed shape (see meant_rmsnorm_pooled_ok)", (long long)rows,
                (long long)d, (long long)group_rows);
  const NormRoute nr = norm_route(rows, d);
  const size_t eb = dtype_bytes(dtype);
  MEANT_REQUIRE(norm_aligned(nr, x, eb) && norm_aligned(nr, scale, 4) && (!y || norm_aligned(nr, y, eb)), MEANT_ERR_ARG,
                "rmsnorm_fwd_pooled: 16-byte alignment");
  MEANT_REQUIRE(drop_p >= 0.f && drop_p < 1.f, MEANT_ERR_ARG, "rmsnorm_fwd_pooled: drop_p out of range");
  const int64_t ngroups = rows / group_rows;
  if (pool_input) return launch_fwd_pooled<2, false>(name, nr, x, scale, y, rinv, pooled, ngroups, d, group_rows, eps, drop_p, seed, dtype, stream);
  if (gelu_input) return launch_fwd_pooled<1, true>(name, nr, x, scale, y, rinv, pooled, ngroups, d, group_rows, eps, drop_p, seed, dtype, stream);
  return launch_fwd_pooled<1, false>(name, nr, x, scale, y, rinv, pooled, ngroups, d, group_rows, eps, drop_p, seed, dtype, stream);
}

extern "C" int meant_rmsnorm_bwd_pooled(const void* dy, int dy_pooled, const void* x, const float* scale, const float* rinv, void* dx,
                                        float* dscale, int64_t rows, int64_t d, int64_t group_rows, float eps, float drop_p, uint64_t seed,
                                        const void* dres, int dres_pooled, const void* gelu_pre, int dtype, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  MEANT_REQUIRE(dy && (x || gelu_pre) && scale && rinv && dx && dscale && workspace, MEANT_ERR_ARG, "rmsnorm_bwd_pooled: null pointer");
  MEANT_REQUIRE((dy_pooled || dres_pooled) && (!dres_pooled || dres), MEANT_ERR_ARG, "rmsnorm_bwd_pooled: nothing pooled (use meant_rmsnorm_bwd)");
  MEANT_REQUIRE(meant_rmsnorm_pooled_ok(rows, d, group_rows) && rows < 2147483647LL, MEANT_ERR_UNSUPPORTED, "rmsnorm_bwd_pooled: not a packed shape");
  MEANT_REQUIRE(workspace_bytes >= meant_rmsnorm_bwd_ws(rows, d), MEANT_ERR_WORKSPACE, "rmsnorm_bwd_pooled: workspace too small");
  const NormRoute nr = norm_route(rows, d);
  const int nbp = packed_blocks_bwd(rows / nr.R);
  const int bc = (dy_pooled ? 1 : 0) | (dres_pooled ? 2 : 0) | (x ? 0 : 4);
  MEANT_REQUIRE(bc == 1 || bc == 2 || bc == 3 || bc == 5, MEANT_ERR_UNSUPPORTED, "rmsnorm_bwd_pooled: unsupported combination");
  auto launch = [&](auto b) -> int {
    return launch_bwd_packed<decltype(b)::value, false>("rmsnorm_bwd_pooled", nr, nbp, dy, x, scale, rinv, dx, (float*)workspace, rows, d, eps,
                                                        drop_p, seed, dres, gelu_pre, group_rows, NormChain{}, dtype, stream);
  };
  const int rc = bc == 1 ? launch(Int<1>{}) : bc == 2 ? launch(Int<2>{}) : bc == 3 ? launch(Int<3>{}) : launch(Int<5>{});
  return rc ? rc : norm_colsums((const float*)workspace, nbp, d, dscale, nullptr, 0, stream);
}

// ---- RMSNorm folded into the consumer Linear (meant_linear_fwd_rowscale): statistics pass and chained backward ----
extern "C" int meant_rmsnorm_stats(const void* x, float* rinv, int64_t rows, int64_t d, float eps, int dtype, void* stream) {
  MEANT_REQUIRE(x && rinv, MEANT_ERR_ARG, "rmsnorm_stats: null pointer");
  const NormRoute nr = norm_route(rows, d);
  MEANT_REQUIRE(nr.kind == NORM_PACKED, MEANT_ERR_UNSUPPORTED,
                "rmsnorm_stats: rows=%lld d=%lld is not a packed shape (see meant_rmsnorm_pooled_ok)", (long long)rows, (long long)d);
  MEANT_REQUIRE(norm_aligned(nr, x, dtype_bytes(dtype)), MEANT_ERR_ARG, "rmsnorm_stats: 16-byte alignment");
  return launch_stats_packed("rmsnorm_stats", nr, x, rinv, rows, d, eps, dtype, stream);
}

extern "C" int meant_rmsnorm_bwd_chain(const void* dy, int dy_pooled, const void* x, const float* scale, const float* rinv, void* dx_scaled,
                                       float* dscale, int64_t rows, int64_t d, int64_t group_rows, float eps, float drop_p, uint64_t seed,
                                       const void* gelu_pre, const float* up_rinv, const float* up_bias, float up_eps, int64_t up_d,
                                       float* kcoef, float* dbias_up, int dtype, void* workspace, size_t workspace_bytes, void* stream) {
  const char* name = "rmsnorm_bwd_chain";
  MEANT_REQUIRE(dy && gelu_pre && scale && rinv && dx_scaled && dscale && up_rinv && up_bias && kcoef && dbias_up && workspace, MEANT_ERR_ARG,
                "rmsnorm_bwd_chain: null pointer");
  MEANT_REQUIRE((x != nullptr) != (dy_pooled != 0), MEANT_ERR_UNSUPPORTED,
                "rmsnorm_bwd_chain: either token-level dy with the stored activation x, or pooled dy with x formed from gelu_pre");
  const NormRoute nr = norm_route(rows, d);
  MEANT_REQUIRE(nr.kind == NORM_PACKED && rows < 2147483647LL && (!dy_pooled || meant_rmsnorm_pooled_ok(rows, d, group_rows)),
                MEANT_ERR_UNSUPPORTED, "rmsnorm_bwd_chain: rows=%lld d=%lld is not a packed shape (see meant_rmsnorm_pooled_ok)", (long long)rows,
                (long long)d);
  MEANT_REQUIRE(workspace_bytes >= meant_rmsnorm_bwd_ws(rows, d), MEANT_ERR_WORKSPACE, "rmsnorm_bwd_chain: workspace too small");
  const int nbp = packed_blocks_bwd(rows / nr.R);
  float* part1 = (float*)workspace;
  MEANT_REQUIRE(up_d > 0 && up_d < (1LL << 30), MEANT_ERR_ARG, "rmsnorm_bwd_chain: bad up_d");
  const NormChain ch{up_rinv, up_bias, kcoef, part1 + (size_t)nbp * d, up_eps, (int)up_d};
  const int rc = dy_pooled ? launch_bwd_packed<5, true>(name, nr, nbp, dy, x, scale, rinv, dx_scaled, part1, rows, d, eps, drop_p, seed, nullptr,
                                                        gelu_pre, group_rows, ch, dtype, stream)
                           : launch_bwd_packed<0, true>(name, nr, nbp, dy, x, scale, rinv, dx_scaled, part1, rows, d, eps, drop_p, seed, nullptr,
                                                        gelu_pre, 1, ch, dtype, stream);
  return rc ? rc : norm_colsums(part1, nbp, d, dscale, dbias_up, 1, stream);      // dbias_up +=: a gradient sink may be handed in
}

extern "C" int meant_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats,
                                   int64_t rows, int64_t d, float eps, int dtype, void* stream) {
  MEANT_REQUIRE(x && gamma && beta && y && stats, MEANT_ERR_ARG, "layernorm_fwd: null pointer");
  MEANT_REQUIRE(rows > 0 && d > 0 && d <= NORM_MAX_D, MEANT_ERR_UNSUPPORTED, "layernorm_fwd: unsupported d=%lld", (long long)d);
  const NormRoute nr = norm_route(rows, d, false);
  const size_t eb = dtype_bytes(dtype);
  // One wave per row is not checked, as it never was: x and y were always read in 16-byte loads there; gamma and beta (and gamma in
  // the backward) were read element by element and are now read in 16-byte loads like the gain, which the global loads of gfx950
  // perform at any float address: a parameter pointer off a 16-byte boundary is served on this route, more slowly.
  MEANT_REQUIRE(nr.kind != NORM_WIDE || (norm_aligned(nr, x, eb) && norm_aligned(nr, y, eb) && norm_aligned(nr, gamma, 4) && norm_aligned(nr, beta, 4)),
                MEANT_ERR_ARG, "layernorm_fwd: alignment");
  return launch_ln_fwd("layernorm_fwd", nr, x, gamma, beta, y, stats, rows, d, eps, dtype, stream);
}

extern "C" int meant_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* stats, void* dx,
                                   float* dgamma, float* dbeta, int64_t rows, int64_t d, int dtype, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  MEANT_REQUIRE(dy && x && gamma && stats && dx && dgamma && dbeta && workspace, MEANT_ERR_ARG, "layernorm_bwd: null pointer");
  MEANT_REQUIRE(rows > 0 && d > 0 && d <= NORM_MAX_D, MEANT_ERR_UNSUPPORTED, "layernorm_bwd: unsupported d=%lld", (long long)d);
  MEANT_REQUIRE(workspace_bytes >= meant_rmsnorm_bwd_ws(rows, d), MEANT_ERR_WORKSPACE, "layernorm_bwd: workspace too small");
  const NormRoute nr = norm_route(rows, d, false);
  const size_t eb = dtype_bytes(dtype);
  MEANT_REQUIRE(nr.kind != NORM_WIDE || (norm_aligned(nr, dy, eb) && norm_aligned(nr, x, eb) && norm_aligned(nr, dx, eb) && norm_aligned(nr, gamma, 4)),
                MEANT_ERR_ARG, "layernorm_bwd: alignment");
  const int nb = norm_blocks(rows);
  const int rc = launch_ln_bwd("layernorm_bwd", nr, nb, dy, x, gamma, stats, dx, (float*)workspace, rows, d, dtype, stream);
  return rc ? rc : norm_colsums((const float*)workspace, nb, d, dgamma, dbeta, 0, stream);
}
