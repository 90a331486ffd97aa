// K9 temporal (lag-axis) attention core: meant_temporal_attn_fwd / _bwd.  One-wave kernels for 1 <= L <= 64 (at the end of the
// kernel section), and the long-lag kernels described here for L > 64 (or any L under the option `temporal_long`).
//   q [B, D] (last lag step), kv [B*L, 2D] (K | V), p [B, H, L] fp32: raw scores while a kernel runs, softmax weights after it.
//
// Row-sweep kernels (Dh % 8 == 0, Dh <= 512, 16-byte aligned operands): one workgroup of four waves per (b, h).  A lane owns
// one 8-element chunk of the head slice, lpr = the power of two >= Dh / 8 lanes cover a row, so one load instruction of a wave
// fetches 64 / lpr key rows (four at Dh = 128); the waves take interleaved row groups.  Every lane group carries its own online
// softmax state (running maximum, sum, partial o) over the rows it saw; the states are merged once, across the groups of a
// wave by shuffles and across the waves through LDS.  LDS does not depend on L except for the backward's dp_l cache, which is
// used up to L = TL_DP_LDS and replaced by a second read of V beyond.
//
// Scalar kernels (any other Dh or alignment): one wave per (b, h), one element per lane, 64 rows per chunk -- the structure of
// the short-lag kernels with the chunk's scores in registers instead of one [64] LDS row.
//
// No atomics: every p, o, dq and dkv element has one writer and every reduction a fixed order.
#include "internal.h"

namespace {

constexpr int TL_WAVES = 4;
constexpr int TL_DP_LDS = 2048;      // backward: floats of dp_l kept in LDS per (b, h) (8 KiB)
constexpr int TL_EBLK = 8;           // scalar backward: dq accumulators per lane (64 * TL_EBLK elements of the head per sweep)

template <typename T>
__device__ __forceinline__ void tl_load8(const T* p, bool ok, float (&v)[8]) {
  if (ok) {
    const Vec8<T> x = load8<T>(p);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = x.get(k);
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = 0.f;
  }
}
template <typename T>
__device__ __forceinline__ void tl_store8(T* p, const float (&v)[8], float f) {
  Vec8<T> x;
#pragma unroll
  for (int k = 0; k < 8; ++k) x.set(k, v[k] * f);
  store8<T>(p, x);
}
__device__ __forceinline__ float tl_dot8(const float (&a)[8], const float (&b)[8]) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += a[k] * b[k];
  return s;
}
// sum over the lpr lanes that share a row (lpr a power of two, wave-uniform)
__device__ __forceinline__ float tl_row_sum(float s, int lpr) {
  for (int off = lpr >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}
// weight of a partial softmax state with maximum m under the merged maximum M; a state that saw no row has m = -inf
__device__ __forceinline__ float tl_weight(float m, float M) { return m == -INFINITY ? 0.f : expf(m - M); }

// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void temporal_long_fwd_kernel(const T* __restrict__ q, const T* __restrict__ kv, T* __restrict__ o,
                                                                 float* p, int L, int H, int Dh, int lpr_log2, float scale) {
  __shared__ float red_a[TL_WAVES][64][8];
  __shared__ float red_ms[TL_WAVES][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t bh = blockIdx.x, b = bh / H;
  const int h = (int)(bh - b * H);
  const int D = H * Dh;
  const int lpr = 1 << lpr_log2, c = lane & (lpr - 1), r = lane >> lpr_log2, rpw = 64 >> lpr_log2;
  const bool live = c * 8 < Dh;                                        // Dh / 8 need not be a power of two
  float qv[8];
  tl_load8(q + b * D + h * Dh + c * 8, live, qv);
  float* pp = p + bh * L;
  const T* kvb = kv + b * L * (int64_t)(2 * D) + h * Dh + c * 8;
  float m = -INFINITY, sum = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int64_t l0 = (int64_t)wave * rpw; l0 < L; l0 += TL_WAVES * rpw) {          // wave-uniform trip count
    const int64_t l = l0 + r;
    const bool ok = l < L;
    float kk[8], vv[8];
    tl_load8(kvb + l * (2 * D), ok && live, kk);
    tl_load8(kvb + l * (2 * D) + D, ok && live, vv);
    const float s = tl_row_sum(tl_dot8(qv, kk), lpr) * scale;
    if (ok) {
      if (c == 0) pp[l] = s;
      const float mn = fmaxf(m, s);
      const float corr = mn == m ? 1.f : expf(m - mn);                 // rescale only when the maximum moved
      const float e = expf(s - mn);
      sum = sum * corr + e;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = acc[k] * corr + e * vv[k];
      m = mn;
    }
  }
  for (int off = lpr; off < 64; off <<= 1) {                           // the row groups of this wave
    const float m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(sum, off, 64);
    const float M = fmaxf(m, m2), w1 = tl_weight(m, M), w2 = tl_weight(m2, M);
    sum = sum * w1 + s2 * w2;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = acc[k] * w1 + __shfl_xor(acc[k], off, 64) * w2;
    m = M;
  }
  if (r == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red_a[wave][c][k] = acc[k];
  }
  if (lane == 0) { red_ms[wave][0] = m; red_ms[wave][1] = sum; }
  __syncthreads();                                                     // also orders the raw scores in p for the sweep below
  float M = red_ms[0][0];
#pragma unroll
  for (int w = 1; w < TL_WAVES; ++w) M = fmaxf(M, red_ms[w][0]);
  float wgt[TL_WAVES], S = 0.f;
#pragma unroll
  for (int w = 0; w < TL_WAVES; ++w) { wgt[w] = tl_weight(red_ms[w][0], M); S += red_ms[w][1] * wgt[w]; }
  const float inv = 1.f / S;
  if (wave == 0 && r == 0 && live) {
    float ov[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float a = 0.f;
#pragma unroll
      for (int w = 0; w < TL_WAVES; ++w) a += red_a[w][c][k] * wgt[w];
      ov[k] = a;
    }
    tl_store8(o + b * D + h * Dh + c * 8, ov, inv);
  }
  for (int64_t l = threadIdx.x; l < L; l += 256) pp[l] = expf(pp[l] - M) * inv;
}

template <typename T>
__global__ __launch_bounds__(256) void temporal_long_bwd_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                                 const float* __restrict__ p, const T* __restrict__ dout,
                                                                 T* __restrict__ dq, T* __restrict__ dkv, int L, int H, int Dh,
                                                                 int lpr_log2, float scale, int dp_cached) {
  __shared__ float red_a[TL_WAVES][64][8];
  __shared__ float red_dot[TL_WAVES];
  __shared__ float dps[TL_DP_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t bh = blockIdx.x, b = bh / H;
  const int h = (int)(bh - b * H);
  const int D = H * Dh;
  const int lpr = 1 << lpr_log2, c = lane & (lpr - 1), r = lane >> lpr_log2, rpw = 64 >> lpr_log2;
  const bool live = c * 8 < Dh;
  float qv[8], dov[8];
  tl_load8(q + b * D + h * Dh + c * 8, live, qv);
  tl_load8(dout + b * D + h * Dh + c * 8, live, dov);
  const float* pp = p + bh * L;
  const int64_t base = b * L * (int64_t)(2 * D) + h * Dh + c * 8;
  // pass 1 over V: dp_l = do . v_l and the row term sum_l p_l dp_l
  float part = 0.f;
  for (int64_t l0 = (int64_t)wave * rpw; l0 < L; l0 += TL_WAVES * rpw) {
    const int64_t l = l0 + r;
    const bool ok = l < L;
    float vv[8];
    tl_load8(kv + base + l * (2 * D) + D, ok && live, vv);
    const float dp = tl_row_sum(tl_dot8(dov, vv), lpr);
    if (ok && c == 0) {
      part += pp[l] * dp;
      if (dp_cached) dps[l] = dp;
    }
  }
  part = wave_sum(part);
  if (lane == 0) red_dot[wave] = part;
  __syncthreads();
  const float dot = (red_dot[0] + red_dot[1]) + (red_dot[2] + red_dot[3]);
  // pass 2 over K: ds_l, dq, and the dk / dv rows
  float dqa[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int64_t l0 = (int64_t)wave * rpw; l0 < L; l0 += TL_WAVES * rpw) {
    const int64_t l = l0 + r;
    const bool ok = l < L;
    float kk[8];
    tl_load8(kv + base + l * (2 * D), ok && live, kk);
    float dp;
    if (dp_cached) {
      dp = ok ? dps[l] : 0.f;
    } else {                                                           // wave-uniform: L > TL_DP_LDS reads V a second time
      float vv[8];
      tl_load8(kv + base + l * (2 * D) + D, ok && live, vv);
      dp = tl_row_sum(tl_dot8(dov, vv), lpr);
    }
    const float pl = ok ? pp[l] : 0.f;
    const float ds = pl * (dp - dot) * scale;
    if (ok && live) {
#pragma unroll
      for (int k = 0; k < 8; ++k) dqa[k] += ds * kk[k];
      tl_store8(dkv + base + l * (2 * D), qv, ds);
      tl_store8(dkv + base + l * (2 * D) + D, dov, pl);
    }
  }
  for (int off = lpr; off < 64; off <<= 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) dqa[k] += __shfl_xor(dqa[k], off, 64);
  }
  if (r == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red_a[wave][c][k] = dqa[k];
  }
  __syncthreads();
  if (wave == 0 && r == 0 && live) {
    float g[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = (red_a[0][c][k] + red_a[1][c][k]) + (red_a[2][c][k] + red_a[3][c][k]);
    tl_store8(dq + b * D + h * Dh + c * 8, g, 1.f);
  }
}

// ------------------------------------------------------------------------------------------------
// any Dh, any alignment: one wave per (b, h)
template <typename T>
__global__ __launch_bounds__(256) void temporal_long_fwd_scalar_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                                        T* __restrict__ o, float* p, int64_t BH, int L, int H,
                                                                        int Dh, float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t bh = (int64_t)blockIdx.x * 4 + wave;
  if (bh >= BH) return;
  const int64_t b = bh / H;
  const int h = (int)(bh - b * H);
  const int D = H * Dh;
  const T* qp = q + b * D + h * Dh;
  const T* kvb = kv + b * L * (int64_t)(2 * D) + h * Dh;
  float* pp = p + bh * L;
  float m = -INFINITY, sum = 0.f;
  for (int64_t l0 = 0; l0 < L; l0 += 64) {
    const int cnt = (int)(L - l0 < 64 ? L - l0 : 64);
    float mine = 0.f;
    for (int j = 0; j < cnt; ++j) {
      const T* kp = kvb + (l0 + j) * (2 * D);
      float s = 0.f;
      for (int e = lane; e < Dh; e += 64) s += to_f(qp[e]) * to_f(kp[e]);
      s = wave_sum(s) * scale;                                         // the same bits in every lane
      if (lane == j) mine = s;
      const float mn = fmaxf(m, s);
      sum = sum * (mn == m ? 1.f : expf(m - mn)) + expf(s - mn);
      m = mn;
    }
    if (lane < cnt) pp[l0 + lane] = mine;                              // each lane reads back only what it wrote itself
  }
  const float inv = 1.f / sum;
  for (int64_t l0 = 0; l0 < L; l0 += 64)
    if (l0 + lane < L) pp[l0 + lane] = expf(pp[l0 + lane] - m) * inv;
  for (int e0 = 0; e0 < Dh; e0 += 64) {
    const int e = e0 + lane;
    const bool ok = e < Dh;
    float acc = 0.f;
    for (int64_t l0 = 0; l0 < L; l0 += 64) {
      const int cnt = (int)(L - l0 < 64 ? L - l0 : 64);
      const float w = lane < cnt ? pp[l0 + lane] : 0.f;
      for (int j = 0; j < cnt; ++j) {
        const float wj = __shfl(w, j, 64);
        if (ok) acc += wj * to_f(kvb[(l0 + j) * (2 * D) + D + e]);
      }
    }
    if (ok) o[b * D + h * Dh + e] = from_f<T>(acc);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void temporal_long_bwd_scalar_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                                        const float* __restrict__ p, const T* __restrict__ dout,
                                                                        T* __restrict__ dq, T* __restrict__ dkv, int64_t BH, int L,
                                                                        int H, int Dh, float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t bh = (int64_t)blockIdx.x * 4 + wave;
  if (bh >= BH) return;
  const int64_t b = bh / H;
  const int h = (int)(bh - b * H);
  const int D = H * Dh;
  const T* qp = q + b * D + h * Dh;
  const T* dop = dout + b * D + h * Dh;
  const int64_t base = b * L * (int64_t)(2 * D) + h * Dh;
  const float* pp = p + bh * L;
  float dot = 0.f;                                                     // sum_l p_l dp_l
  for (int64_t l = 0; l < L; ++l) {
    const T* vp = kv + base + l * (2 * D) + D;
    float s = 0.f;
    for (int e = lane; e < Dh; e += 64) s += to_f(dop[e]) * to_f(vp[e]);
    dot += pp[l] * wave_sum(s);
  }
  // 64 * TL_EBLK elements of the head per sweep over L (one sweep up to Dh = 512); a sweep recomputes dp_l from V
  for (int e0 = 0; e0 < Dh; e0 += 64 * TL_EBLK) {
    float qe[TL_EBLK], doe[TL_EBLK], dqa[TL_EBLK];
#pragma unroll
    for (int k = 0; k < TL_EBLK; ++k) {
      const int e = e0 + k * 64 + lane;
      qe[k] = e < Dh ? to_f(qp[e]) : 0.f;
      doe[k] = e < Dh ? to_f(dop[e]) : 0.f;
      dqa[k] = 0.f;
    }
    for (int64_t l0 = 0; l0 < L; l0 += 64) {
      const int cnt = (int)(L - l0 < 64 ? L - l0 : 64);
      float mine = 0.f;
      for (int j = 0; j < cnt; ++j) {
        const T* vp = kv + base + (l0 + j) * (2 * D) + D;
        float s = 0.f;
        for (int e = lane; e < Dh; e += 64) s += to_f(dop[e]) * to_f(vp[e]);
        s = wave_sum(s);
        if (lane == j) mine = s;
      }
      const float pw = lane < cnt ? pp[l0 + lane] : 0.f;
      const float ds = pw * (mine - dot) * scale;
      for (int j = 0; j < cnt; ++j) {
        const float dsj = __shfl(ds, j, 64), pj = __shfl(pw, j, 64);
        const int64_t row = base + (l0 + j) * (2 * D);
#pragma unroll
        for (int k = 0; k < TL_EBLK; ++k) {
          const int e = e0 + k * 64 + lane;
          if (e < Dh) {
            dqa[k] += dsj * to_f(kv[row + e]);
            dkv[row + e] = from_f<T>(dsj * qe[k]);
            dkv[row + D + e] = from_f<T>(pj * doe[k]);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < TL_EBLK; ++k) {
      const int e = e0 + k * 64 + lane;
      if (e < Dh) dq[b * D + h * Dh + e] = from_f<T>(dqa[k]);
    }
  }
}

// lanes per row of the row-sweep kernels as a power of two, or -1 when the shape takes the scalar kernels
int tl_lpr_log2(int Dh, const void* a, const void* b, const void* c, const void* d, const void* e) {
  if (Dh % 8 != 0 || Dh > 512) return -1;
  if (!(meant_aligned16(a) && meant_aligned16(b) && meant_aligned16(c) && meant_aligned16(d) && meant_aligned16(e))) return -1;
  int lg = 0;
  while ((8 << lg) < Dh) ++lg;
  return lg;
}

// ------------------------------------------------------------------------------------------------
// short lags: one wave per (b, h); L <= 64 keys, any Dh
template <typename T>
__global__ __launch_bounds__(256) void temporal_fwd_kernel(const T* __restrict__ q, const T* __restrict__ kv, T* __restrict__ o,
                                                            float* __restrict__ p, int64_t B, int L, int H, int Dh, float scale) {
  __shared__ float sc[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t bh = (int64_t)blockIdx.x * 4 + wave;
  if (bh >= B * H) return;
  const int64_t b = bh / H;
  const int h = (int)(bh - b * H);
  const int D = H * Dh;
  const T* qp = q + b * D + h * Dh;
  for (int l = 0; l < L; ++l) {
    const T* kp = kv + (b * L + l) * (int64_t)(2 * D) + h * Dh;
    float s = 0.f;
    for (int e = lane; e < Dh; e += 64) s += to_f(qp[e]) * to_f(kp[e]);
    s = wave_sum(s) * scale;
    if (lane == 0) sc[wave][l] = s;
  }
  __builtin_amdgcn_wave_barrier();
  float m = -INFINITY;
  for (int l = 0; l < L; ++l) m = fmaxf(m, sc[wave][l]);
  float sum = 0.f;
  for (int l = 0; l < L; ++l) sum += __expf(sc[wave][l] - m);
  const float inv = 1.f / sum;
  __builtin_amdgcn_wave_barrier();
  if (lane < L) {
    const float w = __expf(sc[wave][lane] - m) * inv;
    p[bh * L + lane] = w;
    sc[wave][lane] = w;
  }
  __builtin_amdgcn_wave_barrier();
  for (int e = lane; e < Dh; e += 64) {
    float acc = 0.f;
    for (int l = 0; l < L; ++l) acc += sc[wave][l] * to_f(kv[(b * L + l) * (int64_t)(2 * D) + D + h * Dh + e]);
    o[b * D + h * Dh + e] = from_f<T>(acc);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void temporal_bwd_kernel(const T* __restrict__ q, const T* __restrict__ kv,
                                                            const float* __restrict__ p, const T* __restrict__ dout,
                                                            T* __restrict__ dq, T* __restrict__ dkv, int64_t B, int L, int H,
                                                            int Dh, float scale) {
  __shared__ float ds[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t bh = (int64_t)blockIdx.x * 4 + wave;
  if (bh >= B * H) return;
  const int64_t b = bh / H;
  const int h = (int)(bh - b * H);
  const int D = H * Dh;
  const T* dop = dout + b * D + h * Dh;
  float dot = 0.f;                                   // sum_l p_l dp_l
  for (int l = 0; l < L; ++l) {
    const T* vp = kv + (b * L + l) * (int64_t)(2 * D) + D + h * Dh;
    float s = 0.f;
    for (int e = lane; e < Dh; e += 64) s += to_f(dop[e]) * to_f(vp[e]);
    s = wave_sum(s);                                 // dp_l
    if (lane == 0) ds[wave][l] = s;
    dot += p[bh * L + l] * s;
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < L) ds[wave][lane] = p[bh * L + lane] * (ds[wave][lane] - dot) * scale;
  __builtin_amdgcn_wave_barrier();
  for (int e = lane; e < Dh; e += 64) {
    const float qe = to_f(q[b * D + h * Dh + e]);
    const float doe = to_f(dop[e]);
    float dqe = 0.f;
    for (int l = 0; l < L; ++l) {
      const int64_t row = (b * L + l) * (int64_t)(2 * D);
      dqe += ds[wave][l] * to_f(kv[row + h * Dh + e]);
      dkv[row + h * Dh + e] = from_f<T>(ds[wave][l] * qe);
      dkv[row + D + h * Dh + e] = from_f<T>(p[bh * L + l] * doe);
    }
    dq[b * D + h * Dh + e] = from_f<T>(dqe);
  }
}

}  // namespace

static int temporal_long_fwd(const void* q, const void* kv, void* o, float* p, int64_t B, int L, int H, int Dh, float scale, int dtype,
                             hipStream_t stream) {
  const int64_t BH = B * H;
  MEANT_REQUIRE(BH <= 2147483647LL, MEANT_ERR_UNSUPPORTED, "temporal_attn_fwd: B * H = %lld exceeds the grid limit", (long long)BH);
  const int lg = tl_lpr_log2(Dh, q, kv, o, nullptr, nullptr);
  if (lg >= 0) {
    DISPATCH_DTYPE(dtype, T,
                   hipLaunchKernelGGL(temporal_long_fwd_kernel<T>, dim3((unsigned)BH), dim3(256), 0, stream, (const T*)q, (const T*)kv,
                                      (T*)o, p, L, H, Dh, lg, scale));
  } else {
    DISPATCH_DTYPE(dtype, T,
                   hipLaunchKernelGGL(temporal_long_fwd_scalar_kernel<T>, dim3((unsigned)ceil_div(BH, 4)), dim3(256), 0, stream,
                                      (const T*)q, (const T*)kv, (T*)o, p, BH, L, H, Dh, scale));
  }
  MEANT_LAUNCH_CHECK("temporal_attn_fwd (long lag)");
  meant_route_hit(ROUTE_TEMPORAL_LONG);
  return MEANT_OK;
}

static int temporal_long_bwd(const void* q, const void* kv, const float* p, const void* do_, void* dq, void* dkv, int64_t B, int L, int H,
                             int Dh, float scale, int dtype, hipStream_t stream) {
  const int64_t BH = B * H;
  MEANT_REQUIRE(BH <= 2147483647LL, MEANT_ERR_UNSUPPORTED, "temporal_attn_bwd: B * H = %lld exceeds the grid limit", (long long)BH);
  const int lg = tl_lpr_log2(Dh, q, kv, do_, dq, dkv);
  if (lg >= 0) {
    DISPATCH_DTYPE(dtype, T,
                   hipLaunchKernelGGL(temporal_long_bwd_kernel<T>, dim3((unsigned)BH), dim3(256), 0, stream, (const T*)q, (const T*)kv, p,
                                      (const T*)do_, (T*)dq, (T*)dkv, L, H, Dh, lg, scale, L <= TL_DP_LDS ? 1 : 0));
  } else {
    DISPATCH_DTYPE(dtype, T,
                   hipLaunchKernelGGL(temporal_long_bwd_scalar_kernel<T>, dim3((unsigned)ceil_div(BH, 4)), dim3(256), 0, stream,
                                      (const T*)q, (const T*)kv, p, (const T*)do_, (T*)dq, (T*)dkv, BH, L, H, Dh, scale));
  }
  MEANT_LAUNCH_CHECK("temporal_attn_bwd (long lag)");
  meant_route_hit(ROUTE_TEMPORAL_LONG);
  return MEANT_OK;
}

extern "C" int meant_temporal_attn_fwd(const void* q, const void* kv, void* o, float* p, int64_t B, int L, int H, int Dh, float scale, int dtype, void* stream) {
  MEANT_REQUIRE(q && kv && o && p && B > 0 && H > 0 && Dh > 0, MEANT_ERR_ARG, "temporal_attn_fwd: bad argument");
  MEANT_REQUIRE(L > 0, MEANT_ERR_UNSUPPORTED, "temporal_attn_fwd: lag %d is not positive", L);
  if (L > 64 || meant_opt(MEANT_OPT_TEMPORAL_LONG)) return temporal_long_fwd(q, kv, o, p, B, L, H, Dh, scale, dtype, (hipStream_t)stream);
  DISPATCH_DTYPE(dtype, T,
                 hipLaunchKernelGGL(temporal_fwd_kernel<T>, dim3((unsigned)ceil_div(B * H, 4)), dim3(256), 0, (hipStream_t)stream,
                                    (const T*)q, (const T*)kv, (T*)o, p, B, L, H, Dh, scale));
  MEANT_LAUNCH_CHECK("temporal_attn_fwd");
  return MEANT_OK;
}
extern "C" int meant_temporal_attn_bwd(const void* q, const void* kv, const float* p, const void* do_, void* dq, void* dkv, int64_t B, int L, int H, int Dh, float scale, int dtype, void* stream) {
  MEANT_REQUIRE(q && kv && p && do_ && dq && dkv && B > 0 && H > 0 && Dh > 0, MEANT_ERR_ARG, "temporal_attn_bwd: bad argument");
  MEANT_REQUIRE(L > 0, MEANT_ERR_UNSUPPORTED, "temporal_attn_bwd: lag %d is not positive", L);
  if (L > 64 || meant_opt(MEANT_OPT_TEMPORAL_LONG)) return temporal_long_bwd(q, kv, p, do_, dq, dkv, B, L, H, Dh, scale, dtype, (hipStream_t)stream);
  DISPATCH_DTYPE(dtype, T,
                 hipLaunchKernelGGL(temporal_bwd_kernel<T>, dim3((unsigned)ceil_div(B * H, 4)), dim3(256), 0, (hipStream_t)stream,
                                    (const T*)q, (const T*)kv, p, (const T*)do_, (T*)dq, (T*)dkv, B, L, H, Dh, scale));
  MEANT_LAUNCH_CHECK("temporal_attn_bwd");
  return MEANT_OK;
}
