// Classification counts on the device (utils/f1_metrics.py, called per batch at in_loop_train.py:208-241, 281-319, 339-359 after an
// out.detach().cpu()): the prediction of a row is argmax over its C class columns as torch computes it, and everything the seven
// metrics of the reference need is three integer histograms and four row counters.
//   * meant_metrics_update        -- from scores [B, ld] (f32 | bf16)
//   * meant_metrics_update_labels -- from ready-made predictions
// state = int64 [3C + 4]: tp[C], npred[C], ntarget[C], n_rows, n_ignored, n_invalid, n_nan; confusion (optional) int64 [C, C], row = target.
// The calls only add, every counter is an integer: any number of updates in any workgroup arrival order gives the same bits.
// Three kernels, all with a capped grid and a stride loop over the rows:
//   rows   (C <= 16, the class head [128, 2]): a lane per row; per-class counts by wave ballots into LDS, one global atomic per
//          non-zero counter and workgroup.
//   wave   (C > 16, meant_vqa's answers, the MLM vocabulary): a wave per row; 16-byte loads where the rows allow them, a running
//          (value, index) per lane, a butterfly over the pairs, lane 0's atomics on the class counters; the four row counters stay
//          in registers and leave through LDS once per workgroup.
//   labels (C > 16, predictions given): a lane per row, the class counters by global atomics, the row counters as above.
// A row whose target is the ignore index or outside [0, C) is never read and forms no address.
//   * meant_score_capture         -- the scores themselves, kept for the rank statistic of auroc.hip: a lane per row writes the
//                                    order-preserving 32-bit image of each captured column and the row's label to the caller's
//                                    buffers at a slot the host names; the same four row counters, through LDS as above.
//   * meant_vqa_score_update      -- the VQA score of soft targets [B, C] (vqa.py:223; utils/custom_datasets.py:214-218): the wave form's
//                                    argmax, then the target's weight at the predicted column, summed in 2^-32 units as an integer.
#include "common.h"
#include <limits.h>

namespace {

constexpr int MT_THREADS = 256;                        // rows and labels kernels: a lane per row
constexpr int MT_WAVE_THREADS = 1024;                  // wave kernel: 16 rows in flight per workgroup
constexpr int MT_WAVES = MT_WAVE_THREADS / 64;
constexpr int MT_ROWS_MAXC = 16;                       // the cut between the rows and the wave form
// Grid caps.  Atomics on ONE address retire one after the other (measured: ~12.5 ns each, a call whose 2048 workgroups add one row
// counter each takes 27 us for that alone), and every workgroup ends with up to four of them on the row counters, so the grids
// are as small as the work allows: a workgroup per CU of lanes-per-row, two of 16 waves per CU (a full CU) of waves-per-row.
constexpr int MT_ROWS_MAXGRID = 256;
constexpr int MT_WAVE_WGS_PER_CU = 2;
static_assert(MT_THREADS == MT_ROWS_MAXC * MT_ROWS_MAXC && 3 * MT_ROWS_MAXC + 4 <= MT_THREADS, "the rows kernel zeroes and flushes its LDS one entry per thread");
typedef unsigned long long u64;

enum { TAIL_ROWS = 0, TAIL_IGNORED, TAIL_INVALID, TAIL_NAN };

// torch.argmax's order on one pair: is x (at a HIGHER index than the holder of v) the new maximum?  NaN ranks above everything,
// the first one stays
__device__ __forceinline__ bool mt_takes(float x, float v) { return x > v || (x != x && v == v); }

// the same order between two lanes' (value, index) pairs: greater value, then lower index
__device__ __forceinline__ bool mt_better(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return an && (!bn || ai < bi);
  return av > bv || (av == bv && ai < bi);
}

__device__ __forceinline__ void mt_add(int64_t* p, unsigned n) { atomicAdd(reinterpret_cast<u64*>(p), (u64)n); }

// what a lane knows about its row after the target checks: counted (valid) with a prediction, or one of the two skipped kinds
struct RowVerdict { bool valid, ignored, invalid, nan; int pred, tgt; };

// ---- rows form and its label twin: C <= MT_ROWS_MAXC ---------------------------------------------------------------------
template <typename T, bool LABELS>
__global__ __launch_bounds__(MT_THREADS) void metrics_rows_kernel(const T* __restrict__ scores, int64_t ld, const int64_t* __restrict__ pred_in,
                                                                   const int64_t* __restrict__ target, int64_t B, int C, int64_t ignore_index,
                                                                   int64_t* __restrict__ state, int64_t* __restrict__ confusion) {
  __shared__ unsigned cnt[3 * MT_ROWS_MAXC + 4];
  __shared__ unsigned conf[MT_ROWS_MAXC * MT_ROWS_MAXC];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 3 * MT_ROWS_MAXC + 4) cnt[tid] = 0;
  conf[tid] = 0;                                       // MT_THREADS == MT_ROWS_MAXC^2
  __syncthreads();
  unsigned my_tp = 0, my_np = 0, my_nt = 0;            // lane c < C: class c's counts over this wave's rows
  unsigned t_rows = 0, t_ign = 0, t_inv = 0, t_nan = 0;
  const int64_t step = (int64_t)gridDim.x * MT_THREADS;
  for (int64_t r0 = (int64_t)blockIdx.x * MT_THREADS + (tid - lane); r0 < B; r0 += step) {     // wave-uniform: ballots below
    const int64_t r = r0 + lane;
    RowVerdict v = {false, false, false, false, 0, 0};
    if (r < B) {
      const int64_t t = target[r];
      if (t == ignore_index) v.ignored = true;
      else if (t < 0 || t >= C) v.invalid = true;
      else if (LABELS) {
        const int64_t p = pred_in[r];
        if (p < 0 || p >= C) v.invalid = true;
        else { v.valid = true; v.pred = (int)p; v.tgt = (int)t; }
      } else {
        const T* row = scores + r * ld;
        float best = to_f(row[0]);
        int bi = 0;
        for (int j = 1; j < C; ++j) {
          const float x = to_f(row[j]);
          if (mt_takes(x, best)) { best = x; bi = j; }
        }
        v.valid = true; v.pred = bi; v.tgt = (int)t; v.nan = best != best;
      }
    }
    t_rows += (unsigned)__popcll(__ballot(v.valid));
    t_ign += (unsigned)__popcll(__ballot(v.ignored));
    t_inv += (unsigned)__popcll(__ballot(v.invalid));
    t_nan += (unsigned)__popcll(__ballot(v.nan));
    for (int c = 0; c < C; ++c) {
      const unsigned long long bp = __ballot(v.valid && v.pred == c), bt = __ballot(v.valid && v.tgt == c);
      const unsigned long long btp = __ballot(v.valid && v.pred == c && v.tgt == c);
      if (lane == c) { my_np += (unsigned)__popcll(bp); my_nt += (unsigned)__popcll(bt); my_tp += (unsigned)__popcll(btp); }
    }
    if (confusion && v.valid) atomicAdd(&conf[v.tgt * C + v.pred], 1u);
  }
  if (lane < C) {
    if (my_tp) atomicAdd(&cnt[lane], my_tp);
    if (my_np) atomicAdd(&cnt[C + lane], my_np);
    if (my_nt) atomicAdd(&cnt[2 * C + lane], my_nt);
  }
  if (lane == 0) {
    if (t_rows) atomicAdd(&cnt[3 * C + TAIL_ROWS], t_rows);
    if (t_ign) atomicAdd(&cnt[3 * C + TAIL_IGNORED], t_ign);
    if (t_inv) atomicAdd(&cnt[3 * C + TAIL_INVALID], t_inv);
    if (t_nan) atomicAdd(&cnt[3 * C + TAIL_NAN], t_nan);
  }
  __syncthreads();
  if (tid < 3 * C + 4 && cnt[tid]) mt_add(state + tid, cnt[tid]);
  if (confusion && tid < C * C && conf[tid]) mt_add(confusion + tid, conf[tid]);
}

// the four row counters of a workgroup's waves, through LDS, one global atomic each
__device__ __forceinline__ void mt_flush_tail(unsigned (&tail)[4], unsigned t_rows, unsigned t_ign, unsigned t_inv, unsigned t_nan,
                                              int64_t* state, int C) {
  const int tid = threadIdx.x;
  if (tid < 4) tail[tid] = 0;
  __syncthreads();
  if ((tid & 63) == 0) {
    if (t_rows) atomicAdd(&tail[TAIL_ROWS], t_rows);
    if (t_ign) atomicAdd(&tail[TAIL_IGNORED], t_ign);
    if (t_inv) atomicAdd(&tail[TAIL_INVALID], t_inv);
    if (t_nan) atomicAdd(&tail[TAIL_NAN], t_nan);
  }
  __syncthreads();
  if (tid < 4 && tail[tid]) mt_add(state + 3 * (int64_t)C + tid, tail[tid]);
}

// ---- wave form: any C, a wave per row ------------------------------------------------------------------------------------
template <typename T> struct MtChunk;                  // 16 bytes of a row
template <> struct MtChunk<float> {
  static constexpr int E = 4;
  f32x4 v;
  __device__ __forceinline__ float get(int e) const { return v[e]; }
};
template <> struct MtChunk<bf16> {
  static constexpr int E = 8;
  bf16x8 v;
  __device__ __forceinline__ float get(int e) const { return (float)v[e]; }
};
template <typename T> __device__ __forceinline__ MtChunk<T> mt_load(const T* p) {
  MtChunk<T> c;
  c.v = __builtin_nontemporal_load(reinterpret_cast<const decltype(c.v)*>(p));     // read once
  return c;
}

// a wave's argmax over the C columns of the row at p, in torch's order; every lane gets (v, vi): the value and 0 <= vi < C
template <typename T, bool VEC>
__device__ __forceinline__ void mt_wave_argmax(const T* __restrict__ p, int C, int lane, float& v, int& vi) {
  constexpr int E = MtChunk<T>::E;
  v = -INFINITY;
  vi = INT_MAX;                                        // INT_MAX: nothing taken yet (no candidate, or -inf only)
  int first;                                           // this lane's lowest candidate column
  if (VEC) {                                           // ld % E == 0: the chunk that holds column C - 1 lies inside the row
    first = lane * E;
    const int nfull = C / E, nchunks = (C + E - 1) / E;
    int c = lane;
    for (; c + 192 < nfull; c += 256) {                // four loads in flight per lane
      MtChunk<T> k[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) k[u] = mt_load(p + (int64_t)(c + 64 * u) * E);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const float x = k[u].get(e);
          if (mt_takes(x, v)) { v = x; vi = (c + 64 * u) * E + e; }
        }
    }
    for (; c < nchunks; c += 64) {
      const MtChunk<T> k = mt_load(p + (int64_t)c * E);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float x = k.get(e);
        const int j = c * E + e;
        if (j < C && mt_takes(x, v)) { v = x; vi = j; }
      }
    }
  } else {
    first = lane;
    for (int j = lane; j < C; j += 64) {
      const float x = to_f(p[j]);
      if (mt_takes(x, v)) { v = x; vi = j; }
    }
  }
  if (vi == INT_MAX && first < C) vi = first;          // all of this lane's candidates were -inf: the first of them
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(vi, o, 64);
    if (mt_better(ov, oi, v, vi)) { v = ov; vi = oi; }
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(MT_WAVE_THREADS) void metrics_wave_kernel(const T* __restrict__ scores, int64_t ld, const int64_t* __restrict__ target,
                                                                   int64_t B, int C, int64_t ignore_index, int64_t* __restrict__ state,
                                                                   int64_t* __restrict__ confusion) {
  __shared__ unsigned tail[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned t_rows = 0, t_ign = 0, t_inv = 0, t_nan = 0;                             // wave-uniform
  for (int64_t row = (int64_t)blockIdx.x * MT_WAVES + wave; row < B; row += (int64_t)gridDim.x * MT_WAVES) {
    const int64_t tl = target[row];                    // one address for the wave: make the value (and the branches on it) scalar
    const int64_t t = (int64_t)(((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)((u64)tl >> 32)) << 32) |
                                (unsigned)__builtin_amdgcn_readfirstlane((int)(u64)tl));
    if (t == ignore_index) { ++t_ign; continue; }
    if (t < 0 || t >= C) { ++t_inv; continue; }
    float v;
    int vi;
    mt_wave_argmax<T, VEC>(scores + row * ld, C, lane, v, vi);
    ++t_rows;
    if (v != v) ++t_nan;
    if (lane == 0 && vi >= 0 && vi < C) {              // vi < C always holds (lane 0 has column 0); never form an address beyond
      const int tc = (int)t;
      mt_add(state + C + vi, 1);
      mt_add(state + 2 * (int64_t)C + tc, 1);
      if (vi == tc) mt_add(state + vi, 1);
      if (confusion) mt_add(confusion + (int64_t)tc * C + vi, 1);
    }
  }
  mt_flush_tail(tail, t_rows, t_ign, t_inv, t_nan, state, C);
}

// ---- VQA score: the soft weight of the predicted answer ---------------------------------------------------------------------
// state = int64 [4]: sum_fx (the weights in 2^-32 units), rows, nan rows, invalid rows.  The wave form's walk and argmax; the weight
// is one element of the target row, read by every lane from the same address.
enum { VQ_SUM = 0, VQ_ROWS, VQ_NAN, VQ_INVALID };
constexpr float VQ_MAX_WEIGHT = 16.f;                  // a weight in [0, 16] is below 2^37 units: 2^26 rows of them fit an int64

template <typename T, bool VEC>
__global__ __launch_bounds__(MT_WAVE_THREADS) void vqa_score_kernel(const T* __restrict__ scores, int64_t lds, const void* __restrict__ target,
                                                                    int64_t ldt, bool target_bf16, int64_t B, int C, int64_t* __restrict__ state) {
  __shared__ u64 sum;
  __shared__ unsigned tail[3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u64 t_fx = 0;                                                                     // wave-uniform, like the three counters
  unsigned t_rows = 0, t_nan = 0, t_inv = 0;
  for (int64_t row = (int64_t)blockIdx.x * MT_WAVES + wave; row < B; row += (int64_t)gridDim.x * MT_WAVES) {
    float v;
    int vi;
    mt_wave_argmax<T, VEC>(scores + row * lds, C, lane, v, vi);
    if (vi < 0 || vi >= C) vi = 0;                     // never holds (see metrics_wave_kernel); never form an address beyond
    const int64_t at = row * ldt + vi;
    const float w = target_bf16 ? (float)static_cast<const bf16*>(target)[at] : static_cast<const float*>(target)[at];
    if (v != v) ++t_nan;
    if (w >= 0.f && w <= VQ_MAX_WEIGHT) {              // false for a NaN
      t_fx += (u64)llrint((double)w * 4294967296.0);
      ++t_rows;
    } else {
      ++t_inv;
    }
  }
  if (tid == 0) sum = 0;
  if (tid < 3) tail[tid] = 0;
  __syncthreads();
  if (lane == 0) {
    if (t_fx) atomicAdd(&sum, t_fx);
    if (t_rows) atomicAdd(&tail[VQ_ROWS - 1], t_rows);
    if (t_nan) atomicAdd(&tail[VQ_NAN - 1], t_nan);
    if (t_inv) atomicAdd(&tail[VQ_INVALID - 1], t_inv);
  }
  __syncthreads();
  if (tid == 0 && sum) atomicAdd(reinterpret_cast<u64*>(state + VQ_SUM), sum);
  if (tid >= 1 && tid < 4 && tail[tid - 1]) mt_add(state + tid, tail[tid - 1]);
}

// ---- labels, C > MT_ROWS_MAXC --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_THREADS) void metrics_labels_kernel(const int64_t* __restrict__ pred, const int64_t* __restrict__ target, int64_t B,
                                                                     int C, int64_t ignore_index, int64_t* __restrict__ state,
                                                                     int64_t* __restrict__ confusion) {
  __shared__ unsigned tail[4];
  const int lane = threadIdx.x & 63;
  unsigned t_rows = 0, t_ign = 0, t_inv = 0;
  const int64_t step = (int64_t)gridDim.x * MT_THREADS;
  for (int64_t r0 = (int64_t)blockIdx.x * MT_THREADS + (threadIdx.x - lane); r0 < B; r0 += step) {
    const int64_t r = r0 + lane;
    bool valid = false, ignored = false, invalid = false;
    if (r < B) {
      const int64_t t = target[r];
      if (t == ignore_index) ignored = true;
      else {
        const int64_t q = pred[r];
        if (t < 0 || t >= C || q < 0 || q >= C) invalid = true;
        else {
          valid = true;
          mt_add(state + C + q, 1);
          mt_add(state + 2 * (int64_t)C + t, 1);
          if (q == t) mt_add(state + q, 1);
          if (confusion) mt_add(confusion + t * C + q, 1);
        }
      }
    }
    t_rows += (unsigned)__popcll(__ballot(valid));
    t_ign += (unsigned)__popcll(__ballot(ignored));
    t_inv += (unsigned)__popcll(__ballot(invalid));
  }
  mt_flush_tail(tail, t_rows, t_ign, t_inv, 0u, state, C);
}

// ---- score capture --------------------------------------------------------------------------------------------------------
// the bits of an element widened to float32 (bf16: exactly, denormals included; no float instruction touches the value)
__device__ __forceinline__ uint32_t sc_bits(const float* p) { return __builtin_bit_cast(uint32_t, *p); }
__device__ __forceinline__ uint32_t sc_bits(const bf16* p) { return (uint32_t)__builtin_bit_cast(uint16_t, *p) << 16; }
__device__ __forceinline__ bool sc_is_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }
// unsigned order of the keys = order of the floats: -0.0 first becomes +0.0, then non-negative values get the sign bit set and
// negative ones are complemented
__device__ __forceinline__ uint32_t sc_key(uint32_t b) {
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

template <typename T>
__global__ __launch_bounds__(MT_THREADS) void score_capture_kernel(const T* __restrict__ scores, int64_t ld, const int64_t* __restrict__ target,
                                                                    int64_t B, int C, int col0, int ncol, int64_t ignore_index,
                                                                    uint32_t* __restrict__ keys, int32_t* __restrict__ labels, int64_t capacity,
                                                                    int64_t offset, int64_t* __restrict__ counters) {
  __shared__ unsigned tail[4];
  const int lane = threadIdx.x & 63;
  unsigned t_rows = 0, t_ign = 0, t_inv = 0, t_nan = 0;
  const int64_t step = (int64_t)gridDim.x * MT_THREADS;
  for (int64_t r0 = (int64_t)blockIdx.x * MT_THREADS + (threadIdx.x - lane); r0 < B; r0 += step) {     // wave-uniform: ballots below
    const int64_t r = r0 + lane;
    bool valid = false, ignored = false, invalid = false, nan = false;
    if (r < B) {
      const int64_t t = target[r];
      const T* row = scores + r * ld + col0;
      if (t == ignore_index) ignored = true;
      else if (t < 0 || t >= C) invalid = true;
      else {
        for (int c = 0; c < ncol; ++c) nan = nan || sc_is_nan(sc_bits(row + c));
        valid = !nan;
      }
      const int64_t slot = offset + r;                 // offset + B <= capacity: inside the buffers
      labels[slot] = valid ? (int32_t)t : -1;
      for (int c = 0; c < ncol; ++c) keys[(int64_t)c * capacity + slot] = valid ? sc_key(sc_bits(row + c)) : 0u;
    }
    t_rows += (unsigned)__popcll(__ballot(valid));
    t_ign += (unsigned)__popcll(__ballot(ignored));
    t_inv += (unsigned)__popcll(__ballot(invalid));
    t_nan += (unsigned)__popcll(__ballot(nan));
  }
  mt_flush_tail(tail, t_rows, t_ign, t_inv, t_nan, counters, 0);
}

bool mt_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
constexpr int64_t MT_MAX_ROWS = 1ll << 40;             // a workgroup's 32-bit LDS counters hold its share of this many rows

unsigned mt_grid(int64_t work_items, int64_t cap) { return (unsigned)(work_items < cap ? work_items : cap); }

}  // namespace

extern "C" int meant_metrics_update(const void* scores, int64_t ld, int dtype, const int64_t* target, int64_t B, int C, int64_t ignore_index,
                                    int64_t* state, int64_t* confusion, void* stream) {
  MEANT_REQUIRE(scores && target && state && B >= 0 && C > 0 && ld >= C, MEANT_ERR_ARG,
                "metrics_update: bad argument (null scores / target / state, B=%lld < 0, C=%d <= 0 or ld=%lld < C)", (long long)B, C, (long long)ld);
  MEANT_REQUIRE(dtype == MEANT_F32 || dtype == MEANT_BF16, MEANT_ERR_ARG, "metrics_update: unknown dtype %d", dtype);
  MEANT_REQUIRE(mt_aligned(scores, dtype == MEANT_F32 ? 4 : 2) && mt_aligned(target, 8) && mt_aligned(state, 8) && mt_aligned(confusion, 8),
                MEANT_ERR_ARG, "metrics_update: operands must be aligned to their element size");
  MEANT_REQUIRE(B < MT_MAX_ROWS, MEANT_ERR_UNSUPPORTED, "metrics_update: B=%lld must be below 2^40 rows per call", (long long)B);
  if (B == 0) return MEANT_OK;
  hipStream_t st = (hipStream_t)stream;
  if (C <= MT_ROWS_MAXC) {
    const unsigned grid = mt_grid(ceil_div(B, MT_THREADS), MT_ROWS_MAXGRID);
    DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((metrics_rows_kernel<T, false>), dim3(grid), dim3(MT_THREADS), 0, st, (const T*)scores, ld,
                                                (const int64_t*)nullptr, target, B, C, ignore_index, state, confusion));
    MEANT_LAUNCH_CHECK("metrics_update (rows)");
    meant_route_hit(ROUTE_METRICS_ROWS);
    return MEANT_OK;
  }
  const int cus = meant_num_cus();
  const unsigned grid = mt_grid(ceil_div(B, MT_WAVES), (int64_t)(cus > 0 ? cus : 256) * MT_WAVE_WGS_PER_CU);
  const size_t esz = dtype == MEANT_F32 ? 4 : 2;
  const bool vec = meant_aligned16(scores) && ((size_t)ld * esz) % 16 == 0;                   // every row starts on 16 bytes
  DISPATCH_DTYPE(dtype, T, {
    if (vec)
      hipLaunchKernelGGL((metrics_wave_kernel<T, true>), dim3(grid), dim3(MT_WAVE_THREADS), 0, st, (const T*)scores, ld, target, B, C, ignore_index,
                         state, confusion);
    else
      hipLaunchKernelGGL((metrics_wave_kernel<T, false>), dim3(grid), dim3(MT_WAVE_THREADS), 0, st, (const T*)scores, ld, target, B, C, ignore_index,
                         state, confusion);
  });
  MEANT_LAUNCH_CHECK("metrics_update (wave)");
  meant_route_hit(ROUTE_METRICS_WAVE);
  return MEANT_OK;
}

extern "C" int meant_metrics_update_labels(const int64_t* pred, const int64_t* target, int64_t B, int C, int64_t ignore_index, int64_t* state,
                                           int64_t* confusion, void* stream) {
  MEANT_REQUIRE(pred && target && state && B >= 0 && C > 0, MEANT_ERR_ARG,
                "metrics_update_labels: bad argument (null pred / target / state, B=%lld < 0 or C=%d <= 0)", (long long)B, C);
  MEANT_REQUIRE(mt_aligned(pred, 8) && mt_aligned(target, 8) && mt_aligned(state, 8) && mt_aligned(confusion, 8), MEANT_ERR_ARG,
                "metrics_update_labels: operands must be aligned to their element size");
  MEANT_REQUIRE(B < MT_MAX_ROWS, MEANT_ERR_UNSUPPORTED, "metrics_update_labels: B=%lld must be below 2^40 rows per call", (long long)B);
  if (B == 0) return MEANT_OK;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = mt_grid(ceil_div(B, MT_THREADS), MT_ROWS_MAXGRID);
  if (C <= MT_ROWS_MAXC)
    hipLaunchKernelGGL((metrics_rows_kernel<float, true>), dim3(grid), dim3(MT_THREADS), 0, st, (const float*)nullptr, (int64_t)0, pred, target, B,
                       C, ignore_index, state, confusion);
  else
    hipLaunchKernelGGL(metrics_labels_kernel, dim3(grid), dim3(MT_THREADS), 0, st, pred, target, B, C, ignore_index, state, confusion);
  MEANT_LAUNCH_CHECK("metrics_update_labels");
  meant_route_hit(ROUTE_METRICS_LABELS);
  return MEANT_OK;
}

extern "C" int meant_score_capture(const void* scores, int64_t ld, int dtype, const int64_t* target, int64_t B, int C, int col0, int ncol,
                                   int64_t ignore_index, uint32_t* keys, int32_t* labels, int64_t capacity, int64_t offset,
                                   int64_t* counters, void* stream) {
  MEANT_REQUIRE(scores && target && keys && labels && counters, MEANT_ERR_ARG, "score_capture: null scores / target / keys / labels / counters");
  MEANT_REQUIRE(B >= 0 && C > 0 && ncol > 0 && col0 >= 0 && (int64_t)col0 + ncol <= ld, MEANT_ERR_ARG,
                "score_capture: bad argument (B=%lld < 0, C=%d <= 0, ncol=%d <= 0, col0=%d < 0 or col0 + ncol > ld=%lld)", (long long)B, C, ncol,
                col0, (long long)ld);
  MEANT_REQUIRE(offset >= 0 && capacity >= 0 && B <= capacity && offset <= capacity - B, MEANT_ERR_ARG,
                "score_capture: rows [%lld, %lld + %lld) do not fit the capacity %lld", (long long)offset, (long long)offset, (long long)B,
                (long long)capacity);
  MEANT_REQUIRE(dtype == MEANT_F32 || dtype == MEANT_BF16, MEANT_ERR_ARG, "score_capture: unknown dtype %d", dtype);
  MEANT_REQUIRE(mt_aligned(scores, dtype == MEANT_F32 ? 4 : 2) && mt_aligned(target, 8) && mt_aligned(keys, 4) && mt_aligned(labels, 4) &&
                    mt_aligned(counters, 8),
                MEANT_ERR_ARG, "score_capture: operands must be aligned to their element size");
  MEANT_REQUIRE(capacity < (1ll << 31), MEANT_ERR_UNSUPPORTED, "score_capture: capacity=%lld must be below 2^31", (long long)capacity);
  if (B == 0) return MEANT_OK;
  const unsigned grid = mt_grid(ceil_div(B, MT_THREADS), MT_ROWS_MAXGRID);
  DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(score_capture_kernel<T>, dim3(grid), dim3(MT_THREADS), 0, (hipStream_t)stream, (const T*)scores, ld,
                                              target, B, C, col0, ncol, ignore_index, keys, labels, capacity, offset, counters));
  MEANT_LAUNCH_CHECK("score_capture");
  meant_route_hit(ROUTE_SCORE_CAPTURE);
  return MEANT_OK;
}

extern "C" int meant_vqa_score_update(const void* scores, int64_t lds, int scores_dtype, const void* target, int64_t ldt, int target_dtype,
                                      int64_t B, int64_t C, int64_t* state, void* stream) {
  MEANT_REQUIRE(scores && target && state && B >= 0 && C > 0 && lds >= C && ldt >= C, MEANT_ERR_ARG,
                "vqa_score_update: bad argument (null scores / target / state, B=%lld < 0, C=%lld <= 0, lds=%lld or ldt=%lld below C)",
                (long long)B, (long long)C, (long long)lds, (long long)ldt);
  MEANT_REQUIRE((scores_dtype == MEANT_F32 || scores_dtype == MEANT_BF16) && (target_dtype == MEANT_F32 || target_dtype == MEANT_BF16),
                MEANT_ERR_ARG, "vqa_score_update: unknown dtype (scores %d, target %d)", scores_dtype, target_dtype);
  MEANT_REQUIRE(mt_aligned(scores, scores_dtype == MEANT_F32 ? 4 : 2) && mt_aligned(target, target_dtype == MEANT_F32 ? 4 : 2) &&
                    mt_aligned(state, 8),
                MEANT_ERR_ARG, "vqa_score_update: operands must be aligned to their element size");
  MEANT_REQUIRE(B < MT_MAX_ROWS && C <= INT_MAX, MEANT_ERR_UNSUPPORTED, "vqa_score_update: B=%lld must be below 2^40 rows per call and C=%lld below 2^31",
                (long long)B, (long long)C);
  if (B == 0) return MEANT_OK;
  const int cus = meant_num_cus();
  const unsigned grid = mt_grid(ceil_div(B, MT_WAVES), (int64_t)(cus > 0 ? cus : 256) * MT_WAVE_WGS_PER_CU);
  const size_t esz = scores_dtype == MEANT_F32 ? 4 : 2;
  const bool vec = meant_aligned16(scores) && ((size_t)lds * esz) % 16 == 0;                  // every row starts on 16 bytes
  const bool tbf = target_dtype == MEANT_BF16;
  DISPATCH_DTYPE(scores_dtype, T, {
    if (vec)
      hipLaunchKernelGGL((vqa_score_kernel<T, true>), dim3(grid), dim3(MT_WAVE_THREADS), 0, (hipStream_t)stream, (const T*)scores, lds, target, ldt,
                         tbf, B, (int)C, state);
    else
      hipLaunchKernelGGL((vqa_score_kernel<T, false>), dim3(grid), dim3(MT_WAVE_THREADS), 0, (hipStream_t)stream, (const T*)scores, lds, target, ldt,
                         tbf, B, (int)C, state);
  });
  MEANT_LAUNCH_CHECK("vqa_score_update");
  meant_route_hit(ROUTE_VQA_SCORE);
  return MEANT_OK;
}
