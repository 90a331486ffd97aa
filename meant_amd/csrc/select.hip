// Stable compaction of the labelled rows of an MLM batch (pretrain_mlm.py:160,178; utils/custom_datasets.py:46-54: 15 % of the
// positions carry a label, every other one the ignore index).  A row the loss ignores adds nothing to it and gets an all-zero
// gradient row, so the vocabulary head may run on the labelled rows alone; this makes the row lists for that, on the device.
//   * meant_select_rows -- idx (the labelled rows, ascending, -1 behind them), inv (a row's place in that list, or -1),
//                          target_sel (their labels, the ignore index behind them) and the count.
// Three small launches, all prefix sums, no atomics: the result depends on the labels alone.
//   count   : a workgroup owns SEL_SPAN consecutive rows, a wave SEL_WAVE_SPAN of them; labelled rows per wave by ballot + popcount,
//             per workgroup through LDS.
//   scan    : one workgroup turns the per-workgroup counts into exclusive offsets, SEL_THREADS at a time with a running carry, and
//             leaves the total in count[0].
//   scatter : the same ballots again; a row's place = offset of its workgroup + labelled rows of the earlier waves and rounds +
//             popcount of the ballot below its lane.  Rows t >= n of idx / target_sel get the tail values from thread t.
#include "common.h"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_ROUNDS = 4;                          // 64-row rounds per wave
constexpr int SEL_WAVE_SPAN = 64 * SEL_ROUNDS;
constexpr int SEL_SPAN = (SEL_THREADS / 64) * SEL_WAVE_SPAN;      // rows per workgroup


__device__ __forceinline__ bool sel_labelled(int64_t t, int64_t V, int64_t ignore_index) {
  return t != ignore_index && t >= 0 && t < V;        // the predicate of softmax_ce_fwd / _bwd (optim.hip)
}

__global__ __launch_bounds__(SEL_THREADS) void select_count_kernel(const int64_t* __restrict__ target, int64_t T, int64_t V,
                                                                    int64_t ignore_index, uint32_t* __restrict__ wg_count) {
  __shared__ uint32_t wsum[SEL_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * SEL_SPAN + wave * SEL_WAVE_SPAN;
  uint32_t c = 0;
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r) {
    const int64_t t = base + r * 64 + lane;
    c += (uint32_t)__popcll(__ballot(t < T && sel_labelled(target[t < T ? t : T - 1], V, ignore_index)));
  }
  if (lane == 0) wsum[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) wg_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// exclusive scan of the per-workgroup counts in place, by one workgroup; count[0] = their sum
__global__ __launch_bounds__(SEL_THREADS) void select_scan_kernel(uint32_t* __restrict__ wg_count, int64_t nwg, int32_t* __restrict__ count) {
  __shared__ uint32_t wsum[SEL_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t carry = 0;
  for (int64_t b0 = 0; b0 < nwg; b0 += SEL_THREADS) {
    const int64_t b = b0 + tid;
    const uint32_t x = b < nwg ? wg_count[b] : 0u;
    uint32_t incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    if (b < nwg) wg_count[b] = carry + before + incl - x;
    carry += total;
    __syncthreads();                                   // wsum is rewritten by the next chunk
  }
  if (tid == 0) count[0] = (int32_t)carry;
}

__global__ __launch_bounds__(SEL_THREADS) void select_scatter_kernel(const int64_t* __restrict__ target, int64_t T, int64_t V,
                                                                      int64_t ignore_index, const uint32_t* __restrict__ wg_off,
                                                                      const int32_t* __restrict__ count, int32_t* __restrict__ idx,
                                                                      int32_t* __restrict__ inv, int64_t* __restrict__ target_sel) {
  __shared__ uint32_t wsum[SEL_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * SEL_SPAN + wave * SEL_WAVE_SPAN;
  const int64_t n = count[0];
  int64_t lab[SEL_ROUNDS];
  unsigned long long bal[SEL_ROUNDS];
  uint32_t c = 0;
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r) {
    const int64_t t = base + r * 64 + lane;
    lab[r] = target[t < T ? t : T - 1];
    bal[r] = __ballot(t < T && sel_labelled(lab[r], V, ignore_index));
    c += (uint32_t)__popcll(bal[r]);
  }
  if (lane == 0) wsum[wave] = c;
  __syncthreads();
  int64_t pos0 = wg_off[blockIdx.x];
  for (int w = 0; w < wave; ++w) pos0 += wsum[w];
#pragma unroll
  for (int r = 0; r < SEL_ROUNDS; ++r) {
    const int64_t t = base + r * 64 + lane;
    if (t < T) {
      const bool mine = (bal[r] >> lane) & 1ull;
      const int64_t pos = pos0 + __popcll(bal[r] & ((1ull << lane) - 1ull));
      if (mine && pos < n) {                           // pos < n always holds with consistent counts; never write outside the arrays
        idx[pos] = (int32_t)t;
        target_sel[pos] = lab[r];
      }
      inv[t] = mine && pos < n ? (int32_t)pos : -1;
      if (t >= n) {                                    // the tails: places n .. T-1 belong to nobody else
        idx[t] = -1;
        target_sel[t] = ignore_index;
      }
    }
    pos0 += __popcll(bal[r]);
  }
}

}  // namespace

extern "C" size_t meant_select_rows_ws(int64_t T) {
  if (T <= 0 || T >= (1ll << 31)) return 0;
  return align256((size_t)ceil_div(T, SEL_SPAN) * sizeof(uint32_t));
}

extern "C" int meant_select_rows(const int64_t* target, int64_t T, int64_t V, int64_t ignore_index, int32_t* idx, int32_t* inv,
                                 int64_t* target_sel, int32_t* count, void* workspace, size_t workspace_bytes, void* stream) {
  MEANT_REQUIRE(target && idx && inv && target_sel && count && T > 0 && V > 0, MEANT_ERR_ARG, "select_rows: bad argument");
  MEANT_REQUIRE(T < (1ll << 31), MEANT_ERR_UNSUPPORTED, "select_rows: T=%lld must be below 2^31", (long long)T);
  const size_t need = meant_select_rows_ws(T);
  {
    struct Span { const char* p; size_t len; };
    const Span s[6] = {{(const char*)target, (size_t)T * 8}, {(const char*)idx, (size_t)T * 4}, {(const char*)inv, (size_t)T * 4},
                       {(const char*)target_sel, (size_t)T * 8}, {(const char*)count, 4}, {(const char*)workspace, workspace ? need : 0}};
    for (int i = 0; i < 6; ++i)
      for (int j = i + 1; j < 6; ++j)
        MEANT_REQUIRE(!(s[i].p < s[j].p + s[j].len && s[j].p < s[i].p + s[i].len), MEANT_ERR_ARG,
                      "select_rows: target, idx, inv, target_sel, count and the workspace must not overlap");
  }
  MEANT_REQUIRE(workspace && workspace_bytes >= need, MEANT_ERR_WORKSPACE, "select_rows: workspace of %zu bytes needed, %zu given", need,
                workspace_bytes);
  MEANT_REQUIRE((reinterpret_cast<uintptr_t>(target) & 7) == 0 && (reinterpret_cast<uintptr_t>(target_sel) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(idx) & 3) == 0 && (reinterpret_cast<uintptr_t>(inv) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(count) & 3) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
                MEANT_ERR_ARG, "select_rows: operands must be aligned to their element size");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nwg = ceil_div(T, SEL_SPAN);
  uint32_t* wg = (uint32_t*)workspace;
  hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)nwg), dim3(SEL_THREADS), 0, st, target, T, V, ignore_index, wg);
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_THREADS), 0, st, wg, nwg, count);
  hipLaunchKernelGGL(select_scatter_kernel, dim3((unsigned)nwg), dim3(SEL_THREADS), 0, st, target, T, V, ignore_index, (const uint32_t*)wg,
                     (const int32_t*)count, idx, inv, target_sel);
  MEANT_LAUNCH_CHECK("select_rows");
  meant_route_hit(ROUTE_SELECT_ROWS);
  return MEANT_OK;
}
