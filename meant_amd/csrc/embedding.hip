// Embedding: the gather, and the gradient three ways.
//   meant_embedding_fwd                 one wave per token row
//   meant_embedding_bwd                 scatter-add with f32 atomics
//   meant_embedding_bwd_sorted[_range]  over ids sorted by the caller, d <= 1024: runs of equal ids summed in registers (seg_walk of
//                                       seg_sum.h, as meant_embedding_bwd_seg), atomics only where a run crosses a wave's stretch
//   meant_sort_ids                      LSD radix sort over 8-bit digits of the ids clamped into [0, V); equal ids keep their row order
//   sort_u32_launch (internal.h)        the same passes over caller-made 32-bit keys with a 32-bit value each (auroc.hip)
//   meant_embedding_bwd_seg             dtable[id, :] += sum of the rows of dout that carry id, any d % 8 == 0, no float atomics,
//                                       bit-reproducible ("Embedding gradient at any width")
#include "common.h"
#include "internal.h"

#define EMB_REQ(c, ...) MEANT_REQUIRE(c, MEANT_ERR_ARG, __VA_ARGS__)

namespace {

// ------------------------------------------------------------------------------------------------
// The sort.  A tile is 2048 consecutive entries of a pass's input, owned by one workgroup; wave w of it owns entries
// [512 w, 512 w + 512) and takes them in eight rounds of 64, lane l the l-th of a round, so (tile, wave, round, lane) is the input
// order.  Per pass:  tile counts [digit][tile]  ->  exclusive scan in (digit, tile) order  ->  stable scatter.  The digit totals of
// EVERY pass do not depend on the order of the entries: one kernel over the ids counts them all (integer atomics on 4 x 256
// counters, the only atomics here), together with the tile counts of pass 0.  The tile counts of a later pass are those of the
// previous pass's output and are counted from it.  Nothing waits on another workgroup and no position comes from an atomic, so the
// result does not depend on timing.
constexpr int SORT_TILE = 2048, SORT_WAVE_SPAN = 512, SORT_ROUNDS = 8;

__device__ __forceinline__ uint32_t sort_key(int64_t id, int64_t V) {     // clamped as meant_embedding_fwd clamps
  return (uint32_t)(id < 0 ? 0 : (id >= V ? V - 1 : id));
}

// ghist[p][digit] += occurrences of digit p of every key (all passes); tile_hist[digit][tile] = pass 0's tile counts.
// IDS: the keys are the clamped ids, otherwise the caller's `keys`
template <bool IDS>
__global__ __launch_bounds__(256) void sort_hist_kernel(const int64_t* __restrict__ ids, const uint32_t* __restrict__ keys, int64_t n, int64_t V,
                                                         int passes, uint32_t* __restrict__ ghist, uint32_t* __restrict__ tile_hist,
                                                         int64_t ntiles) {
  __shared__ uint32_t h[4][256];
  const int tid = threadIdx.x;
#pragma unroll
  for (int p = 0; p < 4; ++p) h[p][tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
  for (int i = 0; i < SORT_TILE / 256; ++i) {
    const int64_t j = base + i * 256 + tid;
    if (j < n) {
      const uint32_t key = IDS ? sort_key(ids[j], V) : keys[j];
      for (int p = 0; p < passes; ++p) atomicAdd(&h[p][(key >> (8 * p)) & 255u], 1u);
    }
  }
  __syncthreads();
  tile_hist[(int64_t)tid * ntiles + blockIdx.x] = h[0][tid];
  for (int p = 0; p < passes; ++p)
    if (h[p][tid]) atomicAdd(&ghist[p * 256 + tid], h[p][tid]);
}

// tile counts of a later pass, from the keys as the previous pass left them
__global__ __launch_bounds__(256) void sort_count_kernel(const uint32_t* __restrict__ keys, int64_t n, int shift,
                                                          uint32_t* __restrict__ tile_hist, int64_t ntiles) {
  __shared__ uint32_t h[256];
  const int tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SORT_TILE;
  for (int i = 0; i < SORT_TILE / 256; ++i) {
    const int64_t j = base + i * 256 + tid;
    if (j < n) atomicAdd(&h[(keys[j] >> shift) & 255u], 1u);
  }
  __syncthreads();
  tile_hist[(int64_t)tid * ntiles + blockIdx.x] = h[tid];
}

// tile_hist[digit][tile] -> first output position of that tile's entries with that digit.  One workgroup per digit: its base is
// the total of the smaller digits (ghist), then an exclusive scan along the tiles.
__global__ __launch_bounds__(256) void sort_scan_kernel(const uint32_t* __restrict__ ghist, uint32_t* __restrict__ tile_hist, int64_t ntiles) {
  __shared__ uint32_t wsum[4];
  const int tid = threadIdx.x, digit = blockIdx.x;
  uint32_t carry;
  block_scan_incl(tid < digit ? ghist[tid] : 0u, wsum, &carry);
  uint32_t* row = tile_hist + (int64_t)digit * ntiles;
  for (int64_t t0 = 0; t0 < ntiles; t0 += 256) {
    const int64_t t = t0 + tid;
    const uint32_t x = t < ntiles ? row[t] : 0u;
    uint32_t total;
    const uint32_t incl = block_scan_incl(x, wsum, &total);
    if (t < ntiles) row[t] = carry + incl - x;
    carry += total;
  }
}

// stable scatter of one pass.  Rank of an entry among the equal digits of its round: a match mask from eight wave ballots and a
// population count below the lane; among the earlier rounds of its wave: a running per-wave count in LDS, advanced by the lowest
// lane of each match group; among the earlier waves and tiles: the scanned counts.
// FIRST: keys are the clamped ids and the values the row numbers; LAST: the outputs are the caller's int64 arrays.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void sort_scatter_kernel(const int64_t* __restrict__ ids, const uint32_t* __restrict__ kin,
                                                            const uint32_t* __restrict__ vin, int64_t n, int64_t V, int shift,
                                                            const uint32_t* __restrict__ tile_off, int64_t ntiles,
                                                            uint32_t* __restrict__ kout, uint32_t* __restrict__ vout,
                                                            int64_t* __restrict__ sorted_ids, int64_t* __restrict__ order) {
  __shared__ uint32_t cnt[4][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int w = 0; w < 4; ++w) cnt[w][tid] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SORT_TILE + wave * SORT_WAVE_SPAN;
  uint32_t key[SORT_ROUNDS], val[SORT_ROUNDS], rk[SORT_ROUNDS];
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t j = base + r * 64 + lane;
    const bool valid = j < n;
    key[r] = valid ? (FIRST ? sort_key(ids[j], V) : kin[j]) : 0u;
    val[r] = valid ? (FIRST ? (uint32_t)j : vin[j]) : 0u;
    const uint32_t dig = (key[r] >> shift) & 255u;
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (dig >> b) & 1u;
      const unsigned long long bal = __ballot(valid && bit);
      m &= bit ? bal : ~bal;
    }
    const unsigned long long below = m & ((1ull << lane) - 1ull);
    rk[r] = valid ? cnt[wave][dig] + (uint32_t)__popcll(below) : 0u;
    __syncthreads();
    if (valid && below == 0) cnt[wave][dig] += (uint32_t)__popcll(m);
    __syncthreads();
  }
  {                                                    // per-wave counts of digit `tid` -> first output position of each wave's share
    uint32_t o = tile_off[(int64_t)tid * ntiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t c = cnt[w][tid];
      cnt[w][tid] = o;
      o += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t j = base + r * 64 + lane;
    if (j >= n) continue;
    const int64_t pos = (int64_t)cnt[wave][(key[r] >> shift) & 255u] + rk[r];
    if (pos >= n) continue;                            // cannot happen with consistent counts; never write outside the arrays
    if (LAST) {
      sorted_ids[pos] = (int64_t)key[r];
      order[pos] = (int64_t)val[r];
    } else {
      kout[pos] = key[r];
      vout[pos] = val[r];
    }
  }
}

int sort_passes(int64_t V) {
  int bits = 0;
  for (uint64_t m = (uint64_t)(V - 1); m; m >>= 1) ++bits;
  const int p = (bits + 7) / 8;
  return p < 1 ? 1 : p;
}
struct SortWs { size_t ghist, tile_hist, buf[2], total; int nbuf; };
SortWs sort_ws_layout(int64_t n, int passes) {
  SortWs w;
  const int64_t ntiles = ceil_div(n, SORT_TILE);
  w.nbuf = passes - 1 < 2 ? passes - 1 : 2;            // the last pass writes the caller's arrays
  size_t off = 0;
  w.ghist = off; off += align256(4 * 256 * sizeof(uint32_t));
  w.tile_hist = off; off += align256((size_t)ntiles * 256 * sizeof(uint32_t));
  for (int i = 0; i < 2; ++i) {
    w.buf[i] = off;
    if (i < w.nbuf) off += 2 * align256((size_t)n * sizeof(uint32_t));
  }
  w.total = off;
  return w;
}

// ------------------------------------------------------------------------------------------------
// The reduction at any width: seg_walk (seg_sum.h) over a stretch of 256 sorted entries.  grid.y cuts the row into column blocks of
// at most 128 8-column chunks, so a lane still owns two chunks.  A run inside the stretch is a plain read-modify-write of its table
// row.  The runs that cross the stretch's ends: their partial sums go to the workspace slot [stretch][0] (the run came in from the
// left) or [stretch][1] (it starts here and leaves to the right), and seg_cross_kernel / seg_long_kernel (seg_sum.h) add each such
// run's slots in an order that depends on the sorted ids alone.
#include "seg_sum.h"      // SEG, the walk, and the crossing-run passes seg_cross_kernel / seg_long_kernel
template <typename T>
__global__ __launch_bounds__(256) void emb_seg_kernel(const T* __restrict__ dout, const int64_t* __restrict__ sorted_ids,
                                                       const int64_t* __restrict__ order, float* __restrict__ dtable,
                                                       float* __restrict__ part, int64_t n, int64_t d, int64_t V, int64_t id_lo,
                                                       int64_t id_hi, int cb_chunks) {
  const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t j0 = s * SEG;
  if (j0 >= n) return;
  const int64_t j1 = j0 + SEG < n ? j0 + SEG : n;
  if (sorted_ids[j1 - 1] < id_lo || sorted_ids[j0] >= id_hi) return;     // the ids are sorted: a stretch outside the range leaves at once
  const SegSlotSink<SegAddRow> sink{{dtable, id_lo, id_hi}, part + s * 2 * d, d};
  seg_walk<false>(dout, d, sorted_ids, order, n, V, j0, j1, seg_cols(d, cb_chunks), SegAllRows{}, sink, nullptr);
}

size_t seg_part_bytes(int64_t n, int64_t d) { return (size_t)ceil_div(n, SEG) * 2 * (size_t)d * sizeof(float); }

// ------------------------------------------------------------------------------------------------
// embedding gather (one wave per token row) and scatter-add of its gradient (f32 atomics)
// a lane moves one 8-column chunk (VEC) or, at d % 8 != 0 (rows of the table and of `out` are then only element-aligned), one column: a
// chunk of which one element is real, so a wave's lanes walk consecutive columns of its row
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void embedding_fwd_kernel(const float* __restrict__ table, const int64_t* __restrict__ ids,
                                                             T* __restrict__ out, int64_t n, int d, int64_t V) {
  constexpr int PER = VEC ? 8 : 1;                     // columns per lane
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nch = VEC ? d >> 3 : d;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
    int64_t id = ids[r];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    const float* src = table + id * d;
    for (int ch = lane; ch < nch; ch += 64) {
      const Vec8<float> v = load8n<VEC>(src + ch * PER, 1);
      Vec8<T> o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o.set(k, v.get(k));
      store8n<VEC, true>(out + r * d + ch * PER, o, 1);
    }
  }
}
template <typename T>
__global__ __launch_bounds__(256) void embedding_bwd_kernel(const T* __restrict__ dout, const int64_t* __restrict__ ids,
                                                             float* __restrict__ dtable, int64_t n, int d, int64_t V) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
    int64_t id = ids[r];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    float* dst = dtable + id * d;
    for (int e = lane; e < d; e += 64) atomicAdd(dst + e, to_f(dout[r * d + e]));   // 256 contiguous bytes per wave-instruction
  }
}

// scatter-add of the embedding gradient over ids SORTED by the caller (order[j] = original row of the j-th smallest id), d <= 1024:
// seg_walk (seg_sum.h) over SEG consecutive sorted entries, the lane's chunks `lane` and `lane + 64` covering the whole row.  A run
// that lies entirely inside the wave's stretch belongs to nobody else: its sum is added with a plain read-modify-write.  Only the (at
// most two) runs that cross the stretch's ends use float atomics -- at 12 tokens per id that is one row in eleven (the atomic rate,
// 1.3 TB/s of added bytes, was a third of this kernel's time when every run went that way, and 2-byte loads most of the rest).
struct EmbAtomicSink : SegSlotSink<SegAddRow> {
  __device__ __forceinline__ void cross(int64_t id, int, int64_t col, f32x4 lo, f32x4 hi) const {
    float* dst = st.dtable + id * ld + col;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      atomicAdd(dst + e, lo[e]);
      atomicAdd(dst + 4 + e, hi[e]);
    }
  }
};
template <typename T>
__global__ __launch_bounds__(256) void embedding_bwd_sorted_kernel(const T* __restrict__ dout, const int64_t* __restrict__ sorted_ids,
                                                                    const int64_t* __restrict__ order, float* __restrict__ dtable,
                                                                    int64_t n, int64_t d, int64_t V, int det, int64_t id_lo, int64_t id_hi) {
  int64_t j0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * SEG;
  if (j0 >= n) return;
  int64_t j1 = j0 + SEG < n ? j0 + SEG : n;
  // [id_lo, id_hi): only the rows of this id range are produced (meant_embedding_bwd_sorted_range: the table's gradient in row
  // slices, each handed to its collective as soon as it is final).  The ids are sorted: a stretch outside the range leaves at once.
  if (sorted_ids[j1 - 1] < id_lo || sorted_ids[j0] >= id_hi) return;
  if (det) {
    // option "deterministic": no atomics.  A run belongs to the wave in whose stretch it STARTS: that wave follows it to its end
    // (however far), the others skip the part of their stretch that continues an earlier run.  Slow for a hot id; a debugging mode.
    // After this no run crosses an end of [j0, j1), so the walk meets none that would go to the atomics.
    if (j0 > 0) {
      const int64_t prev = sorted_ids[j0 - 1];
      while (j0 < j1 && sorted_ids[j0] == prev) ++j0;
      if (j0 == j1) return;
    }
    const int64_t last = sorted_ids[j1 - 1];
    while (j1 < n && sorted_ids[j1] == last) ++j1;
  }
  const EmbAtomicSink sink{{{dtable, id_lo, id_hi}, nullptr, d}};
  seg_walk<false>(dout, d, sorted_ids, order, n, V, j0, j1, seg_cols(d, 128), SegAllRows{}, sink, nullptr);
}

}  // namespace

// The passes of one sort, over the clamped `ids` into the int64 arrays (sorted_ids, order) or over the caller's 32-bit (keys, vals)
// into (keys_out, vals_out): the same kernels either way, only the first pass's reads and the last pass's writes differ.
static int sort_run(const int64_t* ids, int64_t V, const uint32_t* keys, const uint32_t* vals, int64_t n, int passes, int64_t* sorted_ids,
                    int64_t* order, uint32_t* keys_out, uint32_t* vals_out, const SortWs& w, char* base, hipStream_t st, const char* what) {
  const bool from_ids = ids != nullptr;
  uint32_t* ghist = (uint32_t*)(base + w.ghist);
  uint32_t* tile_hist = (uint32_t*)(base + w.tile_hist);
  uint32_t* bk[2] = {nullptr, nullptr};
  uint32_t* bv[2] = {nullptr, nullptr};
  for (int i = 0; i < w.nbuf; ++i) {
    bk[i] = (uint32_t*)(base + w.buf[i]);
    bv[i] = (uint32_t*)(base + w.buf[i] + align256((size_t)n * sizeof(uint32_t)));
  }
  const int64_t ntiles = ceil_div(n, SORT_TILE);
  const dim3 grid((unsigned)ntiles), block(256);
  const hipError_t e = hipMemsetAsync(ghist, 0, 4 * 256 * sizeof(uint32_t), st);
  MEANT_REQUIRE(e == hipSuccess, MEANT_ERR_LAUNCH, "%s: clearing the digit counters failed: %s", what, hipGetErrorString(e));
  if (from_ids) hipLaunchKernelGGL(sort_hist_kernel<true>, grid, block, 0, st, ids, keys, n, V, passes, ghist, tile_hist, ntiles);
  else hipLaunchKernelGGL(sort_hist_kernel<false>, grid, block, 0, st, ids, keys, n, V, passes, ghist, tile_hist, ntiles);
  for (int p = 0; p < passes; ++p) {
    const bool first = p == 0, last = p == passes - 1;
    const uint32_t* kin = first ? keys : bk[(p - 1) & 1];
    const uint32_t* vin = first ? vals : bv[(p - 1) & 1];
    uint32_t* kout = last ? keys_out : bk[p & 1];
    uint32_t* vout = last ? vals_out : bv[p & 1];
    const int shift = 8 * p;
    if (!first) hipLaunchKernelGGL(sort_count_kernel, grid, block, 0, st, kin, n, shift, tile_hist, ntiles);
    hipLaunchKernelGGL(sort_scan_kernel, dim3(256), block, 0, st, (const uint32_t*)(ghist + p * 256), tile_hist, ntiles);
#define SORT_SCATTER(F, L)                                                                                                     \
  hipLaunchKernelGGL((sort_scatter_kernel<F, L>), grid, block, 0, st, ids, kin, vin, n, V, shift, (const uint32_t*)tile_hist, \
                     ntiles, kout, vout, sorted_ids, order)
    const bool F = first && from_ids, L = last && from_ids;                // the int64 ends of meant_sort_ids
    if (F && L) SORT_SCATTER(true, true);
    else if (F) SORT_SCATTER(true, false);
    else if (L) SORT_SCATTER(false, true);
    else SORT_SCATTER(false, false);
#undef SORT_SCATTER
  }
  MEANT_LAUNCH_CHECK(what);
  return MEANT_OK;
}

extern "C" size_t meant_sort_ids_ws(int64_t n, int64_t V) {
  if (n <= 0 || V <= 0 || n >= (1ll << 31) || V >= (1ll << 31)) return 0;
  return sort_ws_layout(n, sort_passes(V)).total;
}

extern "C" int meant_sort_ids(const int64_t* ids, int64_t n, int64_t V, int64_t* sorted_ids, int64_t* order, void* workspace,
                              size_t workspace_bytes, void* stream) {
  EMB_REQ(ids && sorted_ids && order && n > 0 && V > 0, "sort_ids: bad argument");
  MEANT_REQUIRE(n < (1ll << 31) && V < (1ll << 31), MEANT_ERR_UNSUPPORTED, "sort_ids: n=%lld and V=%lld must be below 2^31", (long long)n,
                (long long)V);
  // not in place: the first pass still reads ids while the last may already write the outputs (one pass: the same kernel)
  {
    const char *a = (const char*)ids, *o1 = (const char*)sorted_ids, *o2 = (const char*)order;
    const size_t len = (size_t)n * sizeof(int64_t);
    const auto overlap = [len](const char* x, const char* y) { return x < y + len && y < x + len; };
    EMB_REQ(!overlap(a, o1) && !overlap(a, o2) && !overlap(o1, o2), "sort_ids: ids, sorted_ids and order must not overlap");
  }
  const int passes = sort_passes(V);
  const SortWs w = sort_ws_layout(n, passes);
  MEANT_REQUIRE(workspace && workspace_bytes >= w.total, MEANT_ERR_WORKSPACE, "sort_ids: workspace of %zu bytes needed, %zu given", w.total, workspace_bytes);
  EMB_REQ((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "sort_ids: 4-byte workspace alignment");
  const int rc = sort_run(ids, V, nullptr, nullptr, n, passes, sorted_ids, order, nullptr, nullptr, w, (char*)workspace, (hipStream_t)stream, "sort_ids");
  if (rc != MEANT_OK) return rc;
  meant_route_hit(ROUTE_SORT_IDS);
  return MEANT_OK;
}

size_t sort_u32_ws(int64_t n) { return n <= 0 || n >= (1ll << 31) ? 0 : sort_ws_layout(n, 4).total; }

int sort_u32_launch(const uint32_t* keys, const uint32_t* vals, int64_t n, uint32_t* keys_out, uint32_t* vals_out, void* ws, size_t ws_bytes,
                    hipStream_t stream) {
  EMB_REQ(keys && vals && keys_out && vals_out && n > 0 && n < (1ll << 31), "sort_u32: bad argument");
  const SortWs w = sort_ws_layout(n, 4);
  MEANT_REQUIRE(ws && ws_bytes >= w.total, MEANT_ERR_WORKSPACE, "sort_u32: workspace of %zu bytes needed, %zu given", w.total, ws_bytes);
  EMB_REQ((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "sort_u32: 4-byte workspace alignment");
  return sort_run(nullptr, 0, keys, vals, n, 4, nullptr, nullptr, keys_out, vals_out, w, (char*)ws, stream, "sort_u32");
}

extern "C" size_t meant_embedding_bwd_seg_ws(int64_t n, int64_t d) {
  if (n <= 0 || d <= 0) return 0;
  return seg_part_bytes(n, d) + align256((size_t)ceil_div(n, SEG) * sizeof(int));      // partial sums [stretch][2][d], then longk [stretch]
}

extern "C" int meant_embedding_bwd_seg(const void* dout, const int64_t* sorted_ids, const int64_t* order, float* dtable, int64_t n,
                                       int64_t d, int64_t V, int64_t id_lo, int64_t id_hi, int dtype, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  EMB_REQ(dout && sorted_ids && order && dtable && n > 0 && d > 0 && V > 0 && 0 <= id_lo && id_lo <= id_hi && id_hi <= V,
          "embedding_bwd_seg: bad argument");
  MEANT_REQUIRE(d % 8 == 0, MEANT_ERR_UNSUPPORTED, "embedding_bwd_seg: d=%lld must be a multiple of 8", (long long)d);
  MEANT_REQUIRE(d < (1ll << 22), MEANT_ERR_UNSUPPORTED, "embedding_bwd_seg: d=%lld is beyond the launch grid (d < 2^22)", (long long)d);
  const size_t need = meant_embedding_bwd_seg_ws(n, d);
  MEANT_REQUIRE(workspace && workspace_bytes >= need, MEANT_ERR_WORKSPACE, "embedding_bwd_seg: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
  EMB_REQ(meant_aligned16(dout) && meant_aligned16(dtable) && meant_aligned16(workspace), "embedding_bwd_seg: 16-byte alignment");
  if (id_lo == id_hi) return MEANT_OK;
  const SegColBlocks cb = seg_col_blocks(d, 2);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_DTYPE(dtype, T,
                 hipLaunchKernelGGL(emb_seg_kernel<T>, dim3((unsigned)ceil_div(ceil_div(n, SEG), 4), (unsigned)cb.ncb), dim3(256), 0, st, (const T*)dout,
                                    sorted_ids, order, dtable, (float*)workspace, n, d, V, id_lo, id_hi, cb.cb_chunks));
  seg_cross_launch(SegAddRow{dtable, id_lo, id_hi}, sorted_ids, (const float*)workspace, (int*)((char*)workspace + seg_part_bytes(n, d)), n, d, V, st);
  MEANT_LAUNCH_CHECK("embedding_bwd_seg");
  meant_route_hit(ROUTE_EMB_SEG);
  return MEANT_OK;
}

extern "C" int meant_embedding_fwd(const float* table, const int64_t* ids, void* out, int64_t n, int64_t d, int64_t V, int dtype, void* stream) {
  EMB_REQ(table && ids && out && n > 0 && d > 0 && d < (1ll << 30) && V > 0, "embedding_fwd: bad argument");
  int64_t nb = ceil_div(n, 4); if (nb > 8192) nb = 8192;
  DISPATCH_DTYPE_VEC(dtype, d % 8 == 0, T, VEC, hipLaunchKernelGGL((embedding_fwd_kernel<T, VEC>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                                                                   table, ids, (T*)out, n, (int)d, V));
  MEANT_LAUNCH_CHECK("embedding_fwd");
  return MEANT_OK;
}
// the sorted scatter-add over the ids of [id_lo, id_hi), behind both entries
static int emb_sorted_launch(const char* what, const void* dout, const int64_t* sorted_ids, const int64_t* order, float* dtable, int64_t n,
                             int64_t d, int64_t V, int64_t id_lo, int64_t id_hi, int dtype, void* stream) {
  EMB_REQ(dout && sorted_ids && order && dtable && n > 0 && d > 0 && V > 0 && 0 <= id_lo && id_lo <= id_hi && id_hi <= V, "%s: bad argument", what);
  MEANT_REQUIRE(d <= 1024 && d % 8 == 0, MEANT_ERR_UNSUPPORTED, "%s: d=%lld must be a multiple of 8 and <= 1024", what, (long long)d);
  EMB_REQ(meant_aligned16(dout) && meant_aligned16(dtable), "%s: 16-byte alignment", what);
  if (id_lo == id_hi) return MEANT_OK;
  DISPATCH_DTYPE(dtype, T,
                 hipLaunchKernelGGL(embedding_bwd_sorted_kernel<T>, dim3((unsigned)ceil_div(n, 4 * SEG)), dim3(256), 0, (hipStream_t)stream,
                                    (const T*)dout, sorted_ids, order, dtable, n, d, V, meant_opt(MEANT_OPT_DETERMINISTIC) != 0, id_lo, id_hi));
  MEANT_LAUNCH_CHECK(what);
  return MEANT_OK;
}

extern "C" int meant_embedding_bwd_sorted(const void* dout, const int64_t* sorted_ids, const int64_t* order, float* dtable, int64_t n,
                                          int64_t d, int64_t V, int dtype, void* stream) {
  return emb_sorted_launch("embedding_bwd_sorted", dout, sorted_ids, order, dtable, n, d, V, 0, V, dtype, stream);
}

extern "C" int meant_embedding_bwd_sorted_range(const void* dout, const int64_t* sorted_ids, const int64_t* order, float* dtable, int64_t n,
                                                int64_t d, int64_t V, int64_t id_lo, int64_t id_hi, int dtype, void* stream) {
  return emb_sorted_launch("embedding_bwd_sorted_range", dout, sorted_ids, order, dtable, n, d, V, id_lo, id_hi, dtype, stream);
}

extern "C" int meant_embedding_bwd(const void* dout, const int64_t* ids, float* dtable, int64_t n, int64_t d, int64_t V, int dtype, void* stream) {
  EMB_REQ(dout && ids && dtable && n > 0 && d > 0 && V > 0, "embedding_bwd: bad argument");
  int64_t nb = ceil_div(n, 4); if (nb > 8192) nb = 8192;
  DISPATCH_DTYPE(dtype, T,
                 hipLaunchKernelGGL(embedding_bwd_kernel<T>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const T*)dout, ids, dtable, n, (int)d, V));
  MEANT_LAUNCH_CHECK("embedding_bwd");
  return MEANT_OK;
}
