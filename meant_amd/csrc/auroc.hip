// AUROC as an exact rank statistic (utils/f1_metrics.py:3 imports torchmetrics' AUROC; train.py:63-65, 103-117 report it).
//   meant_auroc_rank   out = (2U, P, N) of one class's captured keys (meant_score_capture, metrics.hip) against the labels:
//                      2U = sum over (positive i, negative j) of 2 [key_j < key_i] + [key_j == key_i]
// The keys are sorted with the radix sort of embedding.hip (sort_u32_launch), each carrying its class code (0 negative, 1 positive,
// 2 left out).  Over the sorted array, with NP / PP the exclusive counts of negatives / positives before an entry and start(j) the
// first entry of j's run of equal keys,
//   2U = sum over positives of NP[start(j)] + sum over negatives of (P - PP[start(j)]).
// NP and PP never decrease along the array, so "the value at the start of my run" is a running maximum over the run heads at or before
// me: a scan like the counts themselves.  Three kernels over tiles of 2048 entries (a thread owns 8 consecutive ones):
//   tile   the tile's counts and the counts at its last run head                       (tile sums)
//   scan   one workgroup: exclusive sums of the counts along the tiles, the running maximum of the heads, P and N   (scan of the sums)
//   apply  each tile again with its offsets; a workgroup adds its share of 2U with ONE integer atomic               (apply)
// No position comes from an atomic, nothing waits on another workgroup, every quantity is an integer: the result does not depend on
// timing or on the order the sort leaves equal keys in.
#include "common.h"
#include "internal.h"

namespace {

constexpr int AR_TILE = 2048, AR_PER = 8;              // 256 threads x 8 entries
constexpr uint32_t AR_NEG = 0, AR_POS = 1, AR_OUT = 2;
typedef unsigned long long u64;

size_t ar_align(size_t x) { return (x + 255) & ~(size_t)255; }
struct AurocWs { size_t vals, skeys, svals, tile[4], sort, total; };
AurocWs ar_layout(int64_t n) {
  AurocWs w;
  const size_t arr = ar_align((size_t)n * sizeof(uint32_t)), tl = ar_align((size_t)ceil_div(n, AR_TILE) * sizeof(uint32_t));
  size_t off = 0;
  w.vals = off; off += arr;
  w.skeys = off; off += arr;
  w.svals = off; off += arr;
  for (int i = 0; i < 4; ++i) { w.tile[i] = off; off += tl; }
  w.sort = off; off += sort_u32_ws(n);
  w.total = off;
  return w;
}

// the class code of every entry: what the sort carries along with the key
__global__ __launch_bounds__(256) void auroc_class_kernel(const int32_t* __restrict__ labels, int64_t n, int positive, uint32_t* __restrict__ vals) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const int32_t l = labels[j];
    vals[j] = l < 0 ? AR_OUT : (l == positive ? AR_POS : AR_NEG);
  }
}

// a count pair in one word: negatives in the low half, positives in the high half (a tile holds at most 2048 of each)
__device__ __forceinline__ uint32_t ar_inc(uint32_t code) { return code == AR_NEG ? 1u : (code == AR_POS ? 0x10000u : 0u); }

// This thread's 8 entries of tile blockIdx.x: their packed increments, which of them start a run of equal keys (bit e of heads),
// and `excl`, the packed counts of the tile's entries before them.
struct ArLocal { uint32_t inc[AR_PER]; unsigned heads; uint32_t excl; uint32_t total; };
__device__ __forceinline__ ArLocal ar_local(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t n, uint32_t* wsum) {
  ArLocal L;
  const int64_t j0 = (int64_t)blockIdx.x * AR_TILE + (int64_t)threadIdx.x * AR_PER;
  uint32_t prev = (j0 > 0 && j0 < n) ? keys[j0 - 1] : 0u;
  L.heads = 0;
  uint32_t cnt = 0;
#pragma unroll
  for (int e = 0; e < AR_PER; ++e) {
    const int64_t j = j0 + e;
    L.inc[e] = 0;
    if (j < n) {
      const uint32_t k = keys[j];
      if (j == 0 || k != prev) L.heads |= 1u << e;
      prev = k;
      L.inc[e] = ar_inc(vals[j]);
    }
    cnt += L.inc[e];
  }
  const uint32_t incl = block_scan_incl(cnt, wsum, &L.total);
  L.excl = incl - cnt;
  return L;
}

// tile sums: the tile's packed counts, and 1 + the packed counts before its LAST run head (0: no run starts in this tile)
__global__ __launch_bounds__(256) void auroc_tile_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t n,
                                                          uint32_t* __restrict__ tile_n, uint32_t* __restrict__ tile_p,
                                                          uint32_t* __restrict__ tile_h) {
  __shared__ uint32_t wsum[4];
  const ArLocal L = ar_local(keys, vals, n, wsum);
  uint32_t run = L.excl, hv = 0;
#pragma unroll
  for (int e = 0; e < AR_PER; ++e) {
    if (L.heads >> e & 1u) hv = run + 1;
    run += L.inc[e];
  }
  uint32_t hmax;
  block_scan_incl_max(hv, wsum, &hmax);               // later heads have no smaller counts: in both halves, so as packed words too
  if (threadIdx.x == 0) {
    tile_n[blockIdx.x] = L.total & 0xffffu;
    tile_p[blockIdx.x] = L.total >> 16;
    tile_h[blockIdx.x] = hmax;
  }
}

// x of the thread before (0 for thread 0); buf is 256 words of LDS
__device__ __forceinline__ uint32_t ar_prev_thread(uint32_t x, uint32_t* buf) {
  __syncthreads();
  buf[threadIdx.x] = x;
  __syncthreads();
  return threadIdx.x ? buf[threadIdx.x - 1] : 0u;
}

// scan of the sums, one workgroup, 256 tiles per round with a carry: tile_n / tile_p become the counts of negatives / positives
// before the tile, tile_h / tile_g the counts of negatives / positives before the last run head of the EARLIER tiles (what an
// entry whose run started before its tile needs).  out = (0, P, N).
__global__ __launch_bounds__(256) void auroc_scan_kernel(uint32_t* __restrict__ tile_n, uint32_t* __restrict__ tile_p, uint32_t* __restrict__ tile_h,
                                                          uint32_t* __restrict__ tile_g, int64_t ntiles, int64_t* __restrict__ out) {
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t buf[256];
  const int tid = threadIdx.x;
  uint32_t carry_n = 0, carry_p = 0, carry_hn = 0, carry_hp = 0;      // the head carries hold 1 + count (0: none yet)
  for (int64_t t0 = 0; t0 < ntiles; t0 += 256) {
    const int64_t t = t0 + tid;
    const bool in = t < ntiles;
    const uint32_t xn = in ? tile_n[t] : 0u, xp = in ? tile_p[t] : 0u, h = in ? tile_h[t] : 0u;
    uint32_t tot_n, tot_p, tot_hn, tot_hp;
    const uint32_t pn = carry_n + block_scan_incl(xn, wsum, &tot_n) - xn;
    const uint32_t pp = carry_p + block_scan_incl(xp, wsum, &tot_p) - xp;
    const uint32_t hn = h ? pn + ((h - 1) & 0xffffu) + 1 : 0u, hp = h ? pp + ((h - 1) >> 16) + 1 : 0u;
    uint32_t en = block_scan_incl_max(ar_prev_thread(hn, buf), wsum, &tot_hn);      // over the earlier tiles of this round
    uint32_t ep = block_scan_incl_max(ar_prev_thread(hp, buf), wsum, &tot_hp);
    en = en > carry_hn ? en : carry_hn;
    ep = ep > carry_hp ? ep : carry_hp;
    if (in) {
      tile_n[t] = pn;
      tile_p[t] = pp;
      tile_h[t] = en ? en - 1 : 0u;                    // tile 0 has no earlier head and never asks: its entry 0 starts a run
      tile_g[t] = ep ? ep - 1 : 0u;
    }
    // the round's last thread holds the round's greatest head values (tot_* leave its own out)
    __syncthreads();
    if (tid == 255) { buf[0] = hn > en ? hn : en; buf[1] = hp > ep ? hp : ep; }
    __syncthreads();
    carry_hn = buf[0];
    carry_hp = buf[1];
    carry_n += tot_n;
    carry_p += tot_p;
  }
  if (tid == 0) {
    out[0] = 0;
    out[1] = (int64_t)carry_p;
    out[2] = (int64_t)carry_n;
  }
}

// apply: every counted entry's term, summed per workgroup, one integer atomic into out[0]
__global__ __launch_bounds__(256) void auroc_apply_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t n,
                                                           const uint32_t* __restrict__ tile_n, const uint32_t* __restrict__ tile_p,
                                                           const uint32_t* __restrict__ tile_h, const uint32_t* __restrict__ tile_g,
                                                           int64_t* __restrict__ out) {
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t buf[256];
  __shared__ u64 wacc[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ArLocal L = ar_local(keys, vals, n, wsum);
  uint32_t run = L.excl, hv = 0;
#pragma unroll
  for (int e = 0; e < AR_PER; ++e) {
    if (L.heads >> e & 1u) hv = run + 1;
    run += L.inc[e];
  }
  uint32_t unused;
  uint32_t cur = block_scan_incl_max(ar_prev_thread(hv, buf), wsum, &unused);      // 1 + packed counts at the last head of the earlier threads
  const u64 base_n = tile_n[blockIdx.x], base_p = tile_p[blockIdx.x], in_n = tile_h[blockIdx.x], in_p = tile_g[blockIdx.x];
  const u64 P = (u64)out[1];
  u64 acc = 0;
  run = L.excl;
#pragma unroll
  for (int e = 0; e < AR_PER; ++e) {
    if (L.heads >> e & 1u) cur = run + 1;
    const uint32_t inc = L.inc[e];
    if (inc) {
      const u64 np = cur ? base_n + ((cur - 1) & 0xffffu) : in_n, pp = cur ? base_p + ((cur - 1) >> 16) : in_p;
      acc += inc == 1u ? P - pp : np;                  // a negative: the positives at or above its run; a positive: the negatives below
    }
    run += inc;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) wacc[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    const u64 s = wacc[0] + wacc[1] + wacc[2] + wacc[3];
    if (s) atomicAdd(reinterpret_cast<u64*>(out), s);
  }
}

bool ar_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" size_t meant_auroc_ws(int64_t n) {
  if (n <= 0 || n >= (1ll << 31)) return 0;
  return ar_layout(n).total;
}

extern "C" int meant_auroc_rank(const uint32_t* keys, const int32_t* labels, int64_t n, int positive, int64_t* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
  MEANT_REQUIRE(out && n >= 0 && (n == 0 || (keys && labels)), MEANT_ERR_ARG, "auroc_rank: bad argument (null keys / labels / out or n=%lld < 0)",
                (long long)n);
  MEANT_REQUIRE(ar_aligned(keys, 4) && ar_aligned(labels, 4) && ar_aligned(out, 8) && ar_aligned(workspace, 16), MEANT_ERR_ARG,
                "auroc_rank: keys / labels / out must be aligned to their element size, the workspace to 16 bytes");
  MEANT_REQUIRE(n < (1ll << 31), MEANT_ERR_UNSUPPORTED, "auroc_rank: n=%lld must be below 2^31", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    const hipError_t e = hipMemsetAsync(out, 0, 3 * sizeof(int64_t), st);
    MEANT_REQUIRE(e == hipSuccess, MEANT_ERR_LAUNCH, "auroc_rank: clearing out failed: %s", hipGetErrorString(e));
    return MEANT_OK;
  }
  const AurocWs w = ar_layout(n);
  MEANT_REQUIRE(workspace && workspace_bytes >= w.total, MEANT_ERR_WORKSPACE, "auroc_rank: workspace of %zu bytes needed, %zu given", w.total,
                workspace_bytes);
  char* base = (char*)workspace;
  uint32_t *vals = (uint32_t*)(base + w.vals), *skeys = (uint32_t*)(base + w.skeys), *svals = (uint32_t*)(base + w.svals);
  uint32_t* tl[4];
  for (int i = 0; i < 4; ++i) tl[i] = (uint32_t*)(base + w.tile[i]);
  const int64_t ntiles = ceil_div(n, AR_TILE);
  const int64_t cg = ceil_div(n, 256);
  hipLaunchKernelGGL(auroc_class_kernel, dim3((unsigned)(cg < 4096 ? cg : 4096)), dim3(256), 0, st, labels, n, positive, vals);
  const int rc = sort_u32_launch(keys, vals, n, skeys, svals, base + w.sort, w.total - w.sort, st);
  if (rc != MEANT_OK) return rc;
  hipLaunchKernelGGL(auroc_tile_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, (const uint32_t*)skeys, (const uint32_t*)svals, n, tl[0], tl[1],
                     tl[2]);
  hipLaunchKernelGGL(auroc_scan_kernel, dim3(1), dim3(256), 0, st, tl[0], tl[1], tl[2], tl[3], ntiles, out);
  hipLaunchKernelGGL(auroc_apply_kernel, dim3((unsigned)ntiles), dim3(256), 0, st, (const uint32_t*)skeys, (const uint32_t*)svals, n,
                     (const uint32_t*)tl[0], (const uint32_t*)tl[1], (const uint32_t*)tl[2], (const uint32_t*)tl[3], out);
  MEANT_LAUNCH_CHECK("auroc_rank");
  meant_route_hit(ROUTE_AUROC_RANK);
  return MEANT_OK;
}
