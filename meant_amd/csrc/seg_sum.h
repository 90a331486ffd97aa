// The segmented sums over sorted ids (embedding.hip: meant_embedding_bwd_sorted[_range], meant_embedding_bwd_seg; qkv_by_id.hip: the
// per-id sum of dqkv).  Two parts.
//   seg_walk           the first pass, one definition for the three kernels: a wave walks a stretch of SEG sorted entries and sums
//                      each run of equal ids in registers.  What differs between the kernels is compile-time policy: which rows'
//                      chunks may be read (SegAllRows, or the q|k|v kernel's live-block test), where a finished sum goes (a Sink),
//                      and whether the stretch's column sums are kept.
//   seg_cross_kernel,  the crossing-run passes behind SegSlotSink: the walk leaves fp32 partial sums of the runs that cross its
//   seg_long_kernel    stretch's ends in part[stretch][0] (the run came in from the left) and [stretch][1] (it starts here and leaves
//                      to the right); the two kernels add each such run's partials in an order that depends on the sorted ids alone.
// A finished sum goes to a Store:
//   SegAddRow     dtable[id, :] += sum, for the ids of [id_lo, id_hi)
//   SegStoreHiLo  the sum as two bf16 images, hi = bf16(sum), lo = bf16(sum - hi)
// Included inside each translation unit's anonymous namespace.
#pragma once

constexpr int SEG = 256;
constexpr int SEG_SHORT = 16;

struct SegAddRow {
  float* dtable; int64_t id_lo, id_hi;
  __device__ __forceinline__ bool owns(int64_t id) const { return id >= id_lo && id < id_hi; }
  __device__ __forceinline__ void put(int64_t id, int64_t ld, int64_t col, f32x4 a) const {
    f32x4* dst = reinterpret_cast<f32x4*>(dtable + id * ld + col);
    *dst = *dst + a;
  }
};
struct SegStoreHiLo {
  bf16* hi; bf16* lo;
  __device__ __forceinline__ bool owns(int64_t) const { return true; }
  __device__ __forceinline__ void put(int64_t id, int64_t ld, int64_t col, f32x4 a) const {
    bf16x4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      h[e] = (bf16)a[e];
      l[e] = (bf16)(a[e] - (float)h[e]);
    }
    *reinterpret_cast<bf16x4*>(hi + id * ld + col) = h;
    *reinterpret_cast<bf16x4*>(lo + id * ld + col) = l;
  }
};

// ------------------------------------------------------------------------------------------------
// The walk's policies.
// Rows: may the lane's chunk c (0 or 1) of row `ord` be read?  A chunk that may not counts as zeros.
struct SegAllRows {
  __device__ __forceinline__ bool live(int64_t) const { return true; }
  __device__ __forceinline__ bool reads(int, bool) const { return true; }
};
// Sink: inside() takes the sum of a run that lies inside the stretch and so belongs to nobody else, cross() the partial sum of a run
// that came in from the left (slot 0) or starts here and leaves to the right (slot 1); owns() is the id range in front of both.
// SegSlotSink: the finished run goes to the Store, the partial sums to this stretch's two workspace rows.
template <class Store>
struct SegSlotSink {
  Store st; float* part; int64_t ld;                                       // part: [2][ld], this stretch's
  __device__ __forceinline__ bool owns(int64_t id) const { return st.owns(id); }
  __device__ __forceinline__ void inside(int64_t id, int64_t col, f32x4 lo, f32x4 hi) const {
    st.put(id, ld, col, lo);
    st.put(id, ld, col + 4, hi);
  }
  __device__ __forceinline__ void cross(int64_t, int slot, int64_t col, f32x4 lo, f32x4 hi) const {
    store8<float>(part + slot * ld + col, Vec8<float>{lo, hi});
  }
};

// the lane's two 8-column chunks, `lane` and `lane + 64` of column block blockIdx.y (cb_chunks chunks to a block, seg_col_blocks), and
// the block's first column
struct SegCols { int64_t col[2]; bool has[2]; int64_t first; };
__device__ __forceinline__ SegCols seg_cols(int64_t width, int cb_chunks) {
  const int lane = threadIdx.x & 63;
  const int c0 = blockIdx.y * cb_chunks;                                   // this column block: chunks [c0, c0 + nch)
  const int left = (int)(width >> 3) - c0;
  const int nch = left < cb_chunks ? left : cb_chunks;
  return {{(int64_t)(c0 + lane) * 8, (int64_t)(c0 + lane + 64) * 8}, {lane < nch, lane + 64 < nch}, (int64_t)c0 * 8};
}

// a 64-bit value that is the same in every lane of the wave, and lane t (the same t in every lane) of a per-lane one: through the scalar
// unit, so that what hangs on them (row bases, the loop's own counters) is scalar too
__device__ __forceinline__ long long seg_uniform64(long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long seg_lane64(long long v, int t) {
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, t), hi = __builtin_amdgcn_readlane((int)(v >> 32), t);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// 64 sorted entries, one per lane: the id, the row, and the row's flags (SEG_ROW_OK: the row number is one of src; SEG_ROW_LIVE:
// the rows policy's flag for it)
struct SegBlock { long long id, ord; int flags; };
constexpr int SEG_ROW_OK = 1, SEG_ROW_LIVE = 2;
// four rows on their way: the lane's two chunks of each, whether a chunk counts (or is zeros), and the rows' ids
template <typename T>
struct SegSet { Vec8<T> r[4][2]; bool on[4][2]; long long id[4]; };

// One wave sums the rows src[order[j], :] of the sorted entries j of [j0, j1), run by run of equal ids.  Ids, row numbers and row flags
// are loaded 64 entries at a time, a block ahead, and broadcast from the lanes that loaded them.  The rows (16-byte loads) travel in
// two register sets of four: while one set is added, the other is on its way, and the set after it is requested before the second is
// touched, across the 64-entry blocks too, so four to eight rows are in flight at any time.  A run's rows are added in sorted order
// into one accumulator per column: every bit-reproducibility promise rests on that order.  A run is flushed when the id changes and at
// the end; ids outside [0, V) and outside the sink's range are dropped there.  A run that is open on both sides counts as "from the
// left".  With COLSUM, csum[col] = the sum of every row of the stretch, whatever its id.
template <bool COLSUM, typename T, class Rows, class Sink>
__device__ __forceinline__ void seg_walk(const T* __restrict__ src, int64_t ld, const int64_t* __restrict__ sorted_ids,
                                         const int64_t* __restrict__ order, int64_t n, int64_t V, int64_t j0_, int64_t j1_, const SegCols& c,
                                         const Rows& rows, const Sink& sink, float* __restrict__ csum) {
  const int lane = threadIdx.x & 63;
  const int64_t j0 = seg_uniform64(j0_), j1 = seg_uniform64(j1_);         // a wave's stretch: the same in every lane
  float acc[2][8], cs[2][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[0][e] = acc[1][e] = cs[0][e] = cs[1][e] = 0.f;
  int64_t cur = sorted_ids[j0];
  bool open_left = j0 > 0 && sorted_ids[j0 - 1] == cur;                  // the first run started in an earlier stretch

  // slot < 0: the run is this wave's alone
  auto flush = [&](int64_t id, int slot) {
    if (id < 0 || id >= V || !sink.owns(id)) return;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!c.has[k]) continue;
      const f32x4 lo = {acc[k][0], acc[k][1], acc[k][2], acc[k][3]}, hi = {acc[k][4], acc[k][5], acc[k][6], acc[k][7]};
      if (slot < 0) sink.inside(id, c.col[k], lo, hi);
      else sink.cross(id, slot, c.col[k], lo, hi);
    }
  };

  // the entries jb + lane of a block (past the end: the last entry again), and their flags once the row numbers have arrived
  auto entries = [&](int64_t jb) {
    const int64_t jl = jb + lane < j1 ? jb + lane : j1 - 1;
    return SegBlock{sorted_ids[jl], order[jl], 0};
  };
  auto flags = [&](const SegBlock& b) {
    const bool row_ok = b.ord >= 0 && b.ord < n;        // an order that is no permutation must not become an address
    return !row_ok ? 0 : (rows.live(b.ord) ? SEG_ROW_OK | SEG_ROW_LIVE : SEG_ROW_OK);
  };
  // The four rows of the block's entries [t0, t0 + 4); those past cnt repeat the last one and are not added.  Every lane loads
  // every time -- a chunk that is not to be read (no such chunk, no such row, a dead row) reads the block's first chunk of row 0
  // and counts as zeros (SegSet::on) -- so that the number of loads behind a set is known when the set is waited for: the memory
  // counter retires in order, and a load that may or may not have been issued would turn every wait into a wait for everything.
  auto request = [&](const SegBlock& b, int t0, int cnt, SegSet<T>& g) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = t0 + u < cnt ? t0 + u : cnt - 1;
      g.id[u] = seg_lane64(b.id, t);
      const long long ord = seg_lane64(b.ord, t);
      const int fl = __builtin_amdgcn_readlane(b.flags, t);
      const bool row_ok = (fl & SEG_ROW_OK) != 0, live = (fl & SEG_ROW_LIVE) != 0;
      const T* row = src + (row_ok ? ord : 0) * ld;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        g.on[u][k] = row_ok && rows.reads(k, live);
        g.r[u][k] = load8s<T>(c.has[k] && g.on[u][k] ? row + c.col[k] : src + c.first);
      }
    }
  };
  auto add = [&](int t0, int cnt, const SegSet<T>& g) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (t0 + u >= cnt) break;
      const int64_t id = g.id[u];
      if (id != cur) {
        flush(cur, open_left ? 0 : -1);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[0][e] = acc[1][e] = 0.f;
        cur = id;
        open_left = false;
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const Vec8<T> v = g.on[u][k] ? g.r[u][k] : Vec8<T>{};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float a = v.get(e);
          acc[k][e] += a;
          if constexpr (COLSUM) cs[k][e] += a;
        }
      }
    }
  };

  SegSet<T> ga, gb;
  SegBlock blk = entries(j0), nxt = entries(j0 + 64);
  blk.flags = flags(blk);
  request(blk, 0, (int)(j1 - j0 < 64 ? j1 - j0 : 64), ga);
  for (int64_t jb = j0; jb < j1; jb += 64) {
    const int cnt = (int)(j1 - jb < 64 ? j1 - jb : 64);
    const int ncnt = jb + 64 < j1 ? (int)(j1 - jb - 64 < 64 ? j1 - jb - 64 : 64) : 1;      // past the end: the last entry, not added
    const SegBlock after = entries(jb + 128);
    nxt.flags = flags(nxt);
    for (int t0 = 0; t0 < cnt; t0 += 8) {
      request(blk, t0 + 4, cnt, gb);
      add(t0, cnt, ga);
      const bool last = t0 + 8 >= cnt;                 // the set after the second one opens the next block
      const SegBlock from{last ? nxt.id : blk.id, last ? nxt.ord : blk.ord, last ? nxt.flags : blk.flags};
      request(from, last ? 0 : t0 + 8, last ? ncnt : cnt, ga);
      add(t0 + 4, cnt, gb);
    }
    blk = nxt;
    nxt = after;
  }
  const bool open_right = j1 < n && sorted_ids[j1] == cur;
  flush(cur, open_left ? 0 : (open_right ? 1 : -1));
  if constexpr (COLSUM) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (c.has[k])
        store8<float>(csum + c.col[k], Vec8<float>{{cs[k][0], cs[k][1], cs[k][2], cs[k][3]}, {cs[k][4], cs[k][5], cs[k][6], cs[k][7]}});
  }
}

// ------------------------------------------------------------------------------------------------
// The runs that cross stretch ends.  A run belongs to the stretch it STARTS in: its partial sums are slot 1 of that stretch and
// slot 0 of every following stretch that begins with the same id (sorted ids: a contiguous range).
// Short lists (at most SEG_SHORT partials; two for a typical id): one wave per (stretch, 256 columns) adds them in stretch order and
// hands the sum to the store.  It also leaves the list's length in longk[stretch] where the list is longer (0 otherwise), for
// the kernel below.
template <class Store>
__global__ __launch_bounds__(256) void seg_cross_kernel(const int64_t* __restrict__ sorted_ids, const float* __restrict__ part,
                                                         int* __restrict__ longk, Store st, int64_t n, int64_t d, int64_t V) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t s = (int64_t)blockIdx.x * 4 + wave, j0 = s * SEG, j1 = j0 + SEG;
  if (j1 >= n) return;                                                    // the last stretch has nothing to its right (and no longk slot)
  const int64_t id = sorted_ids[j1 - 1];
  const bool owner = sorted_ids[j1] == id && !(j0 > 0 && sorted_ids[j0 - 1] == id)      // leaves to the right, did not come in from the left
                     && id >= 0 && id < V && st.owns(id);
  int64_t K = 0;
  if (owner) {                                                            // wave-uniform
    const int64_t nst = (n + SEG - 1) / SEG;
    int64_t follow = 0;
    for (int64_t t0 = s + 1;; t0 += 64) {
      const int64_t t = t0 + lane;
      const int k = __popcll(__ballot(t < nst && sorted_ids[t * SEG] == id));
      follow += k;
      if (k < 64) break;
    }
    K = follow + 1;
  }
  if (blockIdx.y == 0 && lane == 0) longk[s] = K > SEG_SHORT ? (int)K : 0;
  if (K == 0 || K > SEG_SHORT) return;
  const int64_t col = (int64_t)blockIdx.y * 256 + lane * 4;
  if (col >= d) return;
  f32x4 acc = *reinterpret_cast<const f32x4*>(part + (s * 2 + 1) * d + col);
  for (int64_t k = 1; k < K; ++k) acc += *reinterpret_cast<const f32x4*>(part + (s + k) * 2 * d + col);
  st.put(id, d, col, acc);
}

// Long lists (a padding id: one partial per stretch it covers).  One workgroup per (stretch, 64 columns), at work only where
// longk says so.  The list is cut into 16 equal pieces (a cut that depends on its length alone), 16 threads with 4 columns each sum
// a piece in order, and the 16 pieces are added as a fixed binary tree: the sum depends on the sorted ids and the rows, on nothing else.
template <class Store>
__global__ __launch_bounds__(256) void seg_long_kernel(const int64_t* __restrict__ sorted_ids, const float* __restrict__ part,
                                                        const int* __restrict__ longk, Store st, int64_t d) {
  __shared__ f32x4 red[16][16];
  const int tid = threadIdx.x;
  const int64_t s = blockIdx.x;
  const int64_t K = longk[s];
  if (K == 0) return;                                                     // uniform over the workgroup
  const int64_t id = sorted_ids[s * SEG + SEG - 1];                       // in range: seg_cross_kernel checked it
  const int p = tid >> 4;
  const int64_t col = (int64_t)blockIdx.y * 64 + (tid & 15) * 4;
  const bool active = col < d;
  const int64_t piece = (K + 15) / 16, k0 = p * piece, k1 = k0 + piece < K ? k0 + piece : K;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (active) {
#pragma unroll 4
    for (int64_t k = k0; k < k1; ++k) {
      const float* row = k == 0 ? part + (s * 2 + 1) * d : part + (s + k) * 2 * d;
      acc += *reinterpret_cast<const f32x4*>(row + col);
    }
  }
  red[p][tid & 15] = acc;
  __syncthreads();
#pragma unroll
  for (int h = 8; h > 0; h >>= 1) {
    if (p < h) red[p][tid & 15] += red[p + h][tid & 15];
    __syncthreads();
  }
  if (p == 0 && active) st.put(id, d, col, red[0][tid & 15]);
}

// ------------------------------------------------------------------------------------------------
// host side
// the cut of a row of `width` columns into grid.y column blocks of at most 64 * per_lane 8-column chunks, as equal as they come
struct SegColBlocks { int ncb, cb_chunks; };
inline SegColBlocks seg_col_blocks(int64_t width, int per_lane) {
  const int64_t chunks = width >> 3, ncb = ceil_div(chunks, 64 * per_lane);
  return {(int)ncb, (int)ceil_div(chunks, ncb)};
}

// the two crossing-run passes over the partial sums a SegSlotSink<Store> walk left; longk: one int per stretch
template <class Store>
void seg_cross_launch(const Store& store, const int64_t* sorted_ids, const float* part, int* longk, int64_t n, int64_t d, int64_t V,
                      hipStream_t st) {
  const int64_t nst = ceil_div(n, SEG);
  if (nst <= 1) return;
  hipLaunchKernelGGL(seg_cross_kernel<Store>, dim3((unsigned)ceil_div(nst - 1, 4), (unsigned)ceil_div(d, 256)), dim3(256), 0, st, sorted_ids,
                     part, longk, store, n, d, V);
  hipLaunchKernelGGL(seg_long_kernel<Store>, dim3((unsigned)(nst - 1), (unsigned)ceil_div(d, 64)), dim3(256), 0, st, sorted_ids, part,
                     (const int*)longk, store, d);
}
