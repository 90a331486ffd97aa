// The crossing-run passes of the segmented sums over sorted ids (embedding.hip: meant_embedding_bwd_seg; qkv_by_id.hip: the per-id sum
// of dqkv).  The first pass of either -- a wave per stretch of SEG sorted entries -- leaves fp32 partial sums of the runs that cross
// its stretch's ends in part[stretch][0] (the run came in from the left) and [stretch][1] (it starts here and leaves to the right);
// the two kernels here add each such run's partials in an order that depends on the sorted ids alone and hand the sum to a Store:
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
