// Pretraining collators on the device (utils/custom_datasets.py:41-57 mlm_dataset.mask_tokens, :116-126 mim_dataset.mask_image;
// pretrain_mim.py:198-204, pretrain_mlm.py:160): what the reference builds per sample on the host -- one Bernoulli per token or per
// pixel element, the masked input and a label tensor with -100 outside the mask -- is a pure function of (seed, dataset index,
// position), so nothing of it has to be stored or sent:
//   * meant_mlm_mask            -- ids -> (masked ids, labels), one launch
//   * meant_patchify_raw_masked -- meant_patchify_raw with the mask applied on load (no masked image is written anywhere)
//   * meant_mim_l1_fwd / _bwd   -- L1Loss of the decoder's NCHW output against labels regenerated per element from the raw image
// The rule, in integers (restated in tests/collate_ref.py): fin = the finaliser of hash_uniform (common.h),
//   bits(seed, stream, idx)  = fin(seed + (idx | (uint64)stream << 60) * 0x9E3779B97F4A7C15)
//   draw24(seed, stream, idx) = bits >> 40
//   idx = sample_id * E + e      E = elements per sample (S tokens, or C * Hh * Ww), e = position in the sample's own storage order
// element e of sample sample_id is CHOSEN iff draw24(seed, 0, idx) < threshold, threshold = floor(p * 2^24) computed by the host in
// double: the device compares integers only.  idx is keyed by the dataset index, so a sample's mask does not depend on the batch
// it arrives in, its place in it, or the number of ranks.  sample_id * E + e must stay below 2^60 (the stream tag's bits): checked
// on the host against the caller's bound on the ids.
// Determinism: no atomics anywhere.  The loss is a two-stage ordered sum: a workgroup owns L1_SPAN consecutive elements and leaves
// one float partial and one count, a second launch of one workgroup adds them in an order fixed by N (in double).
#include "common.h"

namespace {

constexpr int CL_THREADS = 256;
constexpr int L1_PER_THREAD = 16;
constexpr int L1_SPAN = CL_THREADS * L1_PER_THREAD;    // elements per workgroup = per partial
constexpr uint64_t CL_GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr int64_t CL_IDX_LIMIT = 1ll << 60;

__device__ __forceinline__ uint64_t cl_bits(uint64_t seed, uint64_t stream, uint64_t idx) {
  uint64_t z = seed + (idx | (stream << 60)) * CL_GOLDEN;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t cl_draw24(uint64_t seed, uint64_t stream, uint64_t idx) { return (uint32_t)(cl_bits(seed, stream, idx) >> 40); }

__device__ __forceinline__ float cl_raw(double v) { return (float)v; }
__device__ __forceinline__ float cl_raw(float v) { return v; }
__device__ __forceinline__ float cl_raw(bf16 v) { return (float)v; }
__device__ __forceinline__ float cl_raw(unsigned char v) { return (float)v; }

__device__ __forceinline__ bool cl_live(float v) { return v != 0.f; }
__device__ __forceinline__ bool cl_live(bf16 v) { return (float)v != 0.f; }
__device__ __forceinline__ bool cl_live(int64_t v) { return v != 0; }
__device__ __forceinline__ bool cl_live(int32_t v) { return v != 0; }
__device__ __forceinline__ bool cl_live(unsigned char v) { return v != 0; }

struct MlmArgs {
  const int64_t* ids;
  const int64_t* sample_ids;
  const int64_t* special_ids;
  int64_t* ids_out;
  int64_t* labels;
  int64_t sample_base, T, S, mask_id, V, ignore_index;
  uint64_t seed;
  uint32_t threshold, t_replace, t_both;               // t_both = t_replace + t_random (up to 2^25)
  int n_special;
};

// one thread per token.  ids and ids_out may be the same buffer: a thread reads its own id before it writes it, nobody else's.
template <typename TM>
__global__ __launch_bounds__(CL_THREADS) void mlm_mask_kernel(MlmArgs a, const TM* __restrict__ attention_mask) {
  const int64_t i = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
  if (i >= a.T) return;
  const int64_t row = i / a.S;
  const int64_t s = i - row * a.S;
  const int64_t id = a.ids[i];
  bool open = attention_mask ? cl_live(attention_mask[i]) : true;
  for (int k = 0; k < a.n_special; ++k) open = open && id != a.special_ids[k];
  const uint64_t sid = (uint64_t)(a.sample_ids ? a.sample_ids[row] : a.sample_base + row);
  const uint64_t idx = sid * (uint64_t)a.S + (uint64_t)s;
  const bool chosen = open && cl_draw24(a.seed, 0, idx) < a.threshold;
  int64_t o = id;
  if (chosen) {
    const uint32_t r = cl_draw24(a.seed, 1, idx);
    if (r < a.t_replace) o = a.mask_id;
    else if (r < a.t_both) o = (int64_t)(cl_bits(a.seed, 2, idx) % (uint64_t)a.V);
  }
  a.ids_out[i] = o;
  a.labels[i] = chosen ? id : a.ignore_index;
}

// meant_patchify_raw's kernel (elementwise.hip) with the rule on load: one thread = one pixel position of a patch row, C channel
// values in, C consecutive outputs.  The draw is keyed by the element's (c, y, x) place in the RAW image, not by its place in the row.
template <typename TI, typename T>
__global__ __launch_bounds__(CL_THREADS) void patchify_raw_masked_kernel(const TI* __restrict__ img, T* __restrict__ out, int64_t G, int C, int Hh,
                                                                          int Ww, int p, float mean, float inv_std, uint64_t seed,
                                                                          uint32_t threshold, const int64_t* __restrict__ sample_ids,
                                                                          int64_t sample_base, float mask_value) {
  const int nph = Hh / p, npw = Ww / p;
  const int64_t HW = (int64_t)Hh * Ww;
  const int64_t total = G * HW;                        // pixel positions, ordered (g, ph, pw, p1, p2) = output order / C
  const T fill = from_f<T>(mask_value);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i / (p * p);
    const int e = (int)(i - r * (p * p));
    const int p2 = e % p, p1 = e / p;
    const int pw = (int)(r % npw); r /= npw;
    const int ph = (int)(r % nph);
    const int64_t g = r / nph;
    const int64_t pix = (int64_t)(ph * p + p1) * Ww + pw * p + p2;
    const uint64_t sid = (uint64_t)(sample_ids ? sample_ids[g] : sample_base + g);
    const uint64_t idx0 = sid * (uint64_t)(C * HW) + (uint64_t)pix;
    T* o = out + i * C;
    for (int c = 0; c < C; ++c) {
      const T v = from_f<T>((cl_raw(img[(g * C + c) * HW + pix]) - mean) * inv_std);
      o[c] = cl_draw24(seed, 0, idx0 + (uint64_t)c * (uint64_t)HW) < threshold ? fill : v;
    }
  }
}

struct L1Args {
  const int64_t* sample_ids;
  int64_t sample_base;
  int64_t N;                                           // B * Co * Hh * Ww
  int64_t span;                                        // Co * Hh * Ww: out elements per sample = the first `span` of the sample's E
  int64_t E;                                           // C * Hh * Ww
  uint64_t seed;
  uint32_t threshold;
  float mean, inv_std, unmasked_label;
  int on_masked;
};

// element i of out = (b, j) with j < span; the label's source is element j of sample b's raw image (the first Co planes are the
// first span elements of the sample).  One 64-bit division per thread, then steps of CL_THREADS with a carry into b.
struct L1Pos { int64_t b, j; };
__device__ __forceinline__ L1Pos l1_start(int64_t i, int64_t span) {
  L1Pos q; q.b = i / span; q.j = i - q.b * span; return q;
}
__device__ __forceinline__ void l1_step(L1Pos& q, int64_t span) {
  q.j += CL_THREADS;
  while (q.j >= span) { q.j -= span; ++q.b; }
}
// label of element (b, j), and whether it is chosen
template <typename TI>
__device__ __forceinline__ float l1_label(const L1Args& a, const TI* __restrict__ img, const L1Pos& q, bool& chosen) {
  const uint64_t sid = (uint64_t)(a.sample_ids ? a.sample_ids[q.b] : a.sample_base + q.b);
  chosen = cl_draw24(a.seed, 0, sid * (uint64_t)a.E + (uint64_t)q.j) < a.threshold;
  const float x = (cl_raw(img[q.b * a.E + q.j]) - a.mean) * a.inv_std;
  return chosen ? x : a.unmasked_label;
}

template <typename TI, typename T>
__global__ __launch_bounds__(CL_THREADS) void mim_l1_fwd_kernel(L1Args a, const T* __restrict__ out, const TI* __restrict__ img,
                                                                 float* __restrict__ part_sum, uint32_t* __restrict__ part_cnt) {
  __shared__ float wsum[CL_THREADS / 64];
  __shared__ uint32_t wcnt[CL_THREADS / 64];
  const int64_t i0 = (int64_t)blockIdx.x * L1_SPAN + threadIdx.x;
  float acc = 0.f;
  uint32_t cnt = 0;
  if (i0 < a.N) {
    L1Pos q = l1_start(i0, a.span);
#pragma unroll 4
    for (int k = 0; k < L1_PER_THREAD; ++k) {
      const int64_t i = i0 + (int64_t)k * CL_THREADS;
      if (i >= a.N) break;
      bool chosen;
      const float label = l1_label<TI>(a, img, q, chosen);
      const float d = fabsf(to_f(out[i]) - label);
      acc += (!a.on_masked || chosen) ? d : 0.f;
      cnt += chosen ? 1u : 0u;
      l1_step(q, a.span);
    }
  }
  acc = wave_sum(acc);                                 // every lane of every wave gets here: the loop above has no early return
  uint32_t c = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { wsum[wave] = acc; wcnt[wave] = c; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part_sum[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    part_cnt[blockIdx.x] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
  }
}

// loss[0] = sum / divisor, count[0] = chosen elements: one workgroup, thread t adds partials t, t + 256, ... in double, a fixed tree
__global__ __launch_bounds__(CL_THREADS) void mim_l1_finish_kernel(const float* __restrict__ part_sum, const uint32_t* __restrict__ part_cnt,
                                                                    int64_t nparts, int64_t N, int on_masked, float* __restrict__ loss,
                                                                    int64_t* __restrict__ count) {
  __shared__ double ps[CL_THREADS];
  __shared__ int64_t pc[CL_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  int64_t c = 0;
  for (int64_t k = tid; k < nparts; k += CL_THREADS) { s += (double)part_sum[k]; c += (int64_t)part_cnt[k]; }
  ps[tid] = s; pc[tid] = c;
  __syncthreads();
#pragma unroll
  for (int o = CL_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) { ps[tid] += ps[tid + o]; pc[tid] += pc[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t div = on_masked ? (pc[0] > 0 ? pc[0] : 1) : N;
    loss[0] = (float)(ps[0] / (double)div);
    count[0] = pc[0];
  }
}

template <typename TI, typename T>
__global__ __launch_bounds__(CL_THREADS) void mim_l1_bwd_kernel(L1Args a, const T* __restrict__ out, const TI* __restrict__ img,
                                                                 const float* __restrict__ g, const int64_t* __restrict__ count,
                                                                 T* __restrict__ dout) {
  const int64_t i0 = (int64_t)blockIdx.x * L1_SPAN + threadIdx.x;
  if (i0 >= a.N) return;
  int64_t div = a.N;
  if (a.on_masked) { div = count[0]; div = div > 0 ? div : 1; }
  const float scale = g[0] / (float)div;
  L1Pos q = l1_start(i0, a.span);
#pragma unroll 4
  for (int k = 0; k < L1_PER_THREAD; ++k) {
    const int64_t i = i0 + (int64_t)k * CL_THREADS;
    if (i >= a.N) break;
    bool chosen;
    const float label = l1_label<TI>(a, img, q, chosen);
    const float d = to_f(out[i]) - label;
    float v = d > 0.f ? scale : (d < 0.f ? -scale : 0.f);      // 0 where they are equal (and for a NaN), as L1Loss does
    if (a.on_masked && !chosen) v = 0.f;
    dout[i] = from_f<T>(v);
    l1_step(q, a.span);
  }
}

bool cl_aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
size_t cl_raw_size(int raw_dtype) { return raw_dtype == MEANT_RAW_F64 ? 8 : raw_dtype == MEANT_RAW_F32 ? 4 : raw_dtype == MEANT_RAW_BF16 ? 2 : 1; }
bool cl_raw_known(int raw_dtype) { return raw_dtype >= MEANT_RAW_F32 && raw_dtype <= MEANT_RAW_U8; }

// sample ids in [0, bound) times E elements must stay below 2^60
bool cl_idx_fits(int64_t bound, int64_t E) { return bound >= 0 && E > 0 && (bound == 0 || E <= CL_IDX_LIMIT / bound); }

// the rule's arguments shared by the three MIM entries; 0 or an error code with the message set
int l1_check(const char* who, const void* out, const void* images, int raw_dtype, const int64_t* sample_ids, int64_t sample_base, int64_t id_bound,
             int64_t B, int C, int Co, int Hh, int Ww, uint32_t threshold, int dtype) {
  MEANT_REQUIRE(out && images, MEANT_ERR_ARG, "%s: null out / images", who);
  MEANT_REQUIRE(B > 0 && C > 0 && Co > 0 && Co <= C && Hh > 0 && Ww > 0, MEANT_ERR_ARG,
                "%s: bad shape (B=%lld, C=%d, Co=%d (must be in 1..C), Hh=%d, Ww=%d)", who, (long long)B, C, Co, Hh, Ww);
  MEANT_REQUIRE(dtype == MEANT_F32 || dtype == MEANT_BF16, MEANT_ERR_ARG, "%s: unknown act dtype %d", who, dtype);
  MEANT_REQUIRE(cl_raw_known(raw_dtype), MEANT_ERR_ARG, "%s: unknown raw dtype %d", who, raw_dtype);
  MEANT_REQUIRE(threshold <= (1u << 24), MEANT_ERR_ARG, "%s: threshold %u above 2^24", who, threshold);
  MEANT_REQUIRE(cl_aligned(out, dtype == MEANT_F32 ? 4 : 2) && cl_aligned(images, cl_raw_size(raw_dtype)) && cl_aligned(sample_ids, 8), MEANT_ERR_ARG,
                "%s: operands must be aligned to their element size", who);
  const int64_t E = (int64_t)C * Hh * Ww;
  MEANT_REQUIRE(sample_base >= 0 && cl_idx_fits(sample_ids ? id_bound : sample_base + B, E), MEANT_ERR_UNSUPPORTED,
                "%s: sample id * elements per sample (%lld) must stay below 2^60", who, (long long)E);
  MEANT_REQUIRE(B <= (1ll << 40) / ((int64_t)Co * Hh * Ww), MEANT_ERR_UNSUPPORTED, "%s: more than 2^40 elements", who);
  return MEANT_OK;
}

}  // namespace

extern "C" int meant_mlm_mask(const int64_t* ids, const void* attention_mask, int mask_dtype, const int64_t* sample_ids, int64_t sample_base,
                              int64_t id_bound, const int64_t* special_ids, int n_special, int64_t B, int64_t S, uint64_t seed, uint32_t threshold,
                              uint32_t t_replace, uint32_t t_random, int64_t mask_id, int64_t V, int64_t ignore_index, int64_t* ids_out,
                              int64_t* labels, void* stream) {
  MEANT_REQUIRE(ids && ids_out && labels, MEANT_ERR_ARG, "mlm_mask: null ids / ids_out / labels");
  MEANT_REQUIRE(B > 0 && S > 0 && V > 0 && n_special >= 0 && n_special <= 16 && (n_special == 0 || special_ids), MEANT_ERR_ARG,
                "mlm_mask: bad argument (B=%lld, S=%lld, V=%lld, n_special=%d: 0..16, with a list)", (long long)B, (long long)S, (long long)V, n_special);
  MEANT_REQUIRE(threshold <= (1u << 24) && t_replace <= (1u << 24) && t_random <= (1u << 24), MEANT_ERR_ARG,
                "mlm_mask: thresholds (%u, %u, %u) are counts out of 2^24", threshold, t_replace, t_random);
  MEANT_REQUIRE(mask_dtype >= MEANT_MASK_F32 && mask_dtype <= MEANT_MASK_I32, MEANT_ERR_ARG, "mlm_mask: unknown attention mask dtype %d", mask_dtype);
  const size_t msz = mask_dtype == MEANT_MASK_I64 ? 8 : (mask_dtype == MEANT_MASK_F32 || mask_dtype == MEANT_MASK_I32) ? 4 : mask_dtype == MEANT_MASK_BF16 ? 2 : 1;
  MEANT_REQUIRE(cl_aligned(ids, 8) && cl_aligned(ids_out, 8) && cl_aligned(labels, 8) && cl_aligned(sample_ids, 8) && cl_aligned(special_ids, 8) &&
                    cl_aligned(attention_mask, msz),
                MEANT_ERR_ARG, "mlm_mask: operands must be aligned to their element size");
  MEANT_REQUIRE(B <= (1ll << 38) / S, MEANT_ERR_UNSUPPORTED, "mlm_mask: more than 2^38 tokens");
  const int64_t T = B * S;
  {
    const char *l = (const char*)labels, *i = (const char*)ids, *o = (const char*)ids_out;
    const int64_t len = T * 8;
    MEANT_REQUIRE(!(l < i + len && i < l + len) && !(l < o + len && o < l + len), MEANT_ERR_ARG, "mlm_mask: labels must not overlap ids or ids_out");
    MEANT_REQUIRE(o == i || !(o < i + len && i < o + len), MEANT_ERR_ARG, "mlm_mask: ids_out must be ids itself or not overlap it");
  }
  MEANT_REQUIRE(sample_base >= 0 && cl_idx_fits(sample_ids ? id_bound : sample_base + B, S), MEANT_ERR_UNSUPPORTED,
                "mlm_mask: sample id * S (%lld) must stay below 2^60", (long long)S);
  MlmArgs a;
  a.ids = ids; a.sample_ids = sample_ids; a.special_ids = special_ids; a.ids_out = ids_out; a.labels = labels;
  a.sample_base = sample_base; a.T = T; a.S = S; a.mask_id = mask_id; a.V = V; a.ignore_index = ignore_index;
  a.seed = seed; a.threshold = threshold; a.t_replace = t_replace; a.t_both = t_replace + t_random; a.n_special = n_special;
  const dim3 grid((unsigned)ceil_div(T, CL_THREADS)), block(CL_THREADS);
  hipStream_t st = (hipStream_t)stream;
  switch (mask_dtype) {
    case MEANT_MASK_F32: hipLaunchKernelGGL(mlm_mask_kernel<float>, grid, block, 0, st, a, (const float*)attention_mask); break;
    case MEANT_MASK_BF16: hipLaunchKernelGGL(mlm_mask_kernel<bf16>, grid, block, 0, st, a, (const bf16*)attention_mask); break;
    case MEANT_MASK_I64: hipLaunchKernelGGL(mlm_mask_kernel<int64_t>, grid, block, 0, st, a, (const int64_t*)attention_mask); break;
    case MEANT_MASK_U8: hipLaunchKernelGGL(mlm_mask_kernel<unsigned char>, grid, block, 0, st, a, (const unsigned char*)attention_mask); break;
    default: hipLaunchKernelGGL(mlm_mask_kernel<int32_t>, grid, block, 0, st, a, (const int32_t*)attention_mask); break;
  }
  MEANT_LAUNCH_CHECK("mlm_mask");
  return MEANT_OK;
}

extern "C" int meant_patchify_raw_masked(const void* images, int raw_dtype, float mean, float inv_std, void* patches, int64_t G, int C, int Hh,
                                         int Ww, int p, int dtype, uint64_t seed, uint32_t threshold, const int64_t* sample_ids,
                                         int64_t sample_base, int64_t id_bound, float mask_value, void* stream) {
  MEANT_REQUIRE(images && patches && G > 0 && C > 0 && p > 0 && Hh > 0 && Ww > 0 && Hh % p == 0 && Ww % p == 0, MEANT_ERR_ARG,
                "patchify_raw_masked: bad argument");
  MEANT_REQUIRE(dtype == MEANT_F32 || dtype == MEANT_BF16, MEANT_ERR_ARG, "patchify_raw_masked: unknown output dtype %d", dtype);
  MEANT_REQUIRE(cl_raw_known(raw_dtype), MEANT_ERR_ARG, "patchify_raw_masked: unknown raw dtype %d", raw_dtype);
  MEANT_REQUIRE(threshold <= (1u << 24), MEANT_ERR_ARG, "patchify_raw_masked: threshold %u above 2^24", threshold);
  MEANT_REQUIRE(cl_aligned(images, cl_raw_size(raw_dtype)) && cl_aligned(patches, dtype == MEANT_F32 ? 4 : 2) && cl_aligned(sample_ids, 8), MEANT_ERR_ARG,
                "patchify_raw_masked: operands must be aligned to their element size");
  const int64_t E = (int64_t)C * Hh * Ww;
  MEANT_REQUIRE(sample_base >= 0 && cl_idx_fits(sample_ids ? id_bound : sample_base + G, E), MEANT_ERR_UNSUPPORTED,
                "patchify_raw_masked: sample id * elements per sample (%lld) must stay below 2^60", (long long)E);
  MEANT_REQUIRE(G <= (1ll << 40) / E, MEANT_ERR_UNSUPPORTED, "patchify_raw_masked: more than 2^40 elements");
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = G * (int64_t)Hh * Ww;
  const dim3 grid((unsigned)(ceil_div(total, CL_THREADS) < 65535 * 16 ? ceil_div(total, CL_THREADS) : 65535 * 16)), block(CL_THREADS);
#define CL_LAUNCH(TI)                                                                                                                      \
  do {                                                                                                                                     \
    if (dtype == MEANT_F32) hipLaunchKernelGGL((patchify_raw_masked_kernel<TI, float>), grid, block, 0, st, (const TI*)images, (float*)patches, G, C, \
                                               Hh, Ww, p, mean, inv_std, seed, threshold, sample_ids, sample_base, mask_value);          \
    else hipLaunchKernelGGL((patchify_raw_masked_kernel<TI, bf16>), grid, block, 0, st, (const TI*)images, (bf16*)patches, G, C, Hh, Ww, p, mean,   \
                            inv_std, seed, threshold, sample_ids, sample_base, mask_value);                                              \
  } while (0)
  switch (raw_dtype) {
    case MEANT_RAW_F32: CL_LAUNCH(float); break;
    case MEANT_RAW_BF16: CL_LAUNCH(bf16); break;
    case MEANT_RAW_F64: CL_LAUNCH(double); break;
    default: CL_LAUNCH(unsigned char); break;
  }
#undef CL_LAUNCH
  MEANT_LAUNCH_CHECK("patchify_raw_masked");
  return MEANT_OK;
}

extern "C" size_t meant_mim_l1_ws(int64_t N) {
  if (N <= 0 || N > (1ll << 40)) return 0;
  return 2 * align256((size_t)ceil_div(N, L1_SPAN) * 4);
}

#define L1_DISPATCH(KERNEL, ...)                                                                                         \
  do {                                                                                                                   \
    switch (raw_dtype) {                                                                                                 \
      case MEANT_RAW_F32: DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((KERNEL<float, T>), grid, block, 0, st, a, (const T*)out, (const float*)images, __VA_ARGS__)); break; \
      case MEANT_RAW_BF16: DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((KERNEL<bf16, T>), grid, block, 0, st, a, (const T*)out, (const bf16*)images, __VA_ARGS__)); break;  \
      case MEANT_RAW_F64: DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((KERNEL<double, T>), grid, block, 0, st, a, (const T*)out, (const double*)images, __VA_ARGS__)); break; \
      default: DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((KERNEL<unsigned char, T>), grid, block, 0, st, a, (const T*)out, (const unsigned char*)images, __VA_ARGS__)); break; \
    }                                                                                                                    \
  } while (0)

static L1Args l1_args(const int64_t* sample_ids, int64_t sample_base, int64_t B, int C, int Co, int Hh, int Ww, uint64_t seed, uint32_t threshold,
                      float mean, float inv_std, float unmasked_label, int on_masked) {
  L1Args a;
  a.sample_ids = sample_ids; a.sample_base = sample_base;
  a.span = (int64_t)Co * Hh * Ww; a.E = (int64_t)C * Hh * Ww; a.N = B * a.span;
  a.seed = seed; a.threshold = threshold; a.mean = mean; a.inv_std = inv_std; a.unmasked_label = unmasked_label; a.on_masked = on_masked ? 1 : 0;
  return a;
}

extern "C" int meant_mim_l1_fwd(const void* out, int dtype, const void* images, int raw_dtype, float mean, float inv_std, int64_t B, int C, int Co,
                                int Hh, int Ww, uint64_t seed, uint32_t threshold, const int64_t* sample_ids, int64_t sample_base, int64_t id_bound,
                                float unmasked_label, int on_masked, float* loss, int64_t* count, void* workspace, size_t workspace_bytes,
                                void* stream) {
  const int rc = l1_check("mim_l1_fwd", out, images, raw_dtype, sample_ids, sample_base, id_bound, B, C, Co, Hh, Ww, threshold, dtype);
  if (rc) return rc;
  MEANT_REQUIRE(loss && count && cl_aligned(loss, 4) && cl_aligned(count, 8), MEANT_ERR_ARG, "mim_l1_fwd: null or misaligned loss / count");
  const L1Args a = l1_args(sample_ids, sample_base, B, C, Co, Hh, Ww, seed, threshold, mean, inv_std, unmasked_label, on_masked);
  const size_t need = meant_mim_l1_ws(a.N);
  MEANT_REQUIRE(workspace && workspace_bytes >= need && cl_aligned(workspace, 4), MEANT_ERR_WORKSPACE,
                "mim_l1_fwd: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
  const int64_t nparts = ceil_div(a.N, L1_SPAN);
  float* part_sum = (float*)workspace;
  uint32_t* part_cnt = (uint32_t*)((char*)workspace + need / 2);
  const dim3 grid((unsigned)nparts), block(CL_THREADS);
  hipStream_t st = (hipStream_t)stream;
  L1_DISPATCH(mim_l1_fwd_kernel, part_sum, part_cnt);
  MEANT_LAUNCH_CHECK("mim_l1_fwd");
  hipLaunchKernelGGL(mim_l1_finish_kernel, dim3(1), dim3(CL_THREADS), 0, st, (const float*)part_sum, (const uint32_t*)part_cnt, nparts, a.N, a.on_masked,
                     loss, count);
  MEANT_LAUNCH_CHECK("mim_l1_fwd (finish)");
  return MEANT_OK;
}

extern "C" int meant_mim_l1_bwd(const void* out, int dtype, const void* images, int raw_dtype, float mean, float inv_std, int64_t B, int C, int Co,
                                int Hh, int Ww, uint64_t seed, uint32_t threshold, const int64_t* sample_ids, int64_t sample_base, int64_t id_bound,
                                float unmasked_label, int on_masked, const float* g, const int64_t* count, void* dout, void* stream) {
  const int rc = l1_check("mim_l1_bwd", out, images, raw_dtype, sample_ids, sample_base, id_bound, B, C, Co, Hh, Ww, threshold, dtype);
  if (rc) return rc;
  MEANT_REQUIRE(g && dout && cl_aligned(g, 4) && cl_aligned(dout, dtype == MEANT_F32 ? 4 : 2) && (!on_masked || (count && cl_aligned(count, 8))),
                MEANT_ERR_ARG, "mim_l1_bwd: null or misaligned g / dout (/ count with on_masked)");
  MEANT_REQUIRE(dout != out, MEANT_ERR_ARG, "mim_l1_bwd: dout must not alias out");
  const L1Args a = l1_args(sample_ids, sample_base, B, C, Co, Hh, Ww, seed, threshold, mean, inv_std, unmasked_label, on_masked);
  const dim3 grid((unsigned)ceil_div(a.N, L1_SPAN)), block(CL_THREADS);
  hipStream_t st = (hipStream_t)stream;
  L1_DISPATCH(mim_l1_bwd_kernel, g, count, (T*)dout);
  MEANT_LAUNCH_CHECK("mim_l1_bwd");
  return MEANT_OK;
}
