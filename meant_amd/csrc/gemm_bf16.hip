// K5/K2: bf16 MFMA GEMMs of the MEANT path (the d x d Linears are 84 % of the step's FLOPs).
//
//   gemm_bf16_nt : C[M,N] = A[M,K] B[N,K]^T (+bias, GELU / sigmoid, +residual), both operands K-contiguous.
//                  Serves x W^T (forward) and dY (W^T)^T (input gradient, with a pre-transposed weight).
//   gemm_bf16_tn : dW[N,K] += dY[M,N]^T X[M,K] (reduction over the token axis M), fp32 atomics into dW.
//
// MI355X mapping
//   * 256 threads = 4 waves (2 x 2), block tile 128 x 128, K-step 64; each wave owns 64 x 64 of C in
//     16 (NT: 16x16x32) or 4 (TN: 32x32x16) MFMA accumulator tiles (64 accumulator VGPRs).
//   * operands go HBM -> LDS directly (global_load_lds, 16 B per lane, 1 KiB per wave-instruction),
//     double-buffered: the DMA of K-tile t+1 is in flight while tile t feeds the MFMAs; one barrier
//     per K-tile.
//   * LDS images are lane-linear (a DMA constraint), so the bank-conflict swizzle is applied on the
//     SOURCE address and again on the read:
//        NT: 128-byte rows, 16-byte chunk c of row r lives at slot c ^ ((r>>1)&7)   -> ds_read_b128
//            of an MFMA fragment (16 rows x one chunk per 16-lane group) touches 16 distinct slots.
//        TN: 256-byte rows (the reduction index is the ROW), chunk c of row r at slot c ^ (4*(r&3));
//            fragments come out of ds_read_b64_tr_b16 (hardware transpose), 4 consecutive rows each.
//   * blockIdx -> tile mapping is XCD-aware: the 8 XCDs have private L2s and blocks are dealt
//     round-robin, so ids are remapped to give each XCD a contiguous run of tiles; consecutive tiles
//     share the A row-panel (N/128 tiles per panel) which is then served from that XCD's L2, and the
//     weight matrix (<= 7 MB) stays resident in every L2.
//   * epilogue: accumulators -> LDS (fp32) -> coalesced 16-byte bf16 stores with bias / activation /
//     residual applied in fp32 and a single rounding.
// Roofline: MFMA-bound (dense bf16 peak 2.5 PFLOP/s); algorithmic FLOPs 2*M*N*K per launch.
#include "internal.h"
#include <type_traits>
#include <atomic>
#include <mutex>
#include <string>
#include <string.h>
#include <unordered_map>

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = BM * BK * 2;          // 16 KiB per operand per stage
constexpr int NT_LDS = 4 * TILE_BYTES;           // A0 B0 A1 B1 = 64 KiB (also holds the 128x128 fp32 epilogue tile)

__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((gbl_ptr_t)g, (lds_ptr_t)l, 16, 0, 0);
}

// bijective XCD-aware remap of a linear block id (guide: cdna_hip_programming.md T1)
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7, x = bid & 7, j = bid >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
}

// ------------------------------------------------------------------------------------------------
// K-tail forms (KTAIL = true) of the two one-tile NT kernels: K a multiple of 8 but not of 64.  The K loop runs ceil(K / 64)
// steps; a lane whose 8-element chunk starts at or beyond K takes its 16 bytes from this block of zeros instead of the operand,
// so the LDS tile holds zeros there and the MFMA loop and the epilogue are those of the K % 64 == 0 kernels.  The operand is
// never addressed at or beyond column K of a row: the next row's head belongs to another token (a NaN there would poison the
// product even when multiplied by the other operand's zeros), and the last row's tail is past the allocation.
__device__ __attribute__((aligned(16))) const unsigned g_nt_zero16[4] = {0u, 0u, 0u, 0u};   // read-only: nothing ever writes it

// source of the 16-byte chunk at columns kc .. kc+7 of row gr in the K-tail form
__device__ __forceinline__ const bf16* nt_tail_src(const bf16* __restrict__ g, int64_t ld, int64_t gr, int64_t kc, int64_t K) {
  const int64_t off = kc < K ? gr * ld + kc : 0;
  const bf16* p = g + off;
  return kc < K ? p : reinterpret_cast<const bf16*>(g_nt_zero16);
}

// ------------------------------------------------------------------------------------------------
// NT kernel
// stage a wave's 32 rows of a 64-column bf16 tile (rows row0.., columns k0..k0+63 of a K-contiguous matrix) into LDS: the 128-row
// tile of this kernel (4 waves) and the 256-row tile of the one-tile 256 x 256 kernel below (8 waves; 32 pieces of 1 KiB).
// wave w issues DMA pieces 4w..4w+3; piece i covers tile rows 8i..8i+7 (8 lanes per 128-byte row).
template <bool KTAIL>
__device__ __forceinline__ void nt_stage(const bf16* __restrict__ g, int64_t ld, int64_t row0, int64_t nrows, int64_t k0,
                                          char* lds_tile, int wave, int lane, int64_t K) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int piece = wave * 4 + i;
    const int r = piece * 8 + (lane >> 3);
    const int slot = lane & 7;
    const int c = slot ^ ((r >> 1) & 7);
    int64_t gr = row0 + r;
    gr = gr < nrows ? gr : nrows - 1;            // clamp: rows past the edge are computed and discarded
    if (KTAIL) glds16(nt_tail_src(g, ld, gr, k0 + c * 8, K), lds_tile + piece * 1024);
    else glds16(g + gr * ld + k0 + c * 8, lds_tile + piece * 1024);
  }
}

// one output row segment of 8 columns: v = acc + bias already; applies (optional) rotary, activation, residual,
// rounds once and stores 16 bytes.  Rotary epilogue (fused QKV projection): columns are [q | k | v] blocks of
// rot_D = H*Dh columns, a head is Dh columns, lanes c < R of every q/k head are rotated with the tables of the
// token's position m mod S:  out[c] = t[c]*A[pos,c] + rot(t)[c]*B[pos,c]  (meant/rotary_embedding_torch.py:31-44).
__device__ __forceinline__ void nt_store_row8(const GemmBf16Args& a, int64_t m, int64_t n, float (&v)[8], bool vec_ok) {
  if (a.epilogue & GEMM_EPI_F32_OUT) {               // C is float: acc + bias as it stands, two 16-byte stores
    float* c = reinterpret_cast<float*>(a.C) + m * a.ldc + n;
    if (vec_ok) {
      *reinterpret_cast<f32x4*>(c) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(c + 4) = f32x4{v[4], v[5], v[6], v[7]};
    } else {
      for (int e = 0; e < 8 && n + e < a.N; ++e) c[e] = v[e];
    }
    return;
  }
  if (vec_ok) {
    if (a.preact) {
      bf16x8 p;
#pragma unroll
      for (int e = 0; e < 8; ++e) p[e] = (bf16)v[e];
      *reinterpret_cast<bf16x8*>(a.preact + m * a.ldc + n) = p;
    }
    if (a.rot_qa) {
      const int64_t nq = n + a.col0;                 // column inside the q|k|v row (a launch may cover a part of it)
      const int sec = (int)(nq / a.rot_D);
      const int c = (int)((nq - (int64_t)sec * a.rot_D) % a.rot_Dh);
      if (sec < 2 && c < a.rot_R) {
        const int pos = (int)(m % a.rot_S);
        const float* A = (sec ? a.rot_ka : a.rot_qa) + (int64_t)pos * a.rot_R + c;
        const float* B = (sec ? a.rot_kb : a.rot_qb) + (int64_t)pos * a.rot_R + c;
        rot_apply8(v, *reinterpret_cast<const f32x4*>(A), *reinterpret_cast<const f32x4*>(A + 4),
                   *reinterpret_cast<const f32x4*>(B), *reinterpret_cast<const f32x4*>(B + 4));
      }
    }
    if (a.epilogue & MEANT_EPI_GELU) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = gelu_erf_fast(v[e]);
    }
    if (a.epilogue & MEANT_EPI_SIGMOID) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 1.f / (1.f + __expf(-v[e]));
    }
    if (a.residual) {
      const bf16x8 rr = *reinterpret_cast<const bf16x8*>(a.residual + m * a.ldr + n);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += (float)rr[e];
    }
    if (a.sub) {
      const bf16x8 sv = *reinterpret_cast<const bf16x8*>(a.sub + m * a.ldsub + n);
      const float kc = a.sub_coef[m];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaf(-kc, (float)sv[e], v[e]);
    }
    if (a.bres) {
      const float* bp = a.bres + (m / a.bres_rows) * a.N + n;
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(bp), b1 = *reinterpret_cast<const f32x4*>(bp + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaf(a.bres_scale, e < 4 ? b0[e] : b1[e - 4], v[e]);
    }
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (bf16)v[e];
    *reinterpret_cast<bf16x8*>(a.C + m * a.ldc + n) = o;
  } else {
    for (int e = 0; e < 8 && n + e < a.N; ++e) {
      float x = v[e];
      if (a.preact) a.preact[m * a.ldc + n + e] = (bf16)x;
      if (a.epilogue & MEANT_EPI_GELU) x = gelu_erf_fast(x);
      if (a.epilogue & MEANT_EPI_SIGMOID) x = 1.f / (1.f + __expf(-x));
      if (a.residual) x += (float)a.residual[m * a.ldr + n + e];
      if (a.sub) x -= a.sub_coef[m] * (float)a.sub[m * a.ldsub + n + e];
      if (a.bres) x += a.bres_scale * a.bres[(m / a.bres_rows) * a.N + n + e];
      a.C[m * a.ldc + n + e] = (bf16)x;
    }
  }
}

template <bool KTAIL>
__global__ __launch_bounds__(256, 2) void gemm_bf16_nt_kernel(GemmBf16Args a, int ntm, int ntn) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int id = xcd_remap(blockIdx.x, ntm * ntn);
  const int tm = id / ntn, tn = id - tm * ntn;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int nk = KTAIL ? (int)((a.K + BK - 1) / BK) : (int)(a.K / BK);

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  nt_stage<KTAIL>(a.A, a.lda, m0, a.M, 0, smem, wave, lane, a.K);
  nt_stage<KTAIL>(a.B, a.ldb, n0, a.N, 0, smem + TILE_BYTES, wave, lane, a.K);
  __syncthreads();                                  // (drains the DMA: vmcnt(0) + barrier)

  const int frow = lane & 15, fkg = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    char* cur = smem + (kt & 1) * 2 * TILE_BYTES;
    char* nxt = smem + ((kt + 1) & 1) * 2 * TILE_BYTES;
    if (kt + 1 < nk) {
      nt_stage<KTAIL>(a.A, a.lda, m0, a.M, (int64_t)(kt + 1) * BK, nxt, wave, lane, a.K);
      nt_stage<KTAIL>(a.B, a.ldb, n0, a.N, (int64_t)(kt + 1) * BK, nxt + TILE_BYTES, wave, lane, a.K);
    }
    const char* At = cur + (wm * 64) * 128;
    const char* Bt = cur + TILE_BYTES + (wn * 64) * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[4], bfr[4];
      const int c = ks * 4 + fkg;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = i * 16 + frow;
        const int off = r * 128 + ((c ^ ((r >> 1) & 7)) << 4);
        af[i] = *reinterpret_cast<const bf16x8*>(At + off);
        bfr[i] = *reinterpret_cast<const bf16x8*>(Bt + off);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue: acc -> LDS fp32 [128][132] -> coalesced stores --------------------------------
  constexpr int LDC = BN + 4;
  float* Cs = reinterpret_cast<float*>(smem);       // 128*132*4 = 67584 B <= NT_LDS + slack (see launch)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        Cs[(wm * 64 + i * 16 + fkg * 4 + e) * LDC + wn * 64 + j * 16 + frow] = acc[i][j][e];
  __syncthreads();
  // thread -> (row = pass*16 + tid/16, 8 columns at (tid%16)*8)
  const int cc = (tid & 15) * 8;
  const int64_t n = n0 + cc;
  float bias[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bias[e] = (a.bias && n + e < a.N) ? a.bias[n + e] : 0.f;
  const bool vec_ok = (n + 8 <= a.N) && ((a.ldc & 7) == 0) && (!a.residual || (a.ldr & 7) == 0);
#pragma unroll 2
  for (int pass = 0; pass < 8; ++pass) {
    const int r = pass * 16 + (tid >> 4);
    const int64_t m = m0 + r;
    if (m >= a.M || n >= a.N) continue;
    float v[8];
    const f32x4 lo = *reinterpret_cast<const f32x4*>(Cs + r * LDC + cc);
    const f32x4 hi = *reinterpret_cast<const f32x4*>(Cs + r * LDC + cc + 4);
    const float rs = a.row_scale ? a.row_scale[m] : 1.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = fmaf(e < 4 ? lo[e] : hi[e - 4], rs, bias[e]);
    nt_store_row8(a, m, n, v, vec_ok);
  }
}

// ------------------------------------------------------------------------------------------------
// NT kernel, 256 x 256 block tile, 512 threads = 8 waves (2 along M x 4 along N), 128 x 64 per wave.
// Why: the 128 x 128 kernel is bound by the L2 -> LDS load path (~40 GB/s per CU sustained = 64 FLOP per
// loaded byte x 40 GB/s x 256 CUs = 650 TFLOP/s, exactly what it measures); a 256 x 256 tile needs half the
// operand bytes per FLOP.  One block per CU (128 KiB of LDS: 2 stages x (A 32 KiB + B 32 KiB)), 2 waves/SIMD.
constexpr int B2 = 256;
constexpr int T2_BYTES = B2 * BK * 2;              // 32 KiB per operand per stage

template <bool KTAIL>
__global__ __launch_bounds__(512, 2) void gemm_bf16_nt256_kernel(GemmBf16Args a, int ntm, int ntn) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int id = xcd_remap(blockIdx.x, ntm * ntn);
  const int tm = id / ntn, tn = id - tm * ntn;
  const int64_t m0 = (int64_t)tm * B2, n0 = (int64_t)tn * B2;
  const int nk = KTAIL ? (int)((a.K + BK - 1) / BK) : (int)(a.K / BK);

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  nt_stage<KTAIL>(a.A, a.lda, m0, a.M, 0, smem, wave, lane, a.K);
  nt_stage<KTAIL>(a.B, a.ldb, n0, a.N, 0, smem + T2_BYTES, wave, lane, a.K);
  __syncthreads();

  const int frow = lane & 15, fkg = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    char* cur = smem + (kt & 1) * 2 * T2_BYTES;
    char* nxt = smem + ((kt + 1) & 1) * 2 * T2_BYTES;
    // Only waves 0-3 issue DMA (all 64 pieces of the next stage, 16 each): a wave issues no MFMA while it feeds pieces
    // to the address unit, and the two waves of a SIMD (w, w+4) would otherwise both do that right after the barrier
    // with the matrix pipe idle.  This way waves 4-7 start their MFMAs at once and their partners follow (+5 % on the
    // K-loop; issuing late instead -- after the MFMAs -- exposes the load latency at the barrier and measured -10 %).
    const bool late = __builtin_amdgcn_readfirstlane(threadIdx.x) >= 256;
    if (!late && kt + 1 < nk) {
      nt_stage<KTAIL>(a.A, a.lda, m0, a.M, (int64_t)(kt + 1) * BK, nxt, wave, lane, a.K);
      nt_stage<KTAIL>(a.B, a.ldb, n0, a.N, (int64_t)(kt + 1) * BK, nxt + T2_BYTES, wave, lane, a.K);
      nt_stage<KTAIL>(a.A, a.lda, m0, a.M, (int64_t)(kt + 1) * BK, nxt, wave + 4, lane, a.K);
      nt_stage<KTAIL>(a.B, a.ldb, n0, a.N, (int64_t)(kt + 1) * BK, nxt + T2_BYTES, wave + 4, lane, a.K);
    }
    const char* At = cur + (wm * 128) * 128;
    const char* Bt = cur + T2_BYTES + (wn * 64) * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[8], bfr[4];
      const int c = ks * 4 + fkg;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int r = i * 16 + frow;
        af[i] = *reinterpret_cast<const bf16x8*>(At + r * 128 + ((c ^ ((r >> 1) & 7)) << 4));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = j * 16 + frow;
        bfr[j] = *reinterpret_cast<const bf16x8*>(Bt + r * 128 + ((c ^ ((r >> 1) & 7)) << 4));
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);   // swapped: acc = C^T tile
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
  }

  // ---- epilogue: 4 passes of 64 rows through LDS (fp32 [64][260]) ---------------------------------
  constexpr int LDC = B2 + 4;
  float* Cs = reinterpret_cast<float*>(smem);
  const int cc = (tid & 31) * 8;
  const int64_t n = n0 + cc;
  float bias[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bias[e] = (a.bias && n + e < a.N) ? a.bias[n + e] : 0.f;
  const bool vec_ok = (n + 8 <= a.N) && ((a.ldc & 7) == 0) && (!a.residual || (a.ldr & 7) == 0);
  // Operands were fed swapped (B as the MFMA "A"), so acc[i][j][e] = C[m = i*16 + frow][n = j*16 + 4*fkg + e]: a lane
  // owns 4 CONSECUTIVE columns of one row and puts them into the staging tile with one ds_write_b128 (4x fewer LDS
  // store instructions than the natural layout).  Each pass takes 32 rows from each of the two wave rows, so all 8
  // waves write in every pass.
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    if (pass) __syncthreads();
#pragma unroll
    for (int ii = 0; ii < 2; ++ii) {
      const int i = pass * 2 + ii;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<f32x4*>(Cs + (wm * 32 + ii * 16 + frow) * LDC + wn * 64 + j * 16 + fkg * 4) = acc[i][j];
    }
    __syncthreads();
#pragma unroll 2
    for (int q = 0; q < 4; ++q) {
      const int r = q * 16 + (tid >> 5);               // staging row: (wave row, 32 rows of this pass)
      const int64_t m = m0 + (r >> 5) * 128 + pass * 32 + (r & 31);
      if (m >= a.M || n >= a.N) continue;
      float v[8];
      const f32x4 lo = *reinterpret_cast<const f32x4*>(Cs + r * LDC + cc);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(Cs + r * LDC + cc + 4);
      const float rs = a.row_scale ? a.row_scale[m] : 1.0f;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaf(e < 4 ? lo[e] : hi[e - 4], rs, bias[e]);
      nt_store_row8(a, m, n, v, vec_ok);
    }
  }
}

// The 160 KiB of LDS can hold a ring of FIVE 32 KiB operand tiles (A_0 B_0 A_1 B_1 A_2 ...; tile t lives in slot
// t mod 5) instead of two 64 KiB stages.  While step n computes from A_n / B_n, the DMA fills B_{n+1} (needed next
// step) and A_{n+2} (needed in two), so only half of a stage has to make the issue -> land round trip within one
// K-step; the barrier waits with a COUNTED vmcnt for exactly the tiles the next step needs.  (The two-stage kernel
// above is bound by that round trip: 64 KiB per CU through a 64 B/clk address path is 1024 clocks of issue alone
// before the last piece even starts its trip.)
constexpr int RING = 5;

// ------------------------------------------------------------------------------------------------
// Streaming (persistent) NT kernel: the kernel this file is built around for the tall GEMMs of the step.
//
// Same 256 x 256 tile and 8 waves as gemm_bf16_nt256_kernel, staged through the 5-slot ring; one workgroup per CU walks a
// SEQUENCE of tiles and treats all their K-steps as one stream: the ring keeps prefetching across the tile boundary
// (B of the next step, A of the one after -- whichever tile they belong to), and the epilogue needs no workgroup-wide
// staging buffer: each wave transposes its 16 x 64 pieces through a private 4 KiB patch in the two ring slots the
// finished step has just vacated and stores complete 128-byte lines.  What that buys at K = 768, where a tile is only
// 12 K-steps long:
//   * no prologue bubble per tile (the first operands of tile t+1 land while tile t still computes);
//   * no epilogue bubble: the 128 KiB of output per tile are fire-and-forget stores that drain under the next tile's
//     K-loop.  In the one-tile-per-workgroup kernels all 256 CUs finish together and write 32 MiB in one burst while
//     the matrix pipes wait for the stores (measured: 4 us of a 24 us tile for the stores, 5 us for the rest of the
//     prologue/epilogue).
// Requirements (the launcher falls back to the kernels above otherwise): M % 256 == 0 (or the ragged last tile, see the
// launcher), N % 256 == 0, K % 64 == 0, K >= 256, ldc % 8 == 0.
// Tile hand-out of the streaming kernel.  A fixed walk (tile += grid) is fragile: when another kernel -- the other HIP stream's,
// or a collective's -- holds a few CUs at launch, the workgroups that start late still own a full share of the tiles and the
// launch takes ~1.5x as long (measured with 8 of 256 CUs pinned: 1.07 -> 1.66 ms).  So only the FIRST tile of a workgroup is
// fixed; every further tile is drawn from a counter.  There is one counter per XCD so that the tiles an XCD works on stay
// neighbours (shared A panels / weights in its L2); an XCD that runs dry steals from the next one.  Tile k of XCD x is
// id(x, k) = (k / CH) * G + x * CH + k % CH with CH = G / 8 workgroups per XCD -- the same order as the fixed walk.
// The draw costs no stall: lane 0 of wave 4 sends the atomic at the top of K-step 2 and picks the answer up behind the wait
// that ends the step anyway; it publishes the tile id to a per-workgroup mailbox in global memory (LDS is full) with a
// fire-and-forget store, acknowledged by the end of step 3; every wave requests the mailbox at the top of step 4 and has it at
// the end of that step.  (Blocking versions of the same protocol cost 5-7 %: memory latency under this
// kernel's own load is ~4 us, two K-steps.)  The last workgroup to leave zeroes the counters for the next launch.
struct alignas(64) TileSched {
  unsigned next[8];
  unsigned done;
  unsigned steals;       // diagnostics: tiles taken from another XCD's counter (never reset by the kernel)
  unsigned pad[6];
  unsigned mailbox[512];
};
constexpr int N_SCHED_SLOTS = 256;
__device__ TileSched g_tile_sched[N_SCHED_SLOTS];

// ------------------------------------------------------------------------------------------------
// Epilogue of one wave's 128 x 64 accumulator block of a 256 x 256 tile (the streaming kernel's per-wave patch epilogue):
// accumulators -> the wave's two private 4 KiB LDS patches (fp32, XOR-swizzled, alternating per 16-row round) -> 128-byte
// row segments.  No workgroup barrier inside; the caller guarantees that nobody else touches the patches.
// Lane layout in: acc[i][j] = C[i*16 + frow][j*16 + 4*fkg .. +3]; out: lane l owns 8 consecutive columns (l & 7) * 8 of row
// (l >> 3) + 8h, i.e. one store instruction writes 8 complete 128-byte lines.  Patch I/O goes through inline asm: hipcc does
// not know the DMA ring is quiescent there and would put a vmcnt(0) -- a full drain of the output stores and of the prefetch in
// flight -- in front of every plain LDS store.
// Epilogue modes: what the launcher knows about a launch is a TEMPLATE parameter, so that the eight rounds are straight-line code.
// With the options as run-time flags every `if (a.residual)` / `if (a.preact)` ... is a branch with loads on one side, and at each
// join hipcc waits for vmcnt(0): every round then waited for the previous round's output stores to be ACKNOWLEDGED by memory
// (2.5 k cycles per round, 20 k of a 64 k-cycle tile at K = 768: round 4, per-phase timestamps) -- a store is fire-and-forget
// only while nothing behind it asks for the counter.
// Float output (GEMM_EPI_F32_OUT: C is float and takes acc + bias unrounded) is one more run-time flag of the generic instantiation, not
// a mode of its own: it loads nothing in its rounds, so nothing can queue behind its stores and they go out round by round as the plain
// mode's do, four 16-byte stores per round where that has two.
enum { NTE_PLAIN = 0, NTE_RES, NTE_GELU_PRE, NTE_ROT, NTE_EXT, NTE_GENERIC };
// Output stores as write-through (sc1) stores: a plain store leaves its line in the XCD's 4 MiB L2 (MI355X_MICROARCH.md, "stores of
// each flavour"), and a tile's 128 KiB of output per CU push the A panels the neighbouring CUs are about to re-read out of it.
// Measured (profiles/r04_nt256p_hbm_traffic*.json): HBM traffic 1.175x -> 1.08x of the algorithmic bytes at N = K = 768, 1.72x ->
// 1.65x at N = 2304; +1-2 % throughput.
#define GAS __attribute__((address_space(1)))
template <typename T> __device__ __forceinline__ const GAS T* gp(const T* p) { return (const GAS T*)p; }

template <int MODE>
__device__ __forceinline__ void nt256_wave_epilogue(const GemmBf16Args& a, f32x4 (&acc)[8][4], float* patch0, float* patch1, int64_t m0,
                                                    int64_t n0, int wm, int wn, int lane) {
  constexpr bool ROT = MODE == NTE_ROT, EXT = MODE == NTE_EXT, GEN = MODE == NTE_GENERIC || EXT;
  // compile-time constants in the specialised modes, run-time flags in the two generic ones
  const bool f_res = MODE == NTE_RES || (GEN && a.residual != nullptr);
  const bool f_pre = MODE == NTE_GELU_PRE || (GEN && a.preact != nullptr);
  const bool f_gelu = MODE == NTE_GELU_PRE || (GEN && (a.epilogue & MEANT_EPI_GELU));
  const bool f_sig = MODE == NTE_GENERIC && (a.epilogue & MEANT_EPI_SIGMOID);
  const bool f_f32 = MODE == NTE_GENERIC && (a.epilogue & GEMM_EPI_F32_OUT);
  const int frow = lane & 15, fkg = lane >> 4;
  float* patch[2] = {patch0, patch1};
  const int orow = lane >> 3, oc = lane & 7;
  const int64_t n = n0 + wn * 64 + oc * 8;
  const int64_t mrow = m0 + wm * 128 + orow;          // this lane's row of round 0, h = 0
  float bias[8];
  if (a.bias) {
    const f32x4 b0 = *gp(reinterpret_cast<const f32x4*>(a.bias + n)), b1 = *gp(reinterpret_cast<const f32x4*>(a.bias + n + 4));
#pragma unroll
    for (int e = 0; e < 8; ++e) bias[e] = e < 4 ? b0[e] : b1[e - 4];
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) bias[e] = 0.f;
  }
  const unsigned pw[2] = {lds_addr(patch[0]) + frow * 256, lds_addr(patch[1]) + frow * 256};
  // rotary epilogue (fused q|k|v projection): the lane's 8 columns sit at a fixed place c of a q or k head for the whole tile,
  // only the position m mod S changes.  vmcnt retires in order, so a table load issued after a round's output stores would wait
  // for those stores to be acknowledged: the operands of round r+1 are requested BEFORE the stores of round r go out.
  // The tile lies inside ONE of the q | k | v sections (256 divides H * Dh = 768; the launcher checks it), so "does this tile rotate
  // at all" is wave-uniform; inside a rotating tile every lane requests table rows (a lane whose 8 columns lie beyond the rotary
  // dimension reads the row's first columns and drops them): no divergent branch around the requests.  The position m mod S of a
  // lane's rows is formed ONCE per tile and stepped: a 64-bit modulo per row was ~60 of a round's 440 instructions.
  bool tile_rot = false, rot_on = false;
  const float *tabA = nullptr, *tabB = nullptr;
  unsigned posb = 0;
  const unsigned rS = ROT ? (unsigned)a.rot_S : 1u;
  const bool bigS = rS >= 256u;                        // then a lane's 16 rows of a tile wrap around S at most once
  if (ROT) {
    const int sec = __builtin_amdgcn_readfirstlane((int)((a.col0 + n0 + wn * 64) / a.rot_D));   // col0: the launch's first column of the q|k|v row
    const int c = (int)((a.col0 + n - (int64_t)sec * a.rot_D) % a.rot_Dh);
    tile_rot = sec < 2;
    rot_on = tile_rot && c < a.rot_R;
    tabA = (sec ? a.rot_ka : a.rot_qa) + (rot_on ? c : 0);
    tabB = (sec ? a.rot_kb : a.rot_qb) + (rot_on ? c : 0);
    posb = (unsigned)(mrow % (int64_t)rS);
  }
  auto pos_of = [&](int i, int h) {
    const unsigned p = posb + (unsigned)(i * 16 + 8 * h);
    return bigS ? (p >= rS ? p - rS : p) : p % rS;
  };
  // Operand registers of a round.  In the rotary mode there are TWO sets and a round's operands are requested two rounds ahead
  // (a round is ~500 cycles, an L2 hit under this kernel's own load more): set i & 1 serves round i and is refilled for round
  // i + 2 as soon as round i has consumed it.  The residual mode requests all eight rounds' rows (64 registers) before the first
  // round: nothing is ever requested behind a store (see DEFER).  The extended mode has no registers to spare (253) and keeps one set, one
  // round ahead.  Either way a round's requests go out BEFORE its stores -- loads never queue behind stores (vmcnt retires in order).
  constexpr int NS = MODE == NTE_ROT ? 2 : MODE == NTE_RES ? 8 : 1;   // residual mode: all eight rounds' rows requested up front
  f32x4 ta[NS][2][2], tb[NS][2][2];                // [set][h][half]
  bf16x8 xres[NS][2] = {}, xsub[2] = {};
  float xrs[2] = {1.f, 1.f}, xkc[2] = {0.f, 0.f};
  f32x4 xbr[2][2] = {};
  auto load_ops = [&](int i, int st) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t m = mrow + i * 16 + 8 * h;
      if (ROT) {
        if (tile_rot) {
          const unsigned o = pos_of(i, h) * (unsigned)a.rot_R;
          ta[st][h][0] = *gp(reinterpret_cast<const f32x4*>(tabA + o));
          ta[st][h][1] = *gp(reinterpret_cast<const f32x4*>(tabA + o + 4));
          tb[st][h][0] = *gp(reinterpret_cast<const f32x4*>(tabB + o));
          tb[st][h][1] = *gp(reinterpret_cast<const f32x4*>(tabB + o + 4));
        }
      } else {
        if (f_res) xres[st][h] = __builtin_nontemporal_load(gp(reinterpret_cast<const bf16x8*>(a.residual + m * a.ldr + n)));
        if (EXT) {
          if (a.row_scale) xrs[h] = *gp(a.row_scale + m);
          if (a.sub) {
            xsub[h] = *gp(reinterpret_cast<const bf16x8*>(a.sub + m * a.ldsub + n));
            xkc[h] = *gp(a.sub_coef + m);
          }
          if (a.bres) {
            const float* bp = a.bres + (m / a.bres_rows) * a.N + n;
            xbr[h][0] = *gp(reinterpret_cast<const f32x4*>(bp));
            xbr[h][1] = *gp(reinterpret_cast<const f32x4*>(bp + 4));
          }
        }
      }
    }
  };
#pragma unroll
  for (int i = 0; i < NS; ++i) load_ops(i, i);
  // output rows by running pointers (rows 8 apart: cstep8 elements): no 64-bit multiply per row
  const int64_t cstep8 = 8 * a.ldc;
  bf16* cp = a.C + mrow * a.ldc + n;
  bf16* pp = f_pre ? a.preact + mrow * a.ldc + n : nullptr;
  float* cpf = f_f32 ? reinterpret_cast<float*>(a.C) + mrow * a.ldc + n : nullptr;
  // vmcnt retires in order: a round's operand request issued behind an earlier round's output stores completes only when those
  // stores have been ACKNOWLEDGED by memory (microseconds under this kernel's own load) -- the rotary projection ran at 0.90 PFLOP/s
  // beside 1.14 for the plain epilogue, and neither fewer instructions per round (440 -> 200) nor one table address per wave
  // changed that.  In the rotary mode the finished rows are therefore HELD in registers (the accumulators drain twice as fast as
  // they fill: 16 registers freed, 8 taken per round) and stored after the last round's requests are out: 0.95-0.99 PFLOP/s.
  constexpr bool DEFER = MODE == NTE_ROT;
  bf16x8 held[DEFER ? 8 : 1][2];
  auto patch_write = [&](int i) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      asm volatile("ds_write_b128 %0, %1" ::"v"(pw[i & 1] + (((j * 4 + fkg) ^ frow) << 4)), "v"(acc[i][j]) : "memory");
  };
  patch_write(0);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int u = i & 1;                           // the two patches alternate
    const int st = NS == 2 ? u : NS == 8 ? i : 0;
    // both rows of the round come back in ONE asm statement that also waits for them: hipcc does not know an asm ds_read is
    // asynchronous and may copy its destination before a wait that sits in a later statement (tools/isa_inflight_check.py)
    f32x4 lo[2], hi[2];
    {
      const unsigned b0 = lds_addr(patch[u]) + orow * 256, b1 = b0 + 8 * 256;
      const int r0 = orow, r1 = orow + 8;
      asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %5\n\tds_read_b128 %2, %6\n\tds_read_b128 %3, %7\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(lo[0]), "=&v"(hi[0]), "=&v"(lo[1]), "=&v"(hi[1])
                   : "v"(b0 + (((2 * oc) ^ r0) << 4)), "v"(b0 + (((2 * oc + 1) ^ r0) << 4)), "v"(b1 + (((2 * oc) ^ r1) << 4)),
                     "v"(b1 + (((2 * oc + 1) ^ r1) << 4))
                   : "memory");
    }
    // the NEXT round's accumulators go into the other patch now: their LDS round trip runs under this round's arithmetic
    if (i + 1 < 8) patch_write(i + 1);
    __builtin_amdgcn_sched_barrier(0);
    bf16x8 outv[2], prev[2];
    f32x4 out32[2][2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaf(e < 4 ? lo[h][e] : hi[h][e - 4], EXT ? xrs[h] : 1.0f, bias[e]);
      if (f_f32) {
        out32[h][0] = f32x4{v[0], v[1], v[2], v[3]};
        out32[h][1] = f32x4{v[4], v[5], v[6], v[7]};
      }
      if (f_pre) {
#pragma unroll
        for (int e = 0; e < 8; ++e) prev[h][e] = (bf16)v[e];
      }
      if (ROT && tile_rot) {
        float w8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) w8[e] = v[e];
        rot_apply8(w8, ta[st][h][0], ta[st][h][1], tb[st][h][0], tb[st][h][1]);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = rot_on ? w8[e] : v[e];
      }
      if (f_gelu) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = gelu_erf_fast(v[e]);
      }
      if (f_sig) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 1.f / (1.f + __expf(-v[e]));
      }
      if (f_res) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += (float)xres[st][h][e];
      }
      if (EXT) {
        if (a.sub) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaf(-xkc[h], (float)xsub[h][e], v[e]);
        }
        if (a.bres) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = fmaf(a.bres_scale, e < 4 ? xbr[h][0][e] : xbr[h][1][e - 4], v[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) outv[h][e] = (bf16)v[e];
    }
    __builtin_amdgcn_sched_barrier(0);
    if (i + NS < 8) load_ops(i + NS, st);
    __builtin_amdgcn_sched_barrier(0);
    if (DEFER) {                                   // rotary / residual modes: see `held`
      held[i][0] = outv[0];
      held[i][1] = outv[1];
      continue;
    }
    if (f_f32) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float* const cq = cpf + (h ? cstep8 : 0);
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(cq), "v"(out32[h][0]) : "memory");
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(cq + 4), "v"(out32[h][1]) : "memory");
      }
      cpf += 2 * cstep8;
      continue;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      bf16* const cq = cp + (h ? cstep8 : 0);
      bf16* const pq = f_pre ? pp + (h ? cstep8 : 0) : nullptr;
      // write-through stores (see above).  The s_nop: the data registers of a 16-byte store may be rewritten right behind it
      // only after a wait state, which hipcc inserts for its own stores and cannot know about here
      if (f_pre) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(pq), "v"(prev[h]) : "memory");
      asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(cq), "v"(outv[h]) : "memory");
    }
    cp += 2 * cstep8;
    if (f_pre) pp += 2 * cstep8;
  }
  if (DEFER) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        bf16* const cq = cp + (h ? cstep8 : 0);
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(cq), "v"(held[i][h]) : "memory");
      }
      cp += 2 * cstep8;
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // the wave is out of its patches
}

// ------------------------------------------------------------------------------------------------
// Streaming NT kernel, PING-PONG form (round 4).  Tile 256 x 256 x 64, 8 waves (2 along M x 4 along N, 128 x 64 per wave), the
// five-slot ring, tile walk and per-wave patch epilogue described above -- and a schedule for WHEN the two waves of a SIMD do
// what.  In the lock-step form this replaced (retired) all eight waves ran in step: both waves of a SIMD read
// fragments at the same time (matrix pipe idle) and then both queued MFMAs (LDS and the address unit idle); a K-step measured
// 1.65 us against 1.08 us of MFMA time.  Here the workgroup is two GROUPS of four waves, one wave per SIMD each: the LEADER (waves
// 0-3, rows 0..127 of the tile) and the FOLLOWER (waves 4-7, rows 128..255), which runs the same program ONE BARRIER INTERVAL
// behind.  A K-step is TWO phases (one 64-row half of the wave's block x all of K = 64: 32 MFMAs; four phases of 16 and one of 64
// both measured slower); a phase is a LOAD half (the phase's fragment reads and its share of the prefetch stream's LDS-DMA
// pieces) and an MFMA half, with a workgroup barrier after each.  The one-interval lag puts every MFMA half of one group beside a
// LOAD half of the other: a SIMD's matrix pipe always has exactly one wave feeding it, and fragment reads, DMA issue and address
// arithmetic of its partner run underneath (cdna_hip_programming.md "The 256^2 8-phase template"; MI355X_MICROARCH.md "Two waves
// per SIMD", items 1, 5, 9).  A wave issues one instruction every ~4-5 cycles, so a LOAD half hides only while it stays well under
// (MFMAs per phase) x 16 / 4.5 instructions: the prefetch cursors are branch-free scalar selects, DMA pieces use the SGPR-base
// form (no per-piece VALU), and everything the epilogue needs is re-read from the kernarg segment per tile instead of living in
// SGPRs across the K-loop.
//
// Barrier intervals of K-step n, P = 2 (I = 4n + ...), L/M = load / MFMA half of phase p:
//     leader:    L0 M0 L1 M1          follower:  -- L0 M0 L1 | M1
// Prefetch stream (wave w owns pieces 4w .. 4w+3 of every tile: rows 32w .. 32w+31): the first half of a step's phases carries
// B of step n+1 (weights: L2 hits, needed at the next step's L0), the second half A of step n+2 (from HBM: more than a step of
// lead).  Each wave waits for its own pieces of step n+1 with a counted vmcnt (its four youngest requests, A of step n+2, stay
// in flight) just before the barrier in front of the leader's next L0: the leader at the end of its last M, the follower at the end
// of its last L.
// Slot reuse: B of step n+1 goes into the slot of A of step n-1, each wave into rows only its OWN group read (the leader's last
// reads of them are two intervals old, the follower's one and complete -- it has issued the MFMAs that needed them); A of step
// n+2 goes into the slot of B of step n-1, last read in the follower's first load half of that step.
// Tile end: the leader runs its epilogue in the interval in which the follower issues its last MFMAs and then runs its own (the
// two epilogues overlap), one barrier, then the leader's L0 of the next tile while the follower idles one interval.  The patches
// live in the two slots of the tile's last step, each wave inside rows only its own group read; the DMA into those slots starts
// behind that barrier.  After the last tile the cursors keep prefetching (valid rows of the last tile, never read): no branch
// in the K-loop distinguishes it.
// the four pieces (1 KiB each, consecutive in LDS) a wave owns of one tile (sbase, lds: wave-uniform).  ONE M0 write for the
// group; the instruction's immediate offset moves source and destination alike, so piece p's lane offset is built as
// v[p] - 1024 p (the launch code adds 3072 to every v[] and subtracts it from the base: the 32-bit lane offset is unsigned)
__device__ __forceinline__ void glds16_x4(const void* sbase, const unsigned (&v)[4], unsigned lds) {
  asm volatile("s_mov_b32 m0, %5\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %4\n\tglobal_load_lds_dwordx4 %1, %4 offset:1024\n\t"
               "global_load_lds_dwordx4 %2, %4 offset:2048\n\tglobal_load_lds_dwordx4 %3, %4 offset:3072"
               ::"v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "s"((const char*)sbase - 3072), "s"(lds) : "memory");
}
// the workgroup barrier of the two ping-pong kernels (this one and the 256 x 256 dW kernel), fenced against the scheduler on both sides
#define PP_BAR()                          \
  do {                                    \
    __builtin_amdgcn_sched_barrier(0);    \
    __builtin_amdgcn_s_barrier();         \
    __builtin_amdgcn_sched_barrier(0);    \
  } while (0)
typedef const __attribute__((address_space(4))) unsigned* kernarg_words_t;
static_assert(sizeof(GemmBf16Args) % 4 == 0, "kernarg copy by words");

template <int MODE>
__global__ __launch_bounds__(512, 2) void gemm_bf16_nt256p_kernel(GemmBf16Args a, int ntm, int ntn, TileSched* __restrict__ sched, int mode) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const bool leader = wm == 0;
  const int nk = (int)(a.K / BK);
  // Rotary mode with a panel list (the k|v section of a key-masked q|k|v projection): only the row panels plist[0 .. *panel_count) exist for
  // this launch -- the count is read here, the grid is the full problem's -- and tile row i of the walk is panel plist[i]; the list
  // comes in walk order (see rotP below).  Everything else (`listed` false) is the code it was.
  typedef const __attribute__((address_space(4))) int* panel_list_t;
  const bool listed = MODE == NTE_ROT && a.panel_list != nullptr;
  const panel_list_t plist = (panel_list_t)a.panel_list;
  const int ntiles = (listed ? __builtin_amdgcn_readfirstlane(*a.panel_count) : ntm) * ntn, G = gridDim.x;
  const int CH = G >> 3, xcd = blockIdx.x & 7;
  int tile = xcd * CH + (blockIdx.x >> 3);
  const bool dynamic = sched != nullptr && nk >= (listed ? 9 : 8);
  auto leave = [&]() {
    if (sched && threadIdx.x == 0) {
      if (atomicAdd(&sched->done, 1u) == (unsigned)G - 1u) {
#pragma unroll
        for (int i = 0; i < 8; ++i) sched->next[i] = 0;
        sched->done = 0;
      }
    }
  };
  if (tile >= ntiles) { leave(); return; }
  auto tile_of = [&](int x, unsigned k) { return (int)((k / (unsigned)CH) * (unsigned)G + (unsigned)(x * CH) + k % (unsigned)CH); };

  // DMA: piece q (1 KiB = 8 rows of 128 B) of a 32-piece tile; wave w owns pieces 4w + p, p = 0..3.  Row r of the tile keeps its
  // 16-byte chunk c at slot c ^ ((r >> 1) & 7): for r = 32w + 8p + (lane >> 3) that is (lane & 7) ^ (lane >> 4 & 3) ^ 4 (p & 1).
  const int rl = lane >> 3;
  const int c0 = (lane & 7) ^ (rl >> 1);
  unsigned vA[4], vB[4];                               // byte offsets of this lane's 16 bytes of piece p from the tile's origin
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    vA[p] = (unsigned)(((32 * wave + 8 * p + rl) * a.lda + (c0 ^ ((p & 1) << 2)) * 8) * 2) + (3072 - 1024 * p);
    vB[p] = (unsigned)(((32 * wave + 8 * p + rl) * a.ldb + (c0 ^ ((p & 1) << 2)) * 8) * 2) + (3072 - 1024 * p);
  }
  const unsigned lds0 = lds_addr(smem) + wave * 4096;  // this wave's first piece inside slot 0
  // Rotary mode, sequences of P = S / 256 > 1 row panels (mode bits 16..: P; the launcher checks that P divides the panel count):
  // the walk takes the panels of one position range after the other (all panels p with p mod P == 0, then == 1, ...) instead of in
  // memory order.  A tile's epilogue reads the 256 table rows of its positions (98 KB at R = 48); an XCD's 32 workgroups turn its
  // 4 MiB L2 over every ~3 us, and in memory order the ~3.5 panels an XCD has in flight cover all position ranges, so a table row is
  // touched again only every ~3 us per (range, section) -- it was evicted every time: 1.86 GB per launch of table rows from beyond L2
  // at (786432, 2304, 768), HBM-side traffic 2.05x the algorithmic bytes (profiles/r04_nt256p_hbm_traffic.json).  With one range
  // at a time the working set halves and every tile touches it.
  const int rotP = MODE == NTE_ROT ? (mode >> 16) : 1;
  const int rotQ = MODE == NTE_ROT && rotP > 1 ? ntm / rotP : 1;
  // (row panel, column tile) -> origins; origin(t): of tile t of the walk
  auto origin_at = [&](int tm, int tn, const bf16*& pa, const bf16*& pb, int64_t& m0, int64_t& n0) {
    m0 = (int64_t)tm * B2;
    n0 = (int64_t)tn * B2;
    pa = a.A + m0 * a.lda;
    pb = a.B + n0 * a.ldb;
  };
  auto origin = [&](int t, const bf16*& pa, const bf16*& pb, int64_t& m0, int64_t& n0) {
    int tm = t / ntn;
    const int tn = t - tm * ntn;
    if (MODE == NTE_ROT && listed) { origin_at(plist[tm], tn, pa, pb, m0, n0); return; }
    if (MODE == NTE_ROT && rotP > 1) { const int r = tm / rotQ; tm = (tm - r * rotQ) * rotP + r; }
    m0 = (int64_t)tm * B2;
    m0 = m0 + B2 <= a.M ? m0 : a.M - B2;               // ragged M: the last row tile is moved up to END at row M (see the launcher)
    n0 = (int64_t)tn * B2;
    pa = a.A + m0 * a.lda;
    pb = a.B + n0 * a.ldb;
  };

  const bf16 *pA, *pB, *pAn, *pBn;                     // origins of this tile and of the next one (the same when there is none)
  int64_t m0, n0, m0n, n0n;
  origin(tile, pA, pB, m0, n0);
  int next = dynamic ? -1 : tile + G;
  bool has_next = !dynamic && next < ntiles;
  pAn = pA; pBn = pB; m0n = m0; n0n = n0;
  if (has_next) origin(next, pAn, pBn, m0n, n0n);
  unsigned* mailbox = sched ? &sched->mailbox[blockIdx.x] : nullptr;

  // prologue: A_0, B_0, A_1 (four pieces per wave and tile); the first two must have landed
  glds16_x4(pA, vA, lds0);
  glds16_x4(pB, vB, lds0 + T2_BYTES);
  glds16_x4(pA + BK, vA, lds0 + 2 * T2_BYTES);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (!leader) {                                       // the follower's one-interval lag
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  // prefetch cursors: what the B pieces (one step ahead) and the A pieces (two steps ahead) of the CURRENT step read
  const bf16* qB = pB + BK;
  const bf16* qA = pA + 2 * BK;

  const int frow = lane & 15, fkg = lane >> 4;
  // fragment read offsets inside a slot: row i*16 + frow, chunk (ks*4 + fkg) ^ ((row >> 1) & 7); i adds 2048 bytes, ks flips bit 6
  const unsigned fo0 = (unsigned)(frow * 128 + ((fkg ^ (frow >> 1)) << 4));
  const unsigned foA[2] = {fo0 + wm * 16384, (fo0 ^ 64u) + wm * 16384};
  const unsigned foB[2] = {fo0 + wn * 8192, (fo0 ^ 64u) + wn * 8192};
  // ---- per-step scalars, software-pipelined: the values of step n+1 are computed in step n's LAST load half (beside the partner
  // group's MFMAs) and pinned in front of its barrier, so that nothing but the moves sits between a step's last barrier and the next
  // step's first DMA piece.  ring slot of A_n: sA; B_n sits in the next one, B_{n+1} goes to sA + 3, A_{n+2} to sA + 4 (mod 5).
  int kspecial = dynamic ? 2 : -1;                     // the draw: request in step 2, published behind it, read in step 4
  int next_tm = 0, next_tn = 0;                        // listed panels: the drawn tile's panel and column tile between steps 4 and 5
  int sA = 0;
  unsigned aoff = 0, boff = T2_BYTES, dB = lds0 + 3 * T2_BYTES, dA = lds0 + 4 * T2_BYTES;
  for (;;) {
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kt = 0; kt < nk; ++kt) {
      // tile draw, part 1 (see TileSched): requests only; they are older than this step's DMA pieces, so the counted wait that
      // ends the step covers them.  hipcc does not know the register is in flight until then, and wherever control flow joins it
      // is free to copy a register (it did: a v_mov of the ticket at a branch join, found by tools/isa_inflight.py) -- so both
      // requests are STRAIGHT-LINE code: one asm statement each, executed in every step, that narrows EXEC to the lanes that
      // really ask (none in most steps: the instruction is then skipped) and restores it; one fresh register per step takes
      // whichever answer the step has.  The load halves stay short: a dozen scalar instructions per step.
      unsigned req;
      asm volatile("" : "=v"(req));                     // "defined" without an instruction
      const bool special = kt == kspecial;              // kspecial: 2, then 4, then never (-1 without the dynamic hand-out)
      const bool own = !((mode & 0xff) == 3 && xcd != 0);
      const bool drawing = special && kt == 2 && wave == 4;
      {
        // EXEC masks as 32-bit halves that are provably scalar (a 64-bit select of constants ends up on the VALU)
        const int m_draw = __builtin_amdgcn_readfirstlane(drawing && own ? 1 : 0);       // lane 0 of wave 4
        const int m_read = __builtin_amdgcn_readfirstlane(special && kt == 4 ? -1 : 0);  // every lane of every wave
        unsigned long long keep;
        asm volatile("s_mov_b64 %1, exec\n\ts_mov_b32 exec_lo, %2\n\ts_mov_b32 exec_hi, 0\n\tglobal_atomic_add %0, %3, %4, off sc0\n\ts_mov_b64 exec, %1"
                     : "+v"(req), "=&s"(keep) : "s"(m_draw), "v"(sched ? &sched->next[xcd] : nullptr), "v"(1u) : "memory");
        asm volatile("s_mov_b64 %1, exec\n\ts_mov_b32 exec_lo, %2\n\ts_mov_b32 exec_hi, %2\n\tglobal_load_dword %0, %3, off sc1\n\ts_mov_b64 exec, %1"
                     : "+v"(req), "=&s"(keep) : "s"(m_read), "v"(mailbox) : "memory");
      }
      const bool drawer = drawing && lane == 0;

      bf16x8 aq[2][4], bq[2][4];
      auto ldA = [&](int ih, int ks, bf16x8 (&d)[4]) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) d[ii] = *reinterpret_cast<const bf16x8*>(smem + aoff + foA[ks] + (ih * 4 + ii) * 2048);
      };
      auto ldB = [&](int ks, bf16x8 (&d)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = *reinterpret_cast<const bf16x8*>(smem + boff + foB[ks] + j * 2048);
      };
      auto mm = [&](int ih, const bf16x8 (&av)[4], const bf16x8 (&bv)[4]) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[ih * 4 + ii][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bv[j], av[ii], acc[ih * 4 + ii][j], 0, 0, 0);   // swapped: acc = C^T tile
      };
      auto wait_step = [&]() { asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); };
      // ---- phase 0: rows 0..63 of the wave's block, both k-halves ------------------------------------------------------
      glds16_x4(qB, vB, dB);
      ldB(0, bq[0]); ldB(1, bq[1]);
      ldA(0, 0, aq[0]); ldA(0, 1, aq[1]);
      PP_BAR();
      __builtin_amdgcn_s_setprio(1);
      mm(0, aq[0], bq[0]); mm(0, aq[1], bq[1]);
      __builtin_amdgcn_s_setprio(0);
      PP_BAR();
      // ---- phase 1: rows 64..127 --------------------------------------------------------------------------------------
      glds16_x4(qA, vA, dA);
      ldA(1, 0, aq[0]); ldA(1, 1, aq[1]);
      // the next step's scalars (see above).  Cursors: one K-block on, or into the next tile when the step they feed is one (B: step
      // kt + 2 of this tile does not exist; A: step kt + 3).  pAn / pBn are final by then: the draw is read behind step 4 and
      // the dynamic hand-out needs nk >= 8.
      int n_sA = sA + 2 >= RING ? sA + 2 - RING : sA + 2;
      const int n_sB = n_sA + 1 == RING ? 0 : n_sA + 1;
      const int n_s3 = n_sA + 3 >= RING ? n_sA + 3 - RING : n_sA + 3, n_s4 = n_sA + 4 >= RING ? n_sA + 4 - RING : n_sA + 4;
      unsigned n_aoff = (unsigned)n_sA * T2_BYTES, n_boff = (unsigned)n_sB * T2_BYTES;
      unsigned n_dB = lds0 + (unsigned)n_s3 * T2_BYTES, n_dA = lds0 + (unsigned)n_s4 * T2_BYTES;
      const bf16* n_qB = kt + 2 == nk ? pBn : qB + BK;
      const bf16* n_qA = kt + 3 == nk ? pAn : qA + BK;
      asm volatile("" : "+s"(n_sA), "+s"(n_aoff), "+s"(n_boff), "+s"(n_dB), "+s"(n_dA), "+s"(n_qB), "+s"(n_qA));
      __builtin_amdgcn_sched_barrier(0);
      if (!leader) wait_step();                        // follower: its pieces of the next step must be in before the leader's L0
      PP_BAR();
      __builtin_amdgcn_s_setprio(1);
      mm(1, aq[0], bq[0]); mm(1, aq[1], bq[1]);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      if (leader) wait_step();
      // the follower's last MFMAs of a tile and its epilogue share one interval (see the header)
      if (leader || kt + 1 < nk) PP_BAR();
      sA = n_sA; aoff = n_aoff; boff = n_boff; dB = n_dB; dA = n_dA; qB = n_qB; qA = n_qA;
      if (special) {
        // tile draw, part 2: the answer is here (the step's counted wait covered it)
        asm volatile("" : "+v"(req) : : "memory");
        if (drawer) {
          int id = own ? tile_of(xcd, (unsigned)CH + req) : ntiles;
          if (id >= ntiles) {
            unsigned seen[8];
#pragma unroll
            for (int x = 0; x < 8; ++x) seen[x] = __hip_atomic_load(&sched->next[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int att = 1; id >= ntiles && att < 8; ++att) {
              const int x2 = (xcd + att) & 7;
              if (tile_of(x2, (unsigned)CH + seen[x2]) >= ntiles) continue;
              id = tile_of(x2, (unsigned)CH + atomicAdd(&sched->next[x2], 1u));
              if (id < ntiles) atomicAdd(&sched->steals, 1u);
            }
          }
          const unsigned pub = id < ntiles ? (unsigned)id : 0xffffffffu;
          asm volatile("global_store_dword %0, %1, off sc1" ::"v"(mailbox), "v"(pub) : "memory");
        }
        if (kt == 4) {
          const unsigned got = (unsigned)__builtin_amdgcn_readfirstlane((int)req);
          next = (int)got;
          has_next = next >= 0;
          if (MODE == NTE_ROT && listed) {
            // the panel index is one more (scalar) load: requested here, turned into the origins behind step 5 -- the first wait
            // of that step's MFMA half has covered it by then -- which is in time for the cursors of step nk - 3 >= 6
            const int tq = next / ntn;
            next_tn = next - tq * ntn;
            next_tm = plist[has_next ? tq : 0];
          } else if (has_next) origin(next, pAn, pBn, m0n, n0n);
        }
        if (MODE == NTE_ROT && kt == 5 && has_next) origin_at(next_tm, next_tn, pAn, pBn, m0n, n0n);
        kspecial = kt == 2 ? 4 : (MODE == NTE_ROT && listed && kt == 4) ? 5 : -1;
      }
    }
    kspecial = dynamic ? 2 : -1;

    // ---- epilogue: the two slots of the tile's last step are free; each wave's patches lie inside rows only its own group read.
    // Its arguments come fresh from the kernarg segment (the pointer is laundered so that hipcc cannot keep them in SGPRs
    // across the K-loop, where they spill into VGPR lanes and cost the load halves v_readlane / s_nop pairs).
    {
      const int f3 = sA + 3 >= RING ? sA + 3 - RING : sA + 3, f4 = sA + 4 >= RING ? sA + 4 - RING : sA + 4;
      kernarg_words_t ka = (kernarg_words_t)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(ka));
      unsigned kw[sizeof(GemmBf16Args) / 4];
#pragma unroll
      for (unsigned i = 0; i < sizeof(GemmBf16Args) / 4; ++i) kw[i] = ka[i];
      GemmBf16Args ea;
      __builtin_memcpy(&ea, kw, sizeof(GemmBf16Args));
      nt256_wave_epilogue<MODE>(ea, acc, reinterpret_cast<float*>(smem + f3 * T2_BYTES + wave * 4096),
                                    reinterpret_cast<float*>(smem + f4 * T2_BYTES + wave * 4096), m0, n0, wm, wn, lane);
    }
    PP_BAR();
    if (!has_next) break;
    if (!leader) PP_BAR();                             // the follower idles through the leader's first L0
    tile = next; pA = pAn; pB = pBn; m0 = m0n; n0 = n0n;
    if (dynamic) { next = -1; has_next = false; }
    else {
      next = next + G;
      has_next = next < ntiles;
      if (has_next) origin(next, pAn, pBn, m0n, n0n);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the cursors' last (unused) pieces
  leave();
}

// ------------------------------------------------------------------------------------------------
// TN kernel: dW[n][k] += sum_m dY[m][n] X[m][k].  LDS tiles are [64 m][128 cols] (256-byte rows).
constexpr int TN_BKM = 64;
constexpr int TN_TILE_BYTES = TN_BKM * 128 * 2;    // 16 KiB

// piece i (1 KiB) covers tile rows 4i..4i+3 (16 lanes per 256-byte row); wave w issues pieces 4w..4w+3.
__device__ __forceinline__ void tn_stage(const bf16* __restrict__ g, int64_t ld, int64_t m0, int64_t mend, int64_t col0,
                                          int64_t ncols, char* lds_tile, int wave, int lane) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int piece = wave * 4 + i;
    const int r = piece * 4 + (lane >> 4);
    const int slot = lane & 15;
    const int c = slot ^ ((r & 3) << 2);
    const int64_t gm = m0 + r;                     // always < mend: the launcher hands over whole 64-row tiles only
    int64_t gc = col0 + c * 8;
    gc = gc + 8 <= ncols ? gc : (ncols >= 8 ? ncols - 8 : 0);     // column clamp (those outputs are discarded)
    glds16(g + gm * ld + gc, lds_tile + piece * 1024);
  }
}

// fragment for mfma_32x32x16: lane (col = lane&31, h = lane>>5) needs rows 16*ks + 8h + j (j = 0..7) of column
// col0 + col: two transposed reads of 4 consecutive rows each.
__device__ __forceinline__ bf16x8 tn_frag(const char* tile, int ks, int col0, int lane) {
  const int h = lane >> 5;
  const int i16 = lane & 15;                       // lane within its 16-lane group
  const int q = i16 >> 2, p = i16 & 3;
  const int colblk = col0 + ((lane >> 4) & 1) * 16; // groups 0/1 (and 2/3) take adjacent 16-column blocks
  const int cbyte = (colblk + 4 * p) * 2;          // byte offset of this lane's 4 columns inside the row
  const int c16 = cbyte >> 4, sub = cbyte & 15;
  bf16x8 out;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r = 16 * ks + 8 * h + 4 * t + q;
    const int off = r * 256 + ((c16 ^ ((r & 3) << 2)) << 4) + sub;
    const bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(tile + off));
    out[4 * t + 0] = v[0]; out[4 * t + 1] = v[1]; out[4 * t + 2] = v[2]; out[4 * t + 3] = v[3];
  }
  return out;
}

__global__ __launch_bounds__(256, 2) void gemm_bf16_tn_kernel(const bf16* __restrict__ dY, int64_t lddy, const bf16* __restrict__ X,
                                                               int64_t ldx, float* __restrict__ dW, int64_t M, int64_t N,
                                                               int64_t K, int ntn, int ntk, int64_t rows_per_split) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);   // a split's tiles run on one XCD and share its L2
  const int tile = bid % (ntn * ntk);
  const int split = bid / (ntn * ntk);
  const int tn = tile / ntk, tk = tile - tn * ntk;
  const int64_t n0 = (int64_t)tn * 128, k0 = (int64_t)tk * 128;
  const int64_t mbeg = (int64_t)split * rows_per_split;
  const int64_t mend = (mbeg + rows_per_split < M) ? mbeg + rows_per_split : M;
  if (mbeg >= mend) return;
  const int nt = (int)((mend - mbeg + TN_BKM - 1) / TN_BKM);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  tn_stage(dY, lddy, mbeg, mend, n0, N, smem, wave, lane);
  tn_stage(X, ldx, mbeg, mend, k0, K, smem + TN_TILE_BYTES, wave, lane);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    char* cur = smem + (t & 1) * 2 * TN_TILE_BYTES;
    char* nxt = smem + ((t + 1) & 1) * 2 * TN_TILE_BYTES;
    if (t + 1 < nt) {
      tn_stage(dY, lddy, mbeg + (int64_t)(t + 1) * TN_BKM, mend, n0, N, nxt, wave, lane);
      tn_stage(X, ldx, mbeg + (int64_t)(t + 1) * TN_BKM, mend, k0, K, nxt + TN_TILE_BYTES, wave, lane);
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = tn_frag(cur, ks, wn * 64 + i * 32, lane);
        bfr[i] = tn_frag(cur + TN_TILE_BYTES, ks, wk * 64 + i * 32, lane);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  // C layout of 32x32: col = lane&31 (k index), row = (e&3) + 8*(e>>2) + 4*(lane>>5) (n index): every
  // wave-instruction adds two 128-byte row segments -> the full-rate shape for global float atomics.
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int64_t kcol = k0 + wk * 64 + j * 32 + (lane & 31);
      if (kcol >= K) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t nrow = n0 + wn * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (nrow < N) atomicAdd(dW + nrow * K + kcol, acc[i][j][e]);
      }
    }
}

// ------------------------------------------------------------------------------------------------
// dW kernel, 256 x 256 output tile: same load-path argument as the 256 x 256 NT kernel.  The bias gradient (column sums of dY)
// is accumulated from the dY fragments the workgroups already hold -- no separate pass over dY.
// per-lane byte offset (inside a [64][256] tile) of the transposed-read address for the 32-column block at col0:
// row 8h + q of the first k-step, this lane's 4 columns; k-step ks / half t add (16 ks + 4 t) * 512 as an immediate.
__device__ __forceinline__ unsigned tn256_lane_off(int col0, int lane) {
  const int h = lane >> 5, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
  const int cbyte = (col0 + ((lane >> 4) & 1) * 16 + 4 * p) * 2;
  const int r = 8 * h + q;                          // (r & 3) == q for every (ks, t)
  return (unsigned)(r * 512 + (((cbyte >> 4) ^ (q << 2)) << 4) + (cbyte & 15));
}
template <int KS>
__device__ __forceinline__ void tn256_frag_issue(unsigned addr, u32x2& lo, u32x2& hi) {
  lo = lds_read_tr16<KS * 8192>(addr);
  hi = lds_read_tr16<KS * 8192 + 2048>(addr);
}

// ------------------------------------------------------------------------------------------------
// DET: instead of float atomics on dW / dbias (whose order differs from run to run) every workgroup stores its 256 x 256 partial
// tile to `part` [split][tile][256][256] and its bias partials to `pbias` [split][tk][wk][N]; tn256_reduce_kernel then adds them
// up in a fixed order.  Same MFMA stream, so the partial sums themselves are bit-identical between runs.
// dW kernel, PING-PONG form (round 4): the structure of gemm_bf16_nt256p_kernel on the tiles and fragments above.  Output tile 256
// (n) x 256 (k), waves 2 (n) x 4 (k), 128 x 64 per wave in 4 x 2 accumulators of v_mfma_f32_32x32x16_bf16; a STEP is 64 token
// rows ([64 m][256] tiles of dY and X, 512-byte rows, transposed fragment reads), a phase is one half of them (k-steps 0-1: token
// rows 0..31; k-steps 2-3: rows 32..63): 24 ds_read_b64_tr_b16 + 4 LDS-DMA pieces in its LOAD half, 16 MFMAs (512 cycles) in its
// MFMA half.  The leader (waves 0-3: n rows 0..127) and the follower (waves 4-7) run one barrier interval apart, so one wave of
// every SIMD is always in an MFMA half.
// Ring of five 32 KiB slots: dY_t, X_t, dY_t+1, X_t+1 (landing during step t), dY_t+2 (landing).  Every wave reads all 64 token rows of
// both tiles (its own columns), so a slot of step t-1 is refilled by halves: token rows 0..31 were last read in the follower's first
// load half of step t-1 and are refilled by waves 0-3 (pieces 4w + p = rows 8w + 2p ..) from the leader's L0 of step t on; rows
// 32..63 were last read in the follower's second load half and are refilled by waves 4-7, whose L0 of step t comes behind the
// barrier that follows those reads' completion.
// Steps past the end of the split keep prefetching its last rows (never read): no branch in the loop distinguishes them.
//
// ROWS: the reduction runs over a LIST of 64-row blocks of the token axis (`rows`, ascending block indices; `*rows_count` of them, read
// here: the host never learns the count) instead of over all of M -- the k|v columns of the q|k|v projection's weight gradient, whose
// dK / dV rows are exact zeros for every block of padded keys the attention skipped.  A step's token rows are block rows[base + t]; a
// split's share is ceil(count / splits) blocks (`rows_per_split` carries the number of splits), so the splits stay balanced whatever
// the padding.  The cursors become pointers that are READY when the load half wants them: in step t the index of block t + 4 is
// requested by a scalar load at the top of the first MFMA half and, behind the last MFMA of the second one, turned into the dY rows the
// next step's load half will ask for (with the X rows of block t + 3, whose index came a step earlier); the load halves only move them.  A wave touches its split's part of the
// list once in the prologue (a vector load the prologue's counted wait covers), so that those scalar loads find it in the XCD's L2.
template <bool DET, bool ROWS = false>
__global__ __launch_bounds__(512, 2) void gemm_bf16_tn256p_kernel(const bf16* __restrict__ dY, int64_t lddy, const bf16* __restrict__ X,
                                                                   int64_t ldx, float* __restrict__ dW, float* __restrict__ dbias,
                                                                   int64_t M, int64_t N, int64_t K, int ntn, int ntk,
                                                                   int64_t rows_per_split, float* __restrict__ part,
                                                                   float* __restrict__ pbias, const int* __restrict__ rows,
                                                                   const int* __restrict__ rows_count) {
  static_assert(!(DET && ROWS), "the row-list form has no deterministic variant");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 2, wk = wave & 3;
  const bool leader = wn == 0;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  // (integer division runs on the VALU: say explicitly that the quotients are wave-uniform, they end up as SGPR operands of asm)
  const int tile = __builtin_amdgcn_readfirstlane(bid % (ntn * ntk));
  const int split = __builtin_amdgcn_readfirstlane(bid / (ntn * ntk));
  const int tn = tile / ntk, tk = tile - tn * ntk;
  const int64_t n0 = (int64_t)tn * 256, k0 = (int64_t)tk * 256;
  int64_t mbeg = 0;
  int nt;
  typedef const __attribute__((address_space(4))) int* rows_list_t;   // scalar loads
  rows_list_t rl = nullptr;                            // ROWS: this split's part of the list
  int touch = 0;
  if (ROWS) {
    const int cnt = __builtin_amdgcn_readfirstlane(*rows_count);
    const int nsplit = (int)rows_per_split;
    const int share = __builtin_amdgcn_readfirstlane((cnt + nsplit - 1) / nsplit);
    const int base = split * share;
    nt = cnt - base < share ? cnt - base : share;
    if (nt <= 0) return;
    rl = (rows_list_t)(rows + base);
    // one word per 64-byte line of the split's part (its first 1024 blocks: more than a split of the step's shapes has)
    touch = rows[base + (lane * 16 < nt ? lane * 16 : 0)];
  } else {
    mbeg = (int64_t)split * rows_per_split;
    const int64_t mend = (mbeg + rows_per_split < M) ? mbeg + rows_per_split : M;
    if (mbeg >= mend) return;
    nt = __builtin_amdgcn_readfirstlane((int)((mend - mbeg + TN_BKM - 1) / TN_BKM));
  }
  const bool do_bias = dbias != nullptr;

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  float csum[4] = {0.f, 0.f, 0.f, 0.f};
  unsigned aoff[4], boff[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) aoff[i] = tn256_lane_off(wn * 128 + i * 32, lane);
#pragma unroll
  for (int j = 0; j < 2; ++j) boff[j] = tn256_lane_off(wk * 64 + j * 32, lane);

  // DMA: piece q (1 KiB = 2 token rows of 512 B) of a 32-piece tile; wave w owns pieces 4w + p, i.e. rows 8w + 2p + (lane >> 5).
  // 16-byte chunk c of row r sits at slot c ^ (4 (r & 3)), and r & 3 = 2 (p & 1) + (lane >> 5).
  unsigned vY[4], vX[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = 8 * wave + 2 * p + (lane >> 5);
    const int c = (lane & 31) ^ ((r & 3) << 2);
    vY[p] = (unsigned)((r * lddy + c * 8) * 2) + (3072 - 1024 * p);
    vX[p] = (unsigned)((r * ldx + c * 8) * 2) + (3072 - 1024 * p);
  }
  const unsigned lds0 = lds_addr(smem) + wave * 4096;
  // ROWS: first rows of block i of the split's list (clamped to its last one), in dY and in X
  auto rowsY = [&](int blk) { return dY + (int64_t)blk * (TN_BKM * lddy) + n0; };
  auto rowsX = [&](int blk) { return X + (int64_t)blk * (TN_BKM * ldx) + k0; };
  auto blk_at = [&](int i) { return rl[i < nt ? i : nt - 1]; };
  const int b0 = ROWS ? blk_at(0) : 0, b1 = ROWS ? blk_at(1) : 0, b2 = ROWS ? blk_at(2) : 0;
  int bn = ROWS ? blk_at(3) : 0;                       // ROWS: the block of step t + 3 at the top of step t
  const bf16* pY = ROWS ? rowsY(b0) : dY + mbeg * lddy + n0;
  const bf16* pX = ROWS ? rowsX(b0) : X + mbeg * ldx + k0;
  const int64_t stepY = (int64_t)TN_BKM * lddy, stepX = (int64_t)TN_BKM * ldx;
  // prologue: dY_0, X_0, dY_1 (the last step's rows again when the split has a single step)
  const bf16* qY = ROWS ? rowsY(b1) : nt > 1 ? pY + stepY : pY;   // cursor of the dY pieces: two steps ahead of the step that issues them
  glds16_x4(pY, vY, lds0);
  glds16_x4(pX, vX, lds0 + T2_BYTES);
  glds16_x4(qY, vY, lds0 + 2 * T2_BYTES);
  const bf16* qX = ROWS ? rowsX(b1) : nt > 1 ? pX + stepX : pX;   // cursor of the X pieces: one step ahead
  qY = ROWS ? rowsY(b2) : nt > 2 ? qY + stepY : qY;
  // ROWS: what the cursors become in step 0's second load half (X of step 2, dY of step 3)
  const bf16* nxtX = ROWS ? rowsX(b2) : nullptr;
  const bf16* nxtY = ROWS ? rowsY(bn) : nullptr;
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  if (ROWS) asm volatile("" ::"v"(touch));             // (the list touch has landed: hipcc waits for it here, behind the counted wait)
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (!leader) {                                       // the follower's one-interval lag
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  const unsigned sbase = lds_addr(smem);
  int sA = 0;
  unsigned ya = sbase, xa = sbase + T2_BYTES, dXs = lds0 + 3 * T2_BYTES, dYs = lds0 + 4 * T2_BYTES;
  for (int t = 0; t < nt; ++t) {
    const bool bias_step = do_bias && (t % ntk) == tk;
    u32x2 alo[2][4], ahi[2][4], blo[2][2], bhi[2][2];
    // the 24 transposed reads of one phase (k-steps 2 ph and 2 ph + 1), inline asm: nothing may touch the destinations before the
    // lgkmcnt(0) at the top of the MFMA half (tools/isa_inflight_check.py)
    auto frag_reads = [&](auto PH) {
      constexpr int ph = decltype(PH)::value;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        alo[0][i] = lds_read_tr16<(2 * ph) * 8192>(ya + aoff[i]);
        ahi[0][i] = lds_read_tr16<(2 * ph) * 8192 + 2048>(ya + aoff[i]);
        alo[1][i] = lds_read_tr16<(2 * ph + 1) * 8192>(ya + aoff[i]);
        ahi[1][i] = lds_read_tr16<(2 * ph + 1) * 8192 + 2048>(ya + aoff[i]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        blo[0][j] = lds_read_tr16<(2 * ph) * 8192>(xa + boff[j]);
        bhi[0][j] = lds_read_tr16<(2 * ph) * 8192 + 2048>(xa + boff[j]);
        blo[1][j] = lds_read_tr16<(2 * ph + 1) * 8192>(xa + boff[j]);
        bhi[1][j] = lds_read_tr16<(2 * ph + 1) * 8192 + 2048>(xa + boff[j]);
      }
    };
    int bnew = 0;
    auto mfma_half = [&](int ph) {
      lds_wait_all();
      // ROWS: the block of step t + 4 -- requested behind the wait (nothing of this wave's is in flight on the counter the fragment
      // reads use), picked up behind the last MFMA of the step's second half
      if (ROWS && ph == 0) {
        bnew = blk_at(t + 4);
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 af[4], bfr[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = pack_tr(alo[s2][i], ahi[s2][i]);
#pragma unroll
        for (int j = 0; j < 2; ++j) bfr[j] = pack_tr(blo[s2][j], bhi[s2][j]);
        // fused dbias: column sums of dY from the A fragments, dealt out over the k-tiles' workgroups (step t belongs to the one
        // with tk == t mod ntk) and over a workgroup's waves (k-sub-step ks belongs to wave wk == ks).  The adds of fragment i sit
        // BEHIND its two MFMAs (which took their operands at issue) and in front of the next pair: an MFMA holds the matrix pipe for
        // 32 cycles and the issue port for 8 of them, so a dozen vector instructions per pair ride along
        const bool bias_now = bias_step && 2 * ph + s2 == wk;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          if (bias_now) {
#pragma unroll
            for (int e = 0; e < 8; ++e) csum[i] += (float)af[i][e];
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    };
    // ---- phase 0: token rows 0..31 ----------------------------------------------------------------------------------------
    glds16_x4(qX, vX, dXs);
    frag_reads(std::integral_constant<int, 0>{});
    PP_BAR();
    mfma_half(0);
    PP_BAR();
    // ---- phase 1: token rows 32..63 ---------------------------------------------------------------------------------------
    glds16_x4(qY, vY, dYs);
    frag_reads(std::integral_constant<int, 1>{});
    // the next step's scalars, computed here (beside the partner group's MFMAs) and pinned in front of the barrier
    int n_sA = sA + 2 >= RING ? sA + 2 - RING : sA + 2;
    const int n_sB = n_sA + 1 == RING ? 0 : n_sA + 1;
    const int n_s3 = n_sA + 3 >= RING ? n_sA + 3 - RING : n_sA + 3, n_s4 = n_sA + 4 >= RING ? n_sA + 4 - RING : n_sA + 4;
    unsigned n_ya = sbase + (unsigned)n_sA * T2_BYTES, n_xa = sbase + (unsigned)n_sB * T2_BYTES;
    unsigned n_dX = lds0 + (unsigned)n_s3 * T2_BYTES, n_dY = lds0 + (unsigned)n_s4 * T2_BYTES;
    const bf16* n_qX = ROWS ? nxtX : t + 2 < nt ? qX + stepX : qX;
    const bf16* n_qY = ROWS ? nxtY : t + 3 < nt ? qY + stepY : qY;
    asm volatile("" : "+s"(n_sA), "+s"(n_ya), "+s"(n_xa), "+s"(n_dX), "+s"(n_dY), "+s"(n_qX), "+s"(n_qY));
    __builtin_amdgcn_sched_barrier(0);
    if (!leader) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // follower: its pieces of the next step must be in before the leader's L0
    PP_BAR();
    mfma_half(1);
    __builtin_amdgcn_sched_barrier(0);
    if (ROWS) {                                        // the next step's cursors: X of step t + 3 (block bn), dY of step t + 4 (block bnew)
      asm volatile("" : "+s"(bnew));
      nxtX = rowsX(bn);
      nxtY = rowsY(bnew);
      bn = bnew;
      asm volatile("" : "+s"(nxtX), "+s"(nxtY), "+s"(bn));
      __builtin_amdgcn_sched_barrier(0);
    }
    if (leader) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    PP_BAR();
    sA = n_sA; ya = n_ya; xa = n_xa; dXs = n_dX; dYs = n_dY; qX = n_qX; qY = n_qY;
  }
  if (leader) PP_BAR();                                // pairs with the barrier behind the follower's last MFMA half
#undef PP_BAR
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the cursors' last (unused) pieces
  float* ptile = DET ? part + ((int64_t)split * (ntn * ntk) + tile) * 65536 : nullptr;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kl = wk * 64 + j * 32 + (lane & 31);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int nl = wn * 128 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (DET) ptile[nl * 256 + kl] = acc[i][j][e];
        else atomicAdd(dW + (n0 + nl) * K + k0 + kl, acc[i][j][e]);
      }
    }
  if (do_bias) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float s2 = csum[i] + __shfl_xor(csum[i], 32, 64);
      if (lane < 32) {
        const int64_t n = n0 + wn * 128 + i * 32 + lane;
        if (DET) pbias[(((int64_t)split * ntk + tk) * 4 + wk) * N + n] = s2;
        else atomicAdd(dbias + n, s2);
      }
    }
  }
}

// (Measured and not kept, round 4: the same kernel on v_mfma_f32_16x16x32_bf16 -- the shape the chip is said to hold a higher clock on --
// with swapped operands and a patch epilogue whose atomics cover 256 contiguous bytes: 2-3 % SLOWER at all six shapes of the step
// (1.08 / 1.11 / 1.14 against 1.10 / 1.14 / 1.18 PFLOP/s at (N, K) = (768, 768) / (2304, 768) / (768, 2304)); twice the MFMA
// instructions for the same fragment traffic.  The source is kept under tools/lab/gemm_bf16_tn256q_16x16x32.hip.txt.)
// ordered reduction of the deterministic dW path: dW[n][k] += sum_s part[s][tile(n,k)][n%256][k%256] (s ascending), and
// dbias[n] += sum over (s, tk, wk) ascending of pbias.  One thread per 4 consecutive k.
__global__ __launch_bounds__(256) void tn256_reduce_kernel(const float* __restrict__ part, const float* __restrict__ pbias,
                                                            float* __restrict__ dW, float* __restrict__ dbias, int64_t N, int64_t K,
                                                            int ntk, int ntiles, int splits) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nq = N * K / 4;
  if (q < nq) {
    const int64_t n = (q * 4) / K, k = (q * 4) % K;
    const int64_t tile = (n >> 8) * ntk + (k >> 8);
    const float* src = part + tile * 65536 + (n & 255) * 256 + (k & 255);
    f32x4 s = *reinterpret_cast<const f32x4*>(src);
    for (int sp = 1; sp < splits; ++sp) s += *reinterpret_cast<const f32x4*>(src + (int64_t)sp * ntiles * 65536);
    f32x4* dst = reinterpret_cast<f32x4*>(dW + n * K + k);
    *dst = *dst + s;
  }
  if (dbias && q < N) {
    float s = 0.f;
    for (int i = 0; i < splits * ntk * 4; ++i) s += pbias[(int64_t)i * N + q];
    dbias[q] += s;
  }
}

// write-only: zeros into `cpr` 16-byte chunks per row of the listed 256-row panels
__global__ __launch_bounds__(256) void zero_panels_kernel(bf16* __restrict__ C, int64_t ldc, int cpr, const int* __restrict__ panels,
                                                          const int* __restrict__ count) {
  const int n = *count;
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    bf16* const base = C + (int64_t)panels[i] * B2 * ldc;
    for (int idx = threadIdx.x; idx < B2 * cpr; idx += 256) {
      const int r = idx / cpr, c = idx - r * cpr;
      *reinterpret_cast<u32x4*>(base + (int64_t)r * ldc + c * 8) = u32x4{0u, 0u, 0u, 0u};
    }
  }
}

}  // namespace

// Scheduler slot of (current device, stream); nullptr when the table is full or the symbol cannot be resolved.
// g_tile_sched is a __device__ array: every device has its own copy at its own address.
static TileSched* tile_sched_for(hipStream_t stream) {
  struct PerDevice { TileSched* base = nullptr; bool tried = false; std::unordered_map<hipStream_t, int> slot; };
  static std::mutex mu;
  static PerDevice table[MEANT_MAX_DEVICES];
  const int dev = meant_current_device();
  if (dev < 0) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  PerDevice& pd = table[dev];
  if (!pd.tried) {
    pd.tried = true;
    if (hipGetSymbolAddress((void**)&pd.base, HIP_SYMBOL(g_tile_sched)) != hipSuccess) pd.base = nullptr;
  }
  if (!pd.base) return nullptr;
  auto it = pd.slot.find(stream);
  if (it != pd.slot.end()) return pd.base + it->second;
  if ((int)pd.slot.size() >= N_SCHED_SLOTS) return nullptr;
  const int idx = (int)pd.slot.size();
  pd.slot.emplace(stream, idx);
  return pd.base + idx;
}

// diagnostics for the tests: tiles that changed XCD in all streaming launches of the current device so far (synchronises)
extern "C" int64_t meant_debug_nt_steals(void) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  static TileSched host[N_SCHED_SLOTS];
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_tile_sched), sizeof(host)) != hipSuccess) return -1;
  int64_t n = 0;
  for (int i = 0; i < N_SCHED_SLOTS; ++i) n += host[i].steals;
  return n;
}

// ---- "the MFMA kernels can take these operands" (global_load_lds moves 16-byte pieces): what the entry points of api.hip ask before they
// choose between these kernels and the exact f32 engine, and what the launchers below require.  K % 64 != 0 runs on the K-tail forms
// of the one-tile NT kernels.
static bool nt_k_ok(int64_t K) { return K >= 8 && K % 8 == 0; }
static bool rows16(const void* p, int64_t ldp, const void* q, int64_t ldq) {
  return (ldp % 8) == 0 && (ldq % 8) == 0 && meant_aligned16(p) && meant_aligned16(q);
}
bool gemm_bf16_nt_ok(const void* A, int64_t lda, const void* B, int64_t ldb, int64_t K) { return nt_k_ok(K) && rows16(A, lda, B, ldb); }
bool gemm_bf16_tn_ok(const void* dY, int64_t lddy, const void* X, int64_t ldx, int64_t N, int64_t K) {
  return N >= 8 && K >= 8 && rows16(dY, lddy, X, ldx);
}

// ---- which kernel a bf16 NT GEMM takes ---------------------------------------------------------------------------------------------
// nt_plan is the one statement of the rule.  It is pure -- no launch, no route counter, no error; options through meant_opt, the
// compute-unit count an argument -- so the launcher, gemm_bf16_nt_streams and meant_debug_gemm_route read the same decision.
enum NtKind { NT128, NT256, NT256S };                  // 128 x 128 one-tile, 256 x 256 one-tile, 256 x 256 streaming (ping-pong)
struct NtPlan {
  NtKind kind;
  bool ktail;                                          // K % 64 != 0: the K-tail forms of the two one-tile kernels; never the streaming, split or overlap routes
  bool overlap;                                        // NT256S over a ragged M: the last row tile ends at row M
  int64_t split_rows;                                  // != 0: rows [0, split_rows) and the < 256 rows behind them are planned and launched on their own
  int64_t ntm, ntn;                                    // tiles of the kind's size along M and N
  int grid, rotP;                                      // NT256S: workgroups; rotary panel walk (see the kernel's `origin`)
};

static int64_t nt_ldc_h(const GemmBf16Args& a) { return (a.epilogue & GEMM_EPI_F32_OUT) ? 2 * a.ldc : a.ldc; }   // C's row stride in 2-byte units

static NtPlan nt_plan(const GemmBf16Args& a, int ncus) {
  NtPlan p{};
  p.ktail = a.K % BK != 0;
  // big tall problems: 256 x 256 tiles (half the operand bytes per FLOP) -- once there are enough of them to occupy at least
  // half the CUs (the temporal encoder's 1536^2 Linears make 36: four times as many 128 x 128 tiles finish in a third of the time)
  const bool big = a.M >= 1024 && a.N % 256 == 0 && ceil_div(a.M, B2) * (a.N / B2) * 2 >= ncus;
  p.kind = big ? NT256 : NT128;
  p.ntm = ceil_div(a.M, big ? B2 : BM); p.ntn = ceil_div(a.N, big ? B2 : BN);
  // the streaming kernel (ping-pong form: the two waves of a SIMD alternate between MFMA and load halves) needs four K-steps;
  // shorter K goes to the one-tile kernel.  Option nt_stream = 0 forces the one-tile-per-workgroup kernel (A/B measurements)
  const bool can_stream = big && meant_opt(MEANT_OPT_NT_STREAM) != 0 && !p.ktail && a.K >= 4 * BK && (a.ldc & 7) == 0 && (!a.residual || (a.ldr & 7) == 0);
  if (can_stream && a.M % B2 != 0) {
    // Ragged M, option nt_ragged = 1 (default): the streaming kernel takes all of it; its last row tile is moved up so that it
    // ENDS at row M and recomputes up to 255 rows of its neighbour.  Every element of C is a function of its own row of A
    // and column of W with a fixed K order, so both tiles store identical bits (no cost in the K-loop, no second launch:
    // the 32 trailing rows of the TimeSformer's 75 296 tokens cost 12 extra launches of 13-97 us per layer as a split).
    // Needs an out-of-place epilogue: a residual (or A) that aliases C would be read after the neighbour's store.
    const auto overlaps = [](const void* x, int64_t ldx, const void* y, int64_t ldy, int64_t rows) {
      const char *x0 = (const char*)x, *y0 = (const char*)y;
      return x && y && x0 < y0 + rows * ldy * 2 && y0 < x0 + rows * ldx * 2;
    };
    const int64_t ldc_h = nt_ldc_h(a);
    p.overlap = meant_opt(MEANT_OPT_NT_RAGGED) != 0 && !overlaps(a.C, ldc_h, a.residual, a.ldr, a.M) && !overlaps(a.C, ldc_h, a.sub, a.ldsub, a.M) &&
                !overlaps(a.C, ldc_h, a.A, a.lda, a.M) && (!a.preact || !overlaps(a.preact, a.ldc, a.A, a.lda, a.M));
    // nt_ragged = 0 (or aliasing operands): the streaming kernel takes the first floor(M / 256) * 256 rows, the remaining < 256 rows go
    // to the 128 x 128 kernel as a second launch (row-local epilogues only: the rotary epilogue indexes its tables by the
    // absolute row, so it splits only where the boundary is a multiple of the sequence length; otherwise all of it stays one-tile).
    const int64_t m_full = (a.M / B2) * B2;
    if (!p.overlap && (!a.rot_qa || m_full % a.rot_S == 0)) p.split_rows = m_full;
  }
  if (can_stream && (a.M % B2 == 0 || p.overlap)) p.kind = NT256S;
  if (p.kind != NT256S) return p;
  int ncu = ncus & ~7;
  const int cap = meant_opt(MEANT_OPT_NT_GRID_CAP) & ~7;       // tests: fewer workgroups => more tiles each, dry XCDs steal
  if (cap >= 8 && cap < ncu) ncu = cap;
  p.grid = (int)(p.ntm * p.ntn < ncu ? ((p.ntm * p.ntn + 7) / 8) * 8 : ncu);
  // rotary mode: panels of one position range after the other (see the kernel's `origin`)
  if (a.rot_qa && a.rot_S % B2 == 0 && a.rot_S / B2 > 1 && a.rot_S / B2 < 256 && a.M % B2 == 0 && p.ntm % (a.rot_S / B2) == 0) p.rotP = (int)(a.rot_S / B2);
  return p;
}

// the streaming kernel over whole 256-row panels: the only route a panel list is legal on, and the one the by-id forward must match
static bool nt_streams(const NtPlan& p) { return p.kind == NT256S && !p.overlap && !p.split_rows; }
bool gemm_bf16_nt_streams(const GemmBf16Args& a) { return nt_streams(nt_plan(a, meant_num_cus())); }

// One launch as its plans spell it: the route counters in hit order through `hit`, the kernel launches through `leaf(args, plan)` -- once,
// or for the head and the tail of a split, which are planned again.  The launcher counts and launches with it; meant_debug_gemm_route
// names the counters and launches nothing, so the order is stated here alone.
template <typename Hit, typename Leaf>
static int nt_walk(const GemmBf16Args& a, int ncus, Hit&& hit, Leaf&& leaf) {
  const NtPlan p = nt_plan(a, ncus);
  if (a.rot_qa) hit(ROUTE_NT_ROT);
  MEANT_REQUIRE(p.ntm * p.ntn < 2147483647LL, MEANT_ERR_UNSUPPORTED, "gemm_bf16_nt: grid too large");
  if (!p.split_rows) {
    if (p.overlap) hit(ROUTE_NT_OVERLAP);
    hit(p.kind == NT256S ? (a.rot_qa ? ROUTE_NT256S_ROT : ROUTE_NT256S) : p.kind == NT256 ? (p.ktail ? ROUTE_NT256K : ROUTE_NT256) : (p.ktail ? ROUTE_NT128K : ROUTE_NT128));
    return leaf(a, p);
  }
  const int64_t m_full = p.split_rows;
  GemmBf16Args head = a, tail = a;
  head.M = m_full;
  tail.M = a.M - m_full;
  tail.A = a.A + m_full * a.lda;
  tail.C = a.C + m_full * nt_ldc_h(a);
  if (a.residual) tail.residual = a.residual + m_full * a.ldr;
  if (a.preact) tail.preact = a.preact + m_full * a.ldc;
  if (a.row_scale) tail.row_scale = a.row_scale + m_full;
  if (a.sub) { tail.sub = a.sub + m_full * a.ldsub; tail.sub_coef = a.sub_coef + m_full; }
  MEANT_REQUIRE(!a.bres || m_full % a.bres_rows == 0, MEANT_ERR_UNSUPPORTED, "gemm_bf16_nt: broadcast residual across the head / tail split");
  if (a.bres) tail.bres = a.bres + (m_full / a.bres_rows) * a.N;
  hit(ROUTE_NT_SPLIT);
  const int rc = nt_walk(head, ncus, hit, leaf);
  return rc ? rc : nt_walk(tail, ncus, hit, leaf);
}

// zero the `cols` columns at C of the 256-row panels panels[0 .. *count) (device memory): the k | v rows nobody computed
int zero_panels_launch(bf16* C, int64_t ldc, int64_t cols, const int* panels, const int* count, int64_t npan, hipStream_t stream) {
  MEANT_REQUIRE(C && panels && count && cols % 8 == 0 && (ldc & 7) == 0 && meant_aligned16(C) && cols < (1 << 20), MEANT_ERR_ARG, "zero_panels: bad argument");
  if (npan <= 0) return MEANT_OK;
  hipLaunchKernelGGL(zero_panels_kernel, dim3((unsigned)(npan < 2048 ? npan : 2048)), dim3(256), 0, stream, C, ldc, (int)(cols / 8), panels, count);
  MEANT_LAUNCH_CHECK("zero_panels");
  return MEANT_OK;
}

int gemm_bf16_nt_launch(const GemmBf16Args& a, hipStream_t stream) {
  MEANT_REQUIRE(a.A && a.B && a.C, MEANT_ERR_ARG, "gemm_bf16_nt: null pointer");
  MEANT_REQUIRE(!a.rot_qa || (a.rot_D > 0 && a.col0 >= 0 && a.col0 % a.rot_D == 0 && a.N % a.rot_D == 0 && a.col0 + a.N <= 3 * (int64_t)a.rot_D &&
                              a.rot_Dh % 8 == 0 && a.rot_R % 8 == 0 && (a.ldc & 7) == 0 && a.rot_D % a.rot_Dh == 0 && a.rot_S > 0),
                MEANT_ERR_ARG, "gemm_bf16_nt: rotary epilogue needs whole q / k / v sections of H*Dh columns, Dh %% 8 == 0, rot_dim %% 8 == 0");
  MEANT_REQUIRE(!a.panel_list || (a.rot_qa && a.panel_count && gemm_bf16_nt_streams(a)), MEANT_ERR_UNSUPPORTED,
                "gemm_bf16_nt: a panel list needs the rotary epilogue on the streaming kernel");
  MEANT_REQUIRE(nt_k_ok(a.K), MEANT_ERR_UNSUPPORTED, "gemm_bf16_nt: K=%lld must be a multiple of 8 (use the fp32 tier otherwise)", (long long)a.K);
  MEANT_REQUIRE(gemm_bf16_nt_ok(a.A, a.lda, a.B, a.ldb, a.K), MEANT_ERR_ARG,
                "gemm_bf16_nt: operands must be 16-byte aligned with row strides that are multiples of 8");
  const bool ext = a.row_scale || a.sub || a.bres;
  const bool act = (a.epilogue & (MEANT_EPI_GELU | MEANT_EPI_SIGMOID)) != 0;
  const bool f32out = (a.epilogue & GEMM_EPI_F32_OUT) != 0;
  MEANT_REQUIRE(!f32out || (!a.rot_qa && !ext && !a.residual && !a.preact && !act && !a.panel_list), MEANT_ERR_UNSUPPORTED,
                "gemm_bf16_nt: float output with rotary / activation / residual / preact / extended operands");
  MEANT_REQUIRE(!f32out || meant_aligned16(a.C), MEANT_ERR_ARG, "gemm_bf16_nt: float output must be 16-byte aligned");
  MEANT_REQUIRE(!a.bres || (a.bres_rows > 0 && (a.N & 7) == 0 && meant_aligned16(a.bres)), MEANT_ERR_ARG, "gemm_bf16_nt: bad broadcast residual");
  MEANT_REQUIRE(!ext || (!a.rot_qa && !(a.epilogue & MEANT_EPI_SIGMOID)), MEANT_ERR_UNSUPPORTED, "gemm_bf16_nt: extended epilogue with rotary / sigmoid");
  MEANT_REQUIRE(!a.rot_qa || (!a.residual && !a.preact && !act), MEANT_ERR_UNSUPPORTED, "gemm_bf16_nt: rotary epilogue with residual / activation / preact");
  MEANT_REQUIRE(!a.sub || (a.sub_coef && (a.ldsub & 7) == 0 && meant_aligned16(a.sub)), MEANT_ERR_ARG, "gemm_bf16_nt: bad sub operand");
  // one launch: `g` is `a`, or the head or the tail of its split (the same epilogue, so the checks above and ext / act / f32out hold for it)
  return nt_walk(a, meant_num_cus(), meant_route_hit, [&](const GemmBf16Args& g, const NtPlan& p) -> int {
    const auto one_tile = [&](auto kernel, int threads, size_t lds, const char* name) -> int {
      MEANT_RAISE_LDS(kernel, lds);
      hipLaunchKernelGGL(kernel, dim3((unsigned)(p.ntm * p.ntn)), dim3(threads), lds, stream, g, (int)p.ntm, (int)p.ntn);
      MEANT_LAUNCH_CHECK(name);
      return MEANT_OK;
    };
    const size_t lds128 = 128 * (128 + 4) * sizeof(float);   // 67584 B: covers the 64 KiB of staging buffers too
    if (p.kind == NT128)
      return p.ktail ? one_tile(gemm_bf16_nt_kernel<true>, 256, lds128, "gemm_bf16_nt_ktail") : one_tile(gemm_bf16_nt_kernel<false>, 256, lds128, "gemm_bf16_nt");
    if (p.kind == NT256)
      return p.ktail ? one_tile(gemm_bf16_nt256_kernel<true>, 512, 4 * T2_BYTES, "gemm_bf16_nt256")
                     : one_tile(gemm_bf16_nt256_kernel<false>, 512, 4 * T2_BYTES, "gemm_bf16_nt256");
    // Tile counters: one slot per (device, stream).  Launches on one stream execute in order and a launch leaves its
    // slot zeroed (last workgroup out), so a slot is never shared by two launches in flight -- by construction, not by
    // distance.  A stream beyond the table's capacity gets the fixed walk (sched = nullptr).  Option nt_dynamic = 0 forces it.
    const int dynmode = meant_opt(MEANT_OPT_NT_DYNAMIC);
    TileSched* sched = (dynmode != 0 && p.grid <= 512) ? tile_sched_for(stream) : nullptr;
    const auto streaming = [&](auto mode) -> int {
      MEANT_RAISE_LDS((gemm_bf16_nt256p_kernel<mode.value>), RING * T2_BYTES);
      hipLaunchKernelGGL((gemm_bf16_nt256p_kernel<mode.value>), dim3((unsigned)p.grid), dim3(512), RING * T2_BYTES, stream, g, (int)p.ntm, (int)p.ntn,
                         sched, dynmode | (p.rotP << 16));
      MEANT_LAUNCH_CHECK("gemm_bf16_nt256");
      return MEANT_OK;
    };
    // the epilogue's options as a template parameter (see nt256_wave_epilogue): the combinations the models run get straight-line
    // code, anything else the generic instantiation with run-time flags
    using std::integral_constant;
    if (g.rot_qa) return streaming(integral_constant<int, NTE_ROT>{});
    if (f32out) return streaming(integral_constant<int, NTE_GENERIC>{});
    if (ext) return streaming(integral_constant<int, NTE_EXT>{});
    if (!g.residual && !g.preact && !act) return streaming(integral_constant<int, NTE_PLAIN>{});
    if (g.residual && !g.preact && !act) return streaming(integral_constant<int, NTE_RES>{});
    if (!g.residual && g.preact && (g.epilogue & MEANT_EPI_GELU) && !(g.epilogue & MEANT_EPI_SIGMOID)) return streaming(integral_constant<int, NTE_GELU_PRE>{});
    return streaming(integral_constant<int, NTE_GENERIC>{});
  });
}

static int tn_tail(const bf16* dY, int64_t lddy, const bf16* X, int64_t ldx, float* dW, float* dbias, int64_t M, int64_t N, int64_t K,
                   hipStream_t stream) {
  // fewer than 64 trailing token rows: exact generic kernel, accumulating into the same dW / dbias
  meant_route_hit(ROUTE_TN_TAIL);
  int rc = gemm_f32_launch(f32_rowmajor(true, dY, lddy, X, ldx, dW, K, N, K, M, MEANT_BF16), stream);
  if (rc) return rc;
  if (dbias) return colsum_launch(dY, lddy, dbias, M, N, MEANT_BF16, 1, stream);
  return MEANT_OK;
}

// ---- which kernel a dW GEMM takes, and its launch geometry: read by the workspace query, both launchers and meant_debug_gemm_route.
// Pure, as nt_plan is.  `listed`: the caller has a list of live 64-row blocks the 256 x 256 kernel may reduce over.
enum TnKind { TN128 = ROUTE_TN128, TN256 = ROUTE_TN256, TN256_DET = ROUTE_TN256_DET, TN256_ROWS = ROUTE_TN256_ROWS };   // a kind is its route counter
struct TnPlan {
  TnKind kind;
  int64_t tail_rows, rows;                             // M % 64 trailing token rows (the exact generic kernel) and the rows in front of them (0: no MFMA launch)
  int64_t ntn, ntk;                                    // tiles of the kind's size along N and K
  int64_t splits, rows_per;                            // the token axis in `splits` parts of rows_per rows (a multiple of 64)
  size_t ws_bytes;                                     // TN256_DET: the splits' partial sums and partial bias sums
};

static TnPlan tn_plan(int64_t M, int64_t N, int64_t K, bool listed, int ncus) {
  const bool det = meant_opt(MEANT_OPT_DETERMINISTIC) != 0;
  TnPlan p{};
  p.tail_rows = M % TN_BKM;
  p.rows = M = M - p.tail_rows;
  const bool t256 = N % 256 == 0 && K % 256 == 0 && M >= 4096;
  // the list form has no deterministic variant and no tail; whatever it does not take runs the full reduction
  p.kind = !t256 ? TN128 : det ? TN256_DET : listed && p.tail_rows == 0 && M / TN_BKM < (1LL << 30) ? TN256_ROWS : TN256;
  if (M == 0) return p;
  p.ntn = ceil_div(N, t256 ? 256 : 128); p.ntk = ceil_div(K, t256 ? 256 : 128);
  // 256 x 256, one resident block per CU: size the launch to whole rounds of the CU count (a lone block in an extra
  // round would cost a full round of time) -- one round when every block still gets >= 32 tiles of 64 rows.
  // 128 x 128: split the token axis so that the launch has >= ~4 blocks per CU
  p.splits = t256 ? (ncus > 0 ? ncus : 256) / (p.ntn * p.ntk) : ceil_div(1024, p.ntn * p.ntk);
  const int64_t max_splits = ceil_div(M, t256 ? 32 * TN_BKM : 256);
  if (p.splits > max_splits) p.splits = max_splits;
  if (p.splits < 1 || (det && !t256)) p.splits = 1;    // 128 x 128, deterministic: every output element has exactly one writer
  p.rows_per = ceil_div(ceil_div(M, p.splits), TN_BKM) * TN_BKM;   // each split is a multiple of 64 rows
  p.splits = ceil_div(M, p.rows_per);
  if (p.kind == TN256_DET) p.ws_bytes = (size_t)(p.splits * N * K + p.splits * p.ntk * 4 * N) * sizeof(float);
  return p;
}

size_t gemm_bf16_tn_ws(int64_t M, int64_t N, int64_t K) {
  return meant_opt(MEANT_OPT_DETERMINISTIC) ? tn_plan(M, N, K, false, meant_num_cus()).ws_bytes : 0;   // (no device look-up without the option)
}

// dW over all token rows (rows == nullptr) or over a list of 64-row blocks of the token axis (gemm_bf16_tn256p_kernel<false, true>): dW += sum
// over the listed blocks; every row of dY outside them is zero by the caller's word, so whatever the list form does not take -- the
// deterministic option, shapes the 256 x 256 kernel does not serve -- runs the full reduction instead and adds the same sums.
int gemm_bf16_tn_rows_launch(const bf16* dY, int64_t lddy, const bf16* X, int64_t ldx, float* dW, float* dbias, const int* rows,
                             const int* rows_count, int64_t M, int64_t N, int64_t K, void* ws, size_t ws_bytes, hipStream_t stream) {
  MEANT_REQUIRE(rows16(dY, lddy, X, ldx), MEANT_ERR_ARG, "gemm_bf16_tn: operands must be 16-byte aligned with row strides that are multiples of 8");
  MEANT_REQUIRE(gemm_bf16_tn_ok(dY, lddy, X, ldx, N, K), MEANT_ERR_UNSUPPORTED, "gemm_bf16_tn: N and K must be >= 8");
  const TnPlan p = tn_plan(M, N, K, rows && rows_count, meant_num_cus());   // the splits are sized for the full M: a list's count is known on the device only
  if (p.tail_rows) {
    int rc = tn_tail(dY + p.rows * lddy, lddy, X + p.rows * ldx, ldx, dW, dbias, p.tail_rows, N, K, stream);
    if (rc || p.rows == 0) return rc;
  }
  if (p.kind != TN128) {
    float *part = nullptr, *pbias = nullptr;
    if (p.kind == TN256_DET) {
      MEANT_REQUIRE(ws && ws_bytes >= p.ws_bytes && meant_aligned16(ws), MEANT_ERR_WORKSPACE,
                    "linear_bwd_dw (deterministic): workspace of %zu bytes needed (meant_linear_bwd_dw_ws), got %zu", p.ws_bytes, ws_bytes);
      part = (float*)ws;
      pbias = part + p.splits * N * K;
    }
    meant_route_hit(p.kind);
    // the one launch site of the 256 x 256 dW kernel.  Its `rows_per_split` argument is two things: the token rows of a split in the two
    // plain forms; in the list form, where a split's share follows from *rows_count on the device, the NUMBER of splits.
    const int64_t rows_per_or_splits = p.kind == TN256_ROWS ? p.splits : p.rows_per;
    const auto launch = [&](auto det, auto listed, const char* name) -> int {
      MEANT_RAISE_LDS((gemm_bf16_tn256p_kernel<det.value, listed.value>), RING * T2_BYTES);
      hipLaunchKernelGGL((gemm_bf16_tn256p_kernel<det.value, listed.value>), dim3((unsigned)(p.ntn * p.ntk * p.splits)), dim3(512), RING * T2_BYTES, stream,
                         dY, lddy, X, ldx, dW, dbias, p.rows, N, K, (int)p.ntn, (int)p.ntk, rows_per_or_splits, part, pbias,
                         listed.value ? rows : nullptr, listed.value ? rows_count : nullptr);
      MEANT_LAUNCH_CHECK(name);
      return MEANT_OK;
    };
    if (p.kind == TN256_ROWS) return launch(std::false_type{}, std::true_type{}, "gemm_bf16_tn256<rows>");
    if (p.kind == TN256) return launch(std::false_type{}, std::false_type{}, "gemm_bf16_tn256");
    const int rc = launch(std::true_type{}, std::false_type{}, "gemm_bf16_tn256<det>");
    if (rc) return rc;
    hipLaunchKernelGGL(tn256_reduce_kernel, dim3((unsigned)ceil_div(N * K / 4, 256)), dim3(256), 0, stream, part, dbias ? pbias : nullptr, dW, dbias,
                       N, K, (int)p.ntk, (int)(p.ntn * p.ntk), (int)p.splits);
    MEANT_LAUNCH_CHECK("tn256_reduce");
    return MEANT_OK;
  }
  MEANT_RAISE_LDS(gemm_bf16_tn_kernel, 4 * TN_TILE_BYTES);
  meant_route_hit(p.kind);
  hipLaunchKernelGGL(gemm_bf16_tn_kernel, dim3((unsigned)(p.ntn * p.ntk * p.splits)), dim3(256), 4 * TN_TILE_BYTES, stream, dY, lddy, X,
                     ldx, dW, p.rows, N, K, (int)p.ntn, (int)p.ntk, p.rows_per);
  MEANT_LAUNCH_CHECK("gemm_bf16_tn");
  if (dbias) return colsum_launch(dY, lddy, dbias, p.rows, N, MEANT_BF16, 1, stream);
  return MEANT_OK;
}

int gemm_bf16_tn_launch(const bf16* dY, int64_t lddy, const bf16* X, int64_t ldx, float* dW, float* dbias, int64_t M, int64_t N,
                        int64_t K, void* ws, size_t ws_bytes, hipStream_t stream) {
  return gemm_bf16_tn_rows_launch(dY, lddy, X, ldx, dW, dbias, nullptr, nullptr, M, N, K, ws, ws_bytes, stream);
}

// ---- diagnostics: the route counters a launch would hit, in hit order, from the plans above and nothing else (no launch, no device)
extern "C" int meant_debug_gemm_route(const char* op, int64_t M, int64_t N, int64_t K, int facts, int64_t rot_S, int num_cus, void* names,
                                      size_t names_bytes) {
  const bool nt = op && !strcmp(op, "nt"), tn_rows = op && !strcmp(op, "tn_rows");
  MEANT_REQUIRE((nt || tn_rows || (op && !strcmp(op, "tn"))) && M > 0 && N > 0 && K > 0 && rot_S >= 0 && rot_S < (1LL << 31) && names, MEANT_ERR_ARG,
                "debug_gemm_route: op is \"nt\", \"tn\" or \"tn_rows\"; positive shape; 0 <= rot_S < 2^31; a buffer for the names");
  std::string s;
  const auto name = [&s](int route) { (s += s.empty() ? "" : " ") += meant_route_name(route); };
  int rc = 0;
  if (nt) {
    // addresses that are never dereferenced: the rule reads strides, null / non-null and whether an operand's rows overlap C's
    GemmBf16Args a = gemm_bf16_nt_args(nullptr, K, nullptr, nullptr, ceil_div(N, 8) * 8 + ((facts & MEANT_FACT_LDC_OFF8) ? 1 : 0), M, N, K);
    a.ldr = ceil_div(N, 8) * 8 + ((facts & MEANT_FACT_LDR_OFF8) ? 1 : 0);
    a.C = reinterpret_cast<bf16*>(uintptr_t(1) << 40);
    const bf16* const apart = a.C + M * a.ldc;         // the first address behind C's rows
    a.A = (facts & MEANT_FACT_ALIAS_C) && !(facts & MEANT_FACT_RESIDUAL) ? a.C : apart;
    if (facts & MEANT_FACT_RESIDUAL) a.residual = (facts & MEANT_FACT_ALIAS_C) ? a.C : apart;
    if (rot_S > 0) { a.rot_qa = reinterpret_cast<const float*>(apart); a.rot_S = (int)rot_S; }
    rc = nt_walk(a, num_cus, name, [](const GemmBf16Args&, const NtPlan&) { return (int)MEANT_OK; });
    if (!rc) rc = nt_streams(nt_plan(a, num_cus)) ? 1 : 0;
  } else {
    const TnPlan p = tn_plan(M, N, K, tn_rows, num_cus);
    if (p.tail_rows) { name(ROUTE_TN_TAIL); name(ROUTE_GEMM_F32); }    // the exact engine counts its own launch
    if (p.rows) name(p.kind);
  }
  MEANT_REQUIRE(s.size() < names_bytes, MEANT_ERR_WORKSPACE, "debug_gemm_route: %zu bytes needed for the names, got %zu", s.size() + 1, names_bytes);
  memcpy(names, s.c_str(), s.size() + 1);
  return rc;
}
