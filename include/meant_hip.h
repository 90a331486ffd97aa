/*
 * meant_hip.h  --  C ABI of libmeant_hip.so, the MI355X (gfx950 / CDNA4) implementation of the
 * MEANT multimodal-encoder forward/backward hot path.
 *
 * The reference (biirving/meant) is pure Python; the native code on its hot path is what PyTorch
 * dispatches to (ATen/cuBLAS kernels, flash-attn).  Each entry point below replaces the native
 * work behind one reference call site (cited as file:line, relative to the reference root).  The host side
 * (the Python modules under meant_amd/) binds these with ctypes and keeps the reference's nn.Module surface.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer owned by the caller (PyTorch);
 *     the library never allocates, frees or retains device memory;
 *   - dtype: MEANT_F32 (0) or MEANT_BF16 (1) is the storage type of activations ("act");
 *     statistics, softmax, accumulators, parameter gradients and norm gains are always float;
 *   - tensors are dense row-major in the documented shape; "ld" arguments are row strides in
 *     elements where a tensor is a column slice of a wider buffer;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); no call synchronises;
 *   - return value: 0 on success, a negative meant_status otherwise; meant_last_error() returns a
 *     thread-local message.  Nothing aborts or throws across the boundary.
 */
#ifndef MEANT_HIP_H
#define MEANT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum meant_dtype { MEANT_F32 = 0, MEANT_BF16 = 1 };
/* storage-only types of raw inputs (meant_patchify_raw): the reference keeps its price graphs as float64 .npy
 * (in_loop_train.py:48,589); uint8 is what a rendered chart is before anyone converts it */
enum meant_raw_dtype { MEANT_RAW_F32 = 0, MEANT_RAW_BF16 = 1, MEANT_RAW_F64 = 2, MEANT_RAW_U8 = 3 };
/* storage types of an attention mask as meant_mlm_mask reads it (the models take float or int64 masks; U8 is also torch.bool) */
enum meant_mask_dtype { MEANT_MASK_F32 = 0, MEANT_MASK_BF16 = 1, MEANT_MASK_I64 = 2, MEANT_MASK_U8 = 3, MEANT_MASK_I32 = 4 };

enum meant_status {
  MEANT_OK = 0,
  MEANT_ERR_ARG = -1,         /* bad shape / null pointer / misalignment */
  MEANT_ERR_UNSUPPORTED = -2, /* shape or dtype the kernels do not cover  */
  MEANT_ERR_LAUNCH = -3,      /* hipGetLastError() after a launch         */
  MEANT_ERR_WORKSPACE = -4    /* workspace too small                      */
};

/* epilogue flags of meant_linear_fwd */
enum meant_epilogue {
  MEANT_EPI_NONE = 0,
  MEANT_EPI_GELU = 1,     /* y = gelu_erf(x W^T + b); optional pre-activation copy */
  MEANT_EPI_RESIDUAL = 2, /* y = x W^T + b + residual                             */
  MEANT_EPI_SIGMOID = 4   /* y = sigmoid(x W^T + b)                               */
};

int meant_version(void);
const char* meant_last_error(void);
/* number of compute units of the current device (for sizing partial-sum workspaces) */
int meant_num_cus(void);

/* ---- process-wide switches and diagnostics --------------------------------------------------------
 * The library keeps no mutable global state except: a per-device table filled on first use (CU count, raised LDS
 * limits, the tile counters of the streaming GEMM -- one slot per (device, stream)), these options, and the
 * route counters below.  All of it is safe to use from several host threads and with several devices in one
 * process (the reference's nn.DataParallel, pretrain_mlm.py:329): every call acts on the calling thread's current
 * device, whose memory all pointer arguments must belong to.
 * Options (initial value from the environment variable MEANT_<NAME IN CAPITALS>):
 *   "deterministic"    0|1   parameter gradients (dW, dbias, the norm gains, the embedding table at any d % 8 == 0) by ordered
 *                            reductions instead of float atomics: two runs on the same inputs are bit-identical;
 *                            meant_linear_bwd_dw then needs its workspace
 *   "nt_stream"        1|0   streaming 256x256 NT GEMM / one tile per workgroup           (A/B measurements)
 *   "nt_dynamic"       1|0|3 streaming GEMM draws tiles from per-XCD counters / fixed walk (A/B measurements) /
 *                            only XCD 0 uses its own counter, all other tiles go through the steal path (tests)
 *   "nt_grid_cap"      0|n   cap the streaming GEMM's grid at n workgroups (tests: many tiles per workgroup, steals)
 *   "nt_ragged"        1|0   M not a multiple of 256: the streaming GEMM's last row tile is moved up to end at row M (it
 *                            recomputes rows of its neighbour bit-identically) / streaming head + 128 x 128 tail launch
 *                            (also what operands that alias the output fall back to)
 *   "attn_short"       1|0   sequences of <= 16 tokens run on the one-wave-per-(group, head) kernels / on the tiled ones
 *   "attn_bwd1"        1|0   attention backward, head dim 64, S <= 256 or causal S <= 512: one pass (scores and dP computed once,
 *                            dS through LDS into the dQ product; persistent workgroups) / the dQ pass followed by the dK, dV pass
 *   "temporal_long"    0|1   the temporal attention core runs its long-lag kernels for L > 64 only / at every lag (a measuring
 *                            switch: tools/probe_temporal_lag.py times both kernel families at L <= 64 with it)
 *   "kv_skip"          3|0   bits: which GEMMs around a key-masked bf16 attention (ops: the fused q|k|v projection) leave out the rows of
 *                            padded key blocks (meant_kv_live_rows).  1: the k|v columns of the projection's weight gradient reduce
 *                            over the live 64-row blocks only (meant_linear_bwd_dw_rows); 2: the forward projection computes k|v for
 *                            the live 256-row panels only (meant_qkv_proj_fwd_live); 0: every GEMM takes all rows
 *   "qkv_by_id"        1|0|2 the first text layer's backward (q|k|v projection, RMSNorm, embedding) once per vocabulary id
 *                            (meant_qkv_embed_bwd_by_id) instead of once per token: where the caller's rule says the tokens outnumber
 *                            the ids enough / never / wherever the route applies.  Read by the callers; the entry point itself always runs
 *   "qkv_fwd_by_id"    1|0|2 the same node's forward (RMSNorm and q|k|v projection on the table's rows, then a gather over the sorted
 *                            ids: meant_qkv_embed_fwd_by_id) where the caller's rule says the tokens outnumber the ids enough / never /
 *                            wherever meant_qkv_embed_fwd_by_id_ok holds.  Read by the callers
 *   "nt_pp"            1     read-only: the streaming GEMM runs in its ping-pong form (setting any other value fails with
 *                            MEANT_ERR_UNSUPPORTED: the lock-step kernel was removed); not read from the environment
 */
int meant_set_option(const char* name, int value);
int meant_get_option(const char* name, int* value);
/* how many launches took a given kernel route since the last reset ("nt128", "nt256", "nt256s", "nt256s_rot",
 * "nt128k", "nt256k" (the K-tail forms of the 128 x 128 and 256 x 256 one-tile kernels: K % 64 != 0),
 * "nt_split", "nt_overlap", "tn128", "tn256", "tn256_det", "tn256_rows" (meant_linear_bwd_dw_rows on its list), "tn_tail", "gemm_f32", "attn_fwd", "attn_fwd_d128",
 * "attn_fwd_d96", "attn_bwd" (the two-pass form), "attn_bwd1" (the single-pass form), "attn_bwd_d128", "attn_bwd_d96",
 * "attn_generic", "attn_cls", "attn_cls_split", "rows_elem", "attn_short", "attn_fwd_d160" ... "attn_bwd_d256", "temporal_long" (the temporal attention
 * core's long-lag kernels, forward and backward each count one), "emb_seg" (meant_embedding_bwd_seg), "sort_ids" (meant_sort_ids), "select_rows" (meant_select_rows),
 * "rotary_qk" (every meant_rotary_qk launch), "rotary_pairs" (those of its pair-by-pair kernel: Dh % 8 != 0 or an unaligned base)
 * "nt_rot" (every bf16 NT GEMM launched with the rotary epilogue, on top of the nt* route it takes), "metrics_rows" /
 * "metrics_wave" / "metrics_labels" (meant_metrics_update by form, every meant_metrics_update_labels launch), "score_capture"
 * (every meant_score_capture launch), "auroc_rank" (every meant_auroc_rank call with n > 0), "ce_soft_wave" / "ce_soft_block"
 * (meant_ce_probs_soft by form), "vqa_score" (every meant_vqa_score_update launch), "grad_stats" (every meant_grad_stats_f32 call
 * with n > 0), "optim_step" (every meant_optim_step_f32 launch), "qkv_by_id" (every meant_qkv_embed_bwd_by_id call that runs its
 * shared stage), "qkv_fwd_by_id" (every meant_qkv_embed_fwd_by_id call), "ce_hard_wave" / "ce_hard_block" (meant_ce_probs_hard by
 * form), "ce_hard_vocab" (every meant_softmax_ce_hard_fwd launch), "ce_probs" (every meant_ce_probs launch) and "softmax_ce"
 * (every meant_softmax_ce_fwd launch));
 * -1 for an unknown name.  The names label routes, not kernels: "nt256s" / "nt256s_rot" count launches of the streaming
 * GEMM (whichever kernel implements it), "nt_split" the ragged head + tail split.  Tests use it to prove that a shape
 * reaches the kernel it is meant to exercise. */
int64_t meant_route_count(const char* route);
void meant_route_reset(void);
/* tiles the streaming GEMM's workgroups took from another XCD's counter, summed over all launches on the current
 * device so far; synchronises the device (test diagnostics) */
int64_t meant_debug_nt_steals(void);
/* which route counters one bf16 GEMM launch would hit, from the launchers' own classifiers: nothing is launched, no device is
 * needed, the options are read as they are set.  op: "nt" (Linear forward / input gradient, C[M,N] = A[M,K] B[N,K]^T), "tn" (weight
 * gradient dW[N,K] over M token rows) or "tn_rows" (the same over a list of live 64-row blocks).  facts: what the rule reads of
 * an "nt" launch beside its shape, a sum of meant_route_fact (C's / the residual's row stride is no multiple of 8 elements; a
 * residual is given; the residual -- without one, A -- is C itself); 0 < rot_S < 2^31: the rotary epilogue with sequences of rot_S rows.
 * num_cus: the compute-unit count to decide for (meant_num_cus() on a device).  names (char[names_bytes]) receives the counter
 * names in hit order, space-separated, e.g. "nt_overlap nt256s", "nt_split nt256s nt128", "tn_tail gemm_f32 tn256".
 * Returns 1 if an "nt" launch runs the streaming kernel over whole 256-row panels (what a key-padding panel list and the by-id
 * forward need), 0 otherwise, a negative meant_status on a bad argument or a buffer too small. */
enum meant_route_fact { MEANT_FACT_LDC_OFF8 = 1, MEANT_FACT_LDR_OFF8 = 2, MEANT_FACT_RESIDUAL = 4, MEANT_FACT_ALIAS_C = 8 };
int meant_debug_gemm_route(const char* op, int64_t M, int64_t N, int64_t K, int facts, int64_t rot_S, int num_cus, void* names,
                           size_t names_bytes);

/* ---- RMSNorm ---------------------------------------------------- utils/rms_norm.py:40-57
 * y = scale * x * rinv,  rinv = 1 / (||x||_2 / sqrt(d) + eps)   (eps outside the sqrt)
 * x,y: act [rows, d]; scale: float [d]; rinv: float [rows] (saved for backward).
 * Optional fused inverted dropout on y (meant/meant.py:105,107): keep-prob 1-p, mask regenerated
 * in backward from (seed, element index); p == 0 disables it.
 * Any d > 0: d % 8 == 0 and d <= 2048 take the one-row-per-wave and packed kernels (16-byte aligned x, y, scale); every
 * other width a one-row-per-workgroup kernel (16-byte alignment when d % 8 == 0, element alignment otherwise).  The same
 * holds for the backward, the partial forms and LayerNorm below. */
int meant_rmsnorm_fwd(const void* x, const float* scale, void* y, float* rinv, int64_t rows, int64_t d,
                      float eps, float drop_p, uint64_t seed, int dtype, void* stream);
/* dx: act [rows, d]; dscale: float [d] (overwritten); workspace: meant_rmsnorm_bwd_ws(rows, d) bytes.
 * Every parameter gradient of this section (dscale, doffset, dbias_up, dgamma, dbeta) is an ordered sum: no atomics, the same bits
 * on every run.
 * Optional fusions (NULL to disable): dres act [rows, d] is added to dx (the gradient of the residual
 * branch that shares x, meant/meant.py:71,74); gelu_pre act [rows, d]: x was gelu(gelu_pre), and dx is
 * multiplied by gelu'(gelu_pre) so that it is the gradient w.r.t. gelu_pre (meant/meant.py:64). */
size_t meant_rmsnorm_bwd_ws(int64_t rows, int64_t d);
int meant_rmsnorm_bwd(const void* dy, const void* x, const float* scale, const float* rinv, void* dx,
                      float* dscale, int64_t rows, int64_t d, float eps, float drop_p, uint64_t seed,
                      const void* dres, const void* gelu_pre, int dtype, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- RMSNorm, partial / bias forms of the reference class ------- utils/rms_norm.py:44-57 (RMSNorm(d, p, bias))
 * statistics over the first d_part = int(d * p) elements of a row (1 <= d_part <= d), y = scale * x / (rms_part + eps) + offset
 * (offset float [d] or NULL).  No MEANT model constructs these; served by the generic one-row-per-wave kernels (d % 8 == 0,
 * d <= 2048) and the one-row-per-workgroup kernels (any other d > 0). */
int meant_rmsnorm_partial_fwd(const void* x, const float* scale, const float* offset, void* y, float* rinv, int64_t rows,
                              int64_t d, int64_t d_part, float eps, int dtype, void* stream);
int meant_rmsnorm_partial_bwd(const void* dy, const void* x, const float* scale, const float* rinv, void* dx, float* dscale,
                              float* doffset, int64_t rows, int64_t d, int64_t d_part, float eps, int dtype, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---- RMSNorm beside the sequence mean-pool -------- utils/rms_norm.py:40-57 + meant/meant.py:74,120 -> :231
 * The last RMSNorm of the last encoder layer has one consumer left once that layer's final Linear is evaluated on the
 * pooled features (mean_s(h W^T + b + x) = mean_s(h) W^T + b + mean_s(x)): the mean over the group_rows tokens of a
 * sequence.  meant_rmsnorm_fwd_pooled writes that mean to pooled[g, :] (float [rows / group_rows, d]; ordered sums, bit-reproducible):
 *   pool_input == 0: of y = dropout(RMSNorm(x)) -- y is NOT written (pass NULL);
 *   pool_input != 0: of x, the residual operand -- y is written as usual.
 * gelu_input != 0 (with pool_input == 0): x is the PRE-activation h of the Linear + GELU in front of the norm
 * (meant/meant.py:63-64,106-107); gelu(h) is formed on load, so the activation tensor is never stored.  The backward
 * then takes x == NULL and h as gelu_pre.
 * meant_rmsnorm_bwd_pooled is meant_rmsnorm_bwd with dy (dy_pooled != 0) and / or dres (dres_pooled != 0) given as the
 * float [groups, d] gradient of the pooled features: row r receives g[r / group_rows] / group_rows, no [rows, d]
 * broadcast is materialised.  Supported where meant_rmsnorm_pooled_ok(rows, d, group_rows) != 0 (the packed widths,
 * d = 768 among them, and group_rows a multiple of the rows a wave packs); the caller falls back to the unfused ops
 * otherwise. */
int meant_rmsnorm_pooled_ok(int64_t rows, int64_t d, int64_t group_rows);
int meant_rmsnorm_fwd_pooled(const void* x, const float* scale, void* y, float* rinv, float* pooled, int64_t rows,
                             int64_t d, int64_t group_rows, int pool_input, int gelu_input, float eps, float drop_p,
                             uint64_t seed, int dtype, void* stream);
int meant_rmsnorm_bwd_pooled(const void* dy, int dy_pooled, const void* x, const float* scale, const float* rinv,
                             void* dx, float* dscale, int64_t rows, int64_t d, int64_t group_rows, float eps,
                             float drop_p, uint64_t seed, const void* dres, int dres_pooled, const void* gelu_pre,
                             int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- RMSNorm folded into the Linear that consumes it -------- utils/rms_norm.py:40-57 followed by an nn.Linear:
 *                                                               meant/meant.py:61-63 (encode2[0] -> encode2[1] -> GELU), :103-106
 * Linear(RMSNorm(x)) = r (x) (x W'^T) + b with W' = W diag(g) and r[m] = 1 / (||x_m|| / sqrt(d) + eps): the normalisation is
 * a per-row factor in the GEMM epilogue (meant_linear_fwd_rowscale), the gain a column scale of the weight (meant_colscale);
 * the normalised tensor never exists, forward or backward.  bf16 tier, packed widths (meant_rmsnorm_pooled_ok) only.
 *   meant_rmsnorm_stats      r[rows] from one read of x.
 *   meant_rmsnorm_bwd_chain  the backward of the NEXT norm down the layer (the one behind the GELU: meant_rmsnorm_bwd with
 *                            gelu_pre, token-level dy and the stored activation x; or its pooled form: dy_pooled != 0, x NULL),
 *                            which is where the gradient dpre of this Linear's output comes from.  In the same pass it also
 *                            writes dx_scaled = up_rinv[m] * dpre (the operand of both backward GEMMs), kcoef[m] =
 *                            rowdot(dpre, gelu_pre - up_bias) up_rinv^2 / ((1 - up_eps up_rinv) up_d), up_d the width of the folded norm (see meant_linear_bwd_dx_norm)
 *                            and dbias_up += column sums of the unscaled dpre (the Linear's bias gradient).
 *   meant_colscale / _bwd    W' = W diag(g);  dW += dW' diag(g), dg[k] += sum_n dW'[n,k] W[n,k]   (float, [N, K]). */
int meant_rmsnorm_stats(const void* x, float* rinv, int64_t rows, int64_t d, float eps, int dtype, void* stream);
int meant_rmsnorm_bwd_chain(const void* dy, int dy_pooled, const void* x, const float* scale, const float* rinv,
                            void* dx_scaled, float* dscale, int64_t rows, int64_t d, int64_t group_rows, float eps,
                            float drop_p, uint64_t seed, const void* gelu_pre, const float* up_rinv, const float* up_bias,
                            float up_eps, int64_t up_d, float* kcoef, float* dbias_up, int dtype, void* workspace, size_t workspace_bytes,
                            void* stream);
int meant_colscale(const float* w, const float* g, float* out, int64_t N, int64_t K, void* stream);
int meant_colscale_bwd(const float* dwp, const float* w, const float* g, float* dw, float* dg, int64_t N, int64_t K,
                       void* stream);

/* ---- LayerNorm (heads of meant_vision / meant_tweet) ----- meant/meant_vision.py:147
 * stats: float [rows, 2] (mean, rstd). */
int meant_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* stats,
                        int64_t rows, int64_t d, float eps, int dtype, void* stream);
int meant_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* stats, void* dx,
                        float* dgamma, float* dbeta, int64_t rows, int64_t d, int dtype, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- Linear ------------------- nn.Linear call sites meant/meant.py:59-64,101-107,132-136,195,204
 *                                   and q/v/k/multi_mad in meant/attention.py:31-33,57-60 etc.
 * y[M,N] = x[M,K] w[N,K]^T + bias[N]  (+ epilogue).  x,w,y,residual,preact: act dtype; bias float
 * (may be NULL).  ldx/ldy/ldr: row strides.  preact (optional, EPI_GELU) receives x W^T + b.
 * bf16 tier: any K that is a multiple of 8 (with ldx % 8 == 0 and 16-byte aligned x, w) runs on the MFMA kernels: K % 64 == 0 on
 * the streaming / one-tile kernels, any other such K on the K-tail forms of the one-tile kernels (routes "nt128k" / "nt256k"),
 * which read neither operand at or beyond column K of a row.  Everything else takes the exact-f32 engine on bf16 storage; a caller
 * with K % 8 != 0 pads both operands to ceil8(K) with meant_pad_copy2d first. */
int meant_linear_fwd(const void* x, int64_t ldx, const void* w, const float* bias, const void* residual,
                     int64_t ldr, void* y, int64_t ldy, void* preact, int64_t M, int64_t N, int64_t K,
                     int epilogue, int dtype, void* stream);
/* y[M,N] (FLOAT, row stride ldy floats) = x[M,K] w[N,K]^T + bias[N] on bf16 x, w: the MFMA kernels of meant_linear_fwd with the
 * accumulator plus bias stored unrounded -- the value the bf16 output is rounded from, so bf16(y) equals meant_linear_fwd's y bit for
 * bit at the same shape.  K % 8 == 0, ldx % 8 == 0, x, w and y 16-byte aligned, otherwise MEANT_ERR_UNSUPPORTED (no f32-engine detour). */
int meant_linear_fwd_f32out(const void* x, int64_t ldx, const void* w, const float* bias, float* y, int64_t ldy, int64_t M,
                            int64_t N, int64_t K, void* stream);
/* Fused q|k|v projection + rotary:  qkv[M, 3*H*Dh] = x[M,K] w[3*H*Dh, K]^T + bias, then the rotation of
 * meant_rotary_qk on the q and k blocks (tables may be NULL: plain projection).  In the bf16 tier the rotation
 * rides the GEMM epilogue (no extra pass over qkv) at every K % 8 == 0 (Dh % 8 == 0, R % 8 == 0), K % 64 != 0 included
 * (K-tail kernels, as meant_linear_fwd); any other (Dh, R), and the f32 tier, run the plain projection and then
 * meant_rotary_qk in place.   meant/attention.py:36-40, meant/xPosAttention.py:37-39
 * meant_qkv_proj_fwd_live, kv_lists: NULL (the same call), or the lists of meant_kv_live_rows(key mask, M / S, S, ...) of the attention that will read qkv (bf16 tier,
 * S % 256 == 0; ignored otherwise).  The k | v columns of the DEAD 256-row panels -- rows the attention never reads -- are then zeros on
 * return, and where the streaming GEMM takes the projection (H*Dh % 256 == 0, its usual shape rules) they are never computed: the q
 * section runs over all row panels, the k | v section over the live ones.  Every other element is what it is without the lists. */
int meant_qkv_proj_fwd(const void* x, int64_t ldx, const void* w, const float* bias, void* qkv, int64_t M,
                       int64_t K, int64_t S, int H, int Dh, int R, const float* qa, const float* qb,
                       const float* ka, const float* kb, int dtype, void* stream);
int meant_qkv_proj_fwd_live(const void* x, int64_t ldx, const void* w, const float* bias, void* qkv, int64_t M,
                            int64_t K, int64_t S, int H, int Dh, int R, const float* qa, const float* qb,
                            const float* ka, const float* kb, const void* kv_lists, int dtype, void* stream);
/* Linear with its input RMSNorm folded in (see "RMSNorm folded into the Linear" above).
 * forward : y = act(row_scale[m] (x w^T) + bias) (+ residual); w = W diag(g) in the act dtype; preact as in meant_linear_fwd.
 * backward: dx[M,K] = dy_scaled[M,N] w  -  coef[m] x[m,:]  (+ dres) (+ dres_pooled[m / group_rows, :] / group_rows),
 *           dy_scaled / coef from meant_rmsnorm_bwd_chain; dres: the gradient through the residual branch that shares x
 *           (act dtype [M,K]); dres_pooled: float [M / group_rows, K], the gradient of the sequence means of x.
 *           (dW' = dy_scaled^T x through meant_linear_bwd_dw with dbias NULL.) */
int meant_linear_fwd_rowscale(const void* x, int64_t ldx, const void* w, const float* bias, const float* row_scale,
                              const void* residual, int64_t ldr, void* y, int64_t ldy, void* preact, int64_t M, int64_t N,
                              int64_t K, int epilogue, int dtype, void* stream);
int meant_linear_bwd_dx_norm(const void* dy_scaled, int64_t lddy, const void* wT, const void* x, int64_t ldx,
                             const float* coef, const void* dres, int64_t lddres, const float* dres_pooled,
                             int64_t group_rows, void* dx, int64_t lddx, int64_t M, int64_t N, int64_t K, int dtype,
                             void* stream);
/* dx[M,K] = dy[M,N] w[N,K]   (wT is w transposed, [K,N], act dtype: see meant_transpose2d).  The reduction length is N: bf16
 * tier, any N % 8 == 0 on the MFMA kernels (N % 64 != 0: the K-tail forms, as meant_linear_fwd); K is free (K % 8 != 0 stores
 * element by element).  N % 8 != 0 (or lddy % 8 != 0, or an unaligned operand) takes the exact-f32 engine on bf16 storage; a caller
 * with such an N pads dy and wT to ceil8(N) zero columns with meant_pad_copy2d first and passes N = lddy = ceil8(N). */
int meant_linear_bwd_dx(const void* dy, int64_t lddy, const void* wT, void* dx, int64_t lddx, int64_t M,
                        int64_t N, int64_t K, int dtype, void* stream);
/* dw[N,K] += dy[M,N]^T x[M,K]  and  dbias[N] += colsum(dy)  -- float accumulators the caller zeroes
 * (or pre-loads: gradient buckets, accumulation across micro-batches).  dbias may be NULL.
 * workspace: meant_linear_bwd_dw_ws(M, N, K, dtype) bytes (0 unless the "deterministic" option is on: then the
 * per-workgroup partial sums go there and are added up in a fixed order); NULL / 0 otherwise.
 * bf16 tier: the MFMA kernels need N >= 8, K >= 8, lddy % 8 == 0, ldx % 8 == 0 and 16-byte aligned dy, x; they fetch both operands in
 * 8-column pieces, so N and K have to be the widths that are really there in multiples of 8: a caller with N % 8 != 0 (K % 8 != 0)
 * pads dy (x) with zero columns to ceil8 first and passes the padded width with a dw of [ceil8(N), ceil8(K)] and a dbias of
 * [ceil8(N)], which it cuts back.  Everything else takes the exact-f32 engine on bf16 storage. */
size_t meant_linear_bwd_dw_ws(int64_t M, int64_t N, int64_t K, int dtype);
int meant_linear_bwd_dw(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, float* dbias,
                        int64_t M, int64_t N, int64_t K, int dtype, void* workspace, size_t workspace_bytes,
                        void* stream);
/* The same "+=" over a LIST of 64-row blocks of the token axis: rows_list[0 .. *rows_count) are ascending block indices (block b = rows
 * 64 b .. 64 b + 63), both in device memory -- the count is read by the kernel, never by the host -- and every row of dy OUTSIDE the listed
 * blocks must be zero (the dK / dV rows of padded key blocks, see meant_kv_live_rows).  bf16 tier with M % 64 == 0, N % 256 == 0,
 * K % 256 == 0, M >= 4096 and the "deterministic" option off: the 256 x 256 MFMA kernel walks the listed blocks only, its token-axis
 * splits sharing them evenly.  Every other case sums all M rows as meant_linear_bwd_dw does (same workspace rule): the same sums. */
int meant_linear_bwd_dw_rows(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, float* dbias,
                             const int* rows_list, const int* rows_count, int64_t M, int64_t N, int64_t K, int dtype,
                             void* workspace, size_t workspace_bytes, void* stream);

/* generic strided batched GEMM, float storage, f32 MFMA (exact fp32 products):
 * C[b1,b2][m,n] = alpha * sum_k A[b1,b2](m,k) * B[b1,b2](k,n)   (+ C if accumulate)
 * element (i,j) of X in batch (b1,b2) is at X + b1*sXb1 + b2*sXb2 + i*sXr + j*sXc. */
int meant_gemm_f32_strided(const float* A, const float* B, float* C, int64_t M, int64_t N, int64_t K,
                           int64_t nb1, int64_t nb2, const int64_t* sA /*b1,b2,m,k*/,
                           const int64_t* sB /*b1,b2,k,n*/, const int64_t* sC /*b1,b2,m,n*/, float alpha,
                           int accumulate, void* stream);

/* ---- rotary / xPos -------------------- meant/rotary_embedding_torch.py:31-44,96-110
 * In-place on the q and k column blocks of a packed [T, 3*H*Dh] projection buffer:
 *   out[c] = t[c]*A[pos,c] + rot(t)[c]*B[pos,c]  for lanes c < R of every head,
 *   rot(t)[2j] = -t[2j+1], rot(t)[2j+1] = t[2j];   pos = row mod S.
 * qa,qb,ka,kb: float [S, R] (cos*scale, sin*scale for q and for k).  `transpose` != 0 applies
 * the adjoint (backward).  Any Dh > 0 and any even R in [0, Dh], both dtypes.  Dh % 8 == 0 with a 16-byte aligned qkv moves
 * 16-byte chunks; any other Dh, or a base that is only element-aligned, is rotated pair by pair.  Lanes >= R of a head, the v
 * block and the tables at or beyond column R of a row are never touched.  Tables padded from R to ceil8(R) columns with
 * identity columns (a = 1, b = 0) rotate to the same values. */
int meant_rotary_qk(void* qkv, int64_t T, int64_t S, int H, int Dh, int R, const float* qa, const float* qb,
                    const float* ka, const float* kb, int transpose, int dtype, void* stream);

/* ---- attention core -------- meant/attention.py:43-57, meant/xPosAttention.py:41-63
 * qkv: act [G*S, 3*H*Dh] packed (q | k | v column blocks, already rotated); o: act [G*S, H*Dh];
 * lse: float [G, H, S, 2] = (row max m, log sum_j exp(score_j - m)) of the scaled, masked scores --
 *      kept as a pair because the additive -1e9 padding term makes m ~ -1e9 on fully padded rows.  It is
 *      opaque state handed from meant_attn_fwd to meant_attn_bwd of the SAME dtype (natural-log units in
 *      the f32 tier, log2 units in the bf16 tier);
 * key_mask: float [G, S] of {0,1} or NULL (adds (1-mask)*-1e9 to the scores);
 * causal: scores[i,j] = -inf for j > i;  scale is the caller's (the reference: 1/sqrt(dim), NOT 1/sqrt(Dh)).
 * bf16: fused flash kernels for Dh = 64, 96 (the reference's default: 8 heads at d = 768, meant/meant.py:149), 128, 160,
 * 192 and 256 (8 heads at d = 1280 / 1536 / 2048) (a caller with another head dim below 256, a multiple of 8 or not, pads every
 * head to one of these with zeros -- zero rows in the projection weight -- and keeps its own scale; other Dh given to this entry
 * take a slow fp32 detour through `workspace`); f32: materialised scores in `workspace`, any Dh. */
size_t meant_attn_ws(int64_t G, int64_t S, int H, int Dh, int dtype);
/* what meant_attn_fwd alone needs (mask bias, tile flags); meant_attn_ws covers forward and backward (bf16: the backward's row
 * statistics and, for 256 < S <= 512 at Dh = 64, the single-pass backward's partial-dQ scratch of G*H*64 KiB) */
size_t meant_attn_fwd_ws(int64_t G, int64_t S, int H, int Dh, int dtype);
/* Live-row lists of a key-masked attention over G sequences of S tokens (S % 256 == 0), for the GEMMs around it.  A 64-row block of
 * the [G * S] token rows is DEAD when the bf16 attention kernels skip its key tile outright: all of its 64 keys are padding and every
 * query row of the sequence has a live visible key (key 0 under the causal mask, any key otherwise) -- the kernels then never read the
 * block's K / V rows and write exact zeros into its dK / dV rows.  It is the kernels' own rule, one device function shared with their mask
 * preparation.  A 256-row panel is dead when its four blocks are.
 * lists (int32 words, meant_kv_live_rows_ws(G, S) bytes; nblk = G * S / 64, npan = nblk / 4):
 *   [0] live blocks, [1] live panels, [2] dead panels, [3 .. 63] unused
 *   [64 ..)               the live blocks, ascending                                  (nblk words, the first [0] valid)
 *   [64 + nblk ..)        the live panels, ordered by position range: all panels p with p mod (S / 256) == 0 first, ascending, then
 *                         == 1, ... -- the order in which the rotary projection walks its row panels   (npan words, [1] valid)
 *   [64 + nblk + npan ..) the dead panels, in the same order                          (npan words, [2] valid)
 *   then nblk words of scratch.
 * The 64 is MEANT_KV_LIST_HDR: the one declaration of the header's length, for the library, its callers and the tests.
 * No host synchronisation: the counts stay on the device. */
enum meant_kv_list_layout { MEANT_KV_LIST_HDR = 64 };
size_t meant_kv_live_rows_ws(int64_t G, int64_t S);
int meant_kv_live_rows(const float* key_mask, int64_t G, int64_t S, int causal, void* lists, size_t lists_bytes, void* stream);
int meant_attn_fwd(const void* qkv, void* o, float* lse, const float* key_mask, int64_t G, int64_t S, int H,
                   int Dh, float scale, int causal, int dtype, void* workspace, size_t workspace_bytes,
                   void* stream);
/* Attention with dropout ON THE SCORE MATRIX, where meant/xPosAttention.py:59 has it (`scores = self.dropout(scores)`: after the
 * causal fill and the key-padding term, before the softmax; p = 0 in every reference model): a dropped score becomes 0 -- also
 * that of a masked position, which thereby becomes visible --, a kept one is divided by 1 - drop_p.  Score (g, h, i, j) is kept iff
 * the counter-based uniform of (seed, ((g H + h) S + i) S + j) is >= drop_p; forward and backward must be given the same
 * (drop_p, seed).  Same buffers and layouts as meant_attn_fwd / meant_attn_bwd; q and k arrive rotated (meant_rotary_qk) and dqkv
 * is the gradient w.r.t. that rotated buffer (apply meant_rotary_qk with transpose = 1 afterwards).  Materialised scores (the
 * fp32 core; bf16 through fp32 copies in the workspace): correct, not fast. */
size_t meant_attn_drop_ws(int64_t G, int64_t S, int H, int Dh, int dtype);
int meant_attn_drop_fwd(const void* qkv, void* o, float* lse, const float* key_mask, int64_t G, int64_t S, int H, int Dh,
                        float scale, int causal, float drop_p, uint64_t seed, int dtype, void* workspace,
                        size_t workspace_bytes, void* stream);
int meant_attn_drop_bwd(const void* qkv, const void* o, const void* do_, const float* lse, const float* key_mask, void* dqkv,
                        int64_t G, int64_t S, int H, int Dh, float scale, int causal, float drop_p, uint64_t seed,
                        int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* dqkv: act [G*S, 3*H*Dh] (every element written); do_: act [G*S, H*Dh].
 * If the rotary tables qa,qb,ka,kb (float [S, R], as in meant_rotary_qk) are given, dq and dk are returned
 * already pulled back through the rotation (the adjoint of meant_rotary_qk), i.e. dqkv is the gradient of
 * the un-rotated projection; pass NULLs (and R = 0) for the gradient of the rotated buffer.  Any even R <= Dh: the bf16 kernels
 * apply the adjoint themselves at R % 8 == 0 and R <= 64, otherwise the backward runs without tables and meant_rotary_qk
 * (transpose = 1) follows in place. */
int meant_attn_bwd(const void* qkv, const void* o, const void* do_, const float* lse, const float* key_mask,
                   void* dqkv, int64_t G, int64_t S, int H, int Dh, float scale, int causal, const float* qa,
                   const float* qb, const float* ka, const float* kb, int R, int dtype, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- divided space-time attention glue ----------------------- src/meant/timesformer_pytorch.py:108-145
 * The fork's TimeSformer regroups the patch tokens between the q|k|v projection and the attention core ('(b n) f' for
 * the time attention, '(b f) n' for the space attention, the cls key / value in front of every group) and lets the cls
 * query attend to every token.  The core itself is meant_attn_fwd / _bwd on the regrouped buffer; these move the rows.
 * dst[r, :] = src[idx[r], :] for idx[r] >= 0, zeros for idx[r] == -1, fill[:] (act [W]) for idx[r] == -2; rows of W
 * elements.  Any W > 0: 16-byte accesses at W % 8 == 0 (16-byte aligned src, dst, fill), element by element otherwise (element
 * alignment; route "rows_elem"); the stored bits are copied, nothing is touched at or beyond column W of a row.  (Regrouping, its
 * inverse for the outputs, and the cls-token concatenation of :211-213.) */
int meant_gather_rows(const void* src, const int32_t* idx, const void* fill, void* dst, int64_t n, int64_t W, int dtype,
                      void* stream);
/* The regrouping gather of a packed q|k|v buffer (rows of 3 * H * Dh) with the rotary map applied on the way: row r of dst is
 * row idx[r] of src (zeros for idx[r] < 0), its q and k heads rotated by the tables' row r % S exactly as meant_rotary_qk
 * (transpose = 0) would rotate them in place afterwards (same arithmetic, one rounding); v is copied.
 * (timesformer_pytorch.py:124-131: rearrange, then rot_emb.rotate_queries_and_keys.) */
int meant_gather_rows_rot(const void* src, const int32_t* idx, void* dst, int64_t n, int64_t S, int H, int Dh, int R,
                          const float* qa, const float* qb, const float* ka, const float* kb, int dtype, void* stream);
/* backward of a regrouping gather with index int32 [G, S] into the L rows of each of B sequences, whose column 0 is
 * the same (cls) row in every group and whose other entries are a permutation of the remaining rows: dsrc [B, L, W]
 * is written completely -- dsrc[b, index[g, s]] = ddst[b, g, s] for s >= 1, dsrc[b, index[0, 0]] = sum_g ddst[b, g, 0]. */
int meant_group_scatter(const void* ddst, const int32_t* index, void* dsrc, int64_t B, int64_t L, int64_t G, int64_t S,
                        int64_t W, int dtype, void* stream);
/* cls query: out[b, h*Dh .. +Dh] (row stride ld_out) = softmax_j(scale q[b, 0, h] . k[b, j, h] + (1 - key_mask[b, j]) * -1e9)
 * v[b, j, h] over all L rows of the packed qkv [B, L, 3*H*Dh] (:116-119, cls_mask :252-253); a key with key_mask 0 gets the
 * score -1e9 itself and no score gradient (masked_fill), so every key masked gives uniform weights.  stats: float [B, H, 2]
 * (max score, log of the sum of exp(score - max)).  The backward ADDS to dqkv (the buffer meant_group_scatter has filled): dq
 * of row 0, dk and dv of every row; ld_dout % 8 == 0.  Dh % 8 == 0, Dh <= 256; L bounded by the LDS score buffer,
 * (L + 4 + rpi*Dh) floats forward and (2L + 4 + rpi*Dh) backward within 159 KiB, rpi = 256 / (Dh / 8) (~38 k / ~19 k
 * tokens); a longer L returns MEANT_ERR_UNSUPPORTED before any launch. */
int meant_attn_cls_fwd(const void* qkv, void* out, int64_t ld_out, float* stats, const float* key_mask, int64_t B, int64_t L,
                       int H, int Dh, float scale, int dtype, void* stream);
int meant_attn_cls_bwd(const void* qkv, const void* out, int64_t ld_out, const void* dout, int64_t ld_dout,
                       const float* stats, const float* key_mask, void* dqkv, int64_t B, int64_t L, int H, int Dh,
                       float scale, int dtype, void* stream);
/* the largest L the pair above takes at head dim Dh (backward != 0: meant_attn_cls_bwd's bound, half the forward's); 0 for a
 * head dim it refuses.  Host arithmetic. */
int64_t meant_attn_cls_max_len(int Dh, int backward);
/* The same attention over key segments, for L past those bounds (route "attn_cls_split"): a workgroup per (head, video, segment)
 * handles ceil(L / nseg) keys, a second kernel merges the segments of a (video, head) in the order 0 ... nseg - 1 (forward:
 * m = max m_s, l = sum l_s e^(m_s - m), o = sum o_s e^(m_s - m) / l; backward: dq = sum of the segments' partial dq, added to row
 * 0).  Same contract as the pair above in every other respect -- stats format (a forward of one pair may be followed by the
 * backward of the other), masked keys, strided out rows written in [0, H*Dh) only, dqkv ADDED to -- and no atomics or completion
 * counters: two runs give the same bits.  nseg = 0: the smallest count whose segment fits the LDS bound of the respective
 * direction; nseg >= 1: taken as given, MEANT_ERR_UNSUPPORTED if a segment does not fit (or nseg > 65535), nseg > L:
 * MEANT_ERR_ARG.  Dh % 8 == 0, Dh <= 256, B, H <= 65535, L < 2^31; row offsets are 64-bit.  workspace:
 * meant_attn_cls_split_ws(B, L, H, Dh, nseg) bytes = B*H*nseg*(Dh+2) floats (host arithmetic; nseg = 0 sizes for the backward's
 * count, which also covers the forward's; 0 for arguments the entries refuse), 16-byte aligned; too small: MEANT_ERR_WORKSPACE. */
size_t meant_attn_cls_split_ws(int64_t B, int64_t L, int H, int Dh, int nseg);
int meant_attn_cls_split_fwd(const void* qkv, void* out, int64_t ld_out, float* stats, const float* key_mask, int64_t B,
                             int64_t L, int H, int Dh, float scale, int nseg, int dtype, void* workspace,
                             size_t workspace_bytes, void* stream);
int meant_attn_cls_split_bwd(const void* qkv, const void* out, int64_t ld_out, const void* dout, int64_t ld_dout,
                             const float* stats, const float* key_mask, void* dqkv, int64_t B, int64_t L, int H, int Dh,
                             float scale, int nseg, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* time token shift of the patch tokens of x act [B, 1 + frames*n, d] (PreTokenShift, src/meant/timesformer_pytorch.py:28-53):
 * columns [0, d/3) from the next frame, [d/3, 2d/3) unchanged, [2d/3, 3(d/3)) from the previous frame, zeros beyond the
 * clip's ends; the cls row and any remainder columns pass through.  Any d >= 3: 16-byte accesses at d % 8 == 0, element by
 * element otherwise (element alignment; route "rows_elem").  transpose != 0: the adjoint (backward).  x != y. */
int meant_token_shift(const void* x, void* y, int64_t B, int64_t frames, int64_t n, int64_t d, int transpose, int dtype,
                      void* stream);
/* inverted dropout y = x * keep / (1 - p) (nn.Dropout at :70,:101): counter-based mask from (seed, element index), so the
 * backward is the same call on dy.  Any n > 0: element i takes part i & 7 of the draw for i >> 3, so the first 8 * (n / 8)
 * outputs are those of the call on that prefix; at n % 8 != 0 (route "rows_elem") the full groups of 8 take 16-byte accesses where
 * x and y are 16-byte aligned, everything else goes element by element (element alignment). */
int meant_dropout(const void* x, void* y, int64_t n, float p, uint64_t seed, int dtype, void* stream);

/* ---- temporal attention core ----------------------------- meant/temporal.py:44-56
 * q: act [B, H*Dh] (last lag step), kv: act [B*L, 2*H*Dh] packed (k | v); o: act [B, H*Dh];
 * p: float [B, H, L] softmax weights (saved; the forward may hold raw scores in it while it runs).
 * Any lag L >= 1 and any head dim: L <= 64 on the one-wave-per-(b, h) kernels, L > 64 on the long-lag kernels (route
 * "temporal_long"; temporal_long.hip): one workgroup per (b, h) whose waves split L, several key rows per 16-byte load
 * instruction, online softmax merged through LDS; head dims that are no multiple of 8 or above 512, and operands that are
 * not 16-byte aligned, on scalar-access kernels.  The backward recomputes nothing from o: its row term sum_l p_l dp_l comes
 * from a first pass over V, whose dp_l stay in LDS up to L = 2048 (beyond, V is read a second time).  No atomics: two runs
 * give the same bits.  L <= 0 fails with MEANT_ERR_UNSUPPORTED. */
int meant_temporal_attn_fwd(const void* q, const void* kv, void* o, float* p, int64_t B, int L, int H, int Dh,
                            float scale, int dtype, void* stream);
int meant_temporal_attn_bwd(const void* q, const void* kv, const float* p, const void* do_, void* dq, void* dkv,
                            int64_t B, int L, int H, int Dh, float scale, int dtype, void* stream);

/* ---- patchify ------------------------------------------------------ meant/meant.py:194
 * images: float or act [G, C, Hh, Ww] -> patches act [G*(Hh/p)*(Ww/p), p*p*C], channel fastest. */
int meant_patchify(const void* images, int images_dtype, void* patches, int64_t G, int C, int Hh, int Ww, int p,
                   int dtype, void* stream);

/* ---- input pipeline: raw pixels -> normalised patches in one pass ----- in_loop_train.py:48,589-602 (float64
 * graphs, optional global (x - mean) / std), meant/meant.py:194 (patchify).
 * images: raw [G, C, Hh, Ww] of meant_raw_dtype; patches act [G*(Hh/p)*(Ww/p), p*p*C] = ((float)x - mean) * inv_std. */
int meant_patchify_raw(const void* images, int raw_dtype, float mean, float inv_std, void* patches, int64_t G, int C,
                       int Hh, int Ww, int p, int dtype, void* stream);

/* ---- sequence mean-pool ------------------------------------------- meant/meant.py:231
 * x: act [G, S, d] -> out[g, col_off : col_off+d] of a [G, ld_out] buffer (the concat) whose storage type
 * is out_dtype: the pooled features and everything after them (temporal encoder, head: 0.06 % of the
 * FLOPs) run in fp32 also in the bf16 tier.  Any d > 0, ld_out and col_off with 0 <= col_off, col_off + d <= ld_out: 16-byte
 * accesses where d, ld_out and col_off are multiples of 8 and both bases are 16-byte aligned, element by element otherwise (the same
 * sums in the same order).  x / dx are not touched at or beyond column d of a row, out / dout not outside [col_off, col_off + d)
 * of a row.  Ordered sums, no atomics: the same bits on every run. */
int meant_meanpool_fwd(const void* x, void* out, int64_t ld_out, int64_t col_off, int64_t G, int64_t S, int64_t d,
                       int dtype, int out_dtype, void* stream);
int meant_meanpool_bwd(const void* dout, int64_t ld_out, int64_t col_off, void* dx, int64_t G, int64_t S, int64_t d,
                       int dtype, int out_dtype, void* stream);

/* ---- learned softmax pooling of the token axis ------- src/meant/meant_tweet.py:173,259-261, src/meant/meant_timesformer.py:274,336-338
 * lang_prep = Linear(d, d) -> LayerNorm(d) -> GELU -> Linear(d, 1) -> Softmax over the sequence, then pooled = sum_s w_s x_s.  The first
 * Linear is meant_linear_fwd; everything behind it is two passes forward and two backward.  With T = G S token rows, h [T, d] the first
 * Linear's output, n = LayerNorm(h) gamma + beta (biased variance), a = gelu_erf(n):
 *   meant_ln_gelu_dot_fwd   score[t] = a[t, :] . w2 + b2 from one read of h (the row stays in registers); n and a are never written.
 *                           score: float [rows]; stats: float [rows, 2] = (mean, rstd) as meant_layernorm_fwd keeps them; b2: float [1] on the
 *                           device (or NULL: 0).
 *   meant_softmax_pool_fwd  per sequence g: w[g, :] = softmax_s(score[g, :]) over the positions the mask keeps (0 elsewhere),
 *                           out[g, col_off : col_off + d] = sum_s w[g, s] x[g, s, :] in a [G, ld_out] buffer of out_dtype, under the contract of
 *                           meant_meanpool_fwd for ld_out, col_off and out_dtype.  key_mask: NULL or [G, S] of mask_kind (a meant_mask_dtype), 0
 *                           = the position is left out; a sequence with every position left out gives w = 0 and out = 0.  w: float [G, S], kept
 *                           for the backward.
 *   meant_softmax_pool_bwd  dx[g, s, :] = w[g, s] dout[g, :] (act), dscore[g, s] = w[g, s] (r[g, s] - sum_t w[g, t] r[g, t]) with the row dots
 *                           r[g, s] = x[g, s, :] . dout[g, :] -- the second term from the dots themselves in a fixed order, one read of x.
 *   meant_ln_gelu_dot_bwd   recomputes n and a from h and stats in float (exact-erf GELU and derivative); dh (act) = the LayerNorm backward of
 *                           dn = dscore w2 gelu_erf'(n); dgamma, dbeta and dw2 = sum_rows dscore a (float [d], overwritten) through per-block
 *                           partial rows in the workspace, reduced in a fixed order.  workspace: meant_ln_gelu_dot_bwd_ws(rows, d) bytes.
 * The gradient of b2 is exactly zero (a softmax does not see a shift) and no entry computes it.
 * Any d > 0, S >= 1, G >= 1, both tiers: 16-byte accesses where d % 8 == 0 (the pool: and ld_out, col_off) and the bases are 16-byte aligned,
 * element access otherwise; nothing is touched at or beyond column d of a row, out / dout not outside [col_off, col_off + d).  All sums
 * are ordered, no atomics: two runs give the same bits.  rows, d, S, G <= 0, a null pointer, an unknown dtype or mask_kind: MEANT_ERR_ARG
 * before any launch. */
int meant_ln_gelu_dot_fwd(const void* h, const float* gamma, const float* beta, const float* w2, const float* b2, float* score,
                          float* stats, int64_t rows, int64_t d, float eps, int dtype, void* stream);
int meant_softmax_pool_fwd(const void* x, const float* score, const void* key_mask, int mask_kind, float* w, void* out, int64_t ld_out,
                           int64_t col_off, int64_t G, int64_t S, int64_t d, int dtype, int out_dtype, void* stream);
int meant_softmax_pool_bwd(const void* dout, int64_t ld_out, int64_t col_off, const void* x, const float* w, void* dx, float* dscore,
                           int64_t G, int64_t S, int64_t d, int dtype, int out_dtype, void* stream);
size_t meant_ln_gelu_dot_bwd_ws(int64_t rows, int64_t d);
int meant_ln_gelu_dot_bwd(const float* dscore, const void* h, const float* stats, const float* gamma, const float* beta, const float* w2,
                          void* dh, float* dgamma, float* dbeta, float* dw2, int64_t rows, int64_t d, int dtype, void* workspace,
                          size_t workspace_bytes, void* stream);
/* the price columns of the fork's Stocknet fusion (src/meant/meant_tweet_price.py:208, torch.cat((pooled, prices), dim=2)):
 * out[r, col_off + c] (float, row stride ld_out) = (float)src[r, c] for c < cols; src dense [rows, cols] of price_dtype, a meant_price_dtype.
 * Element access; nothing else of out is touched. */
enum meant_price_dtype { MEANT_PRICE_F32 = 0, MEANT_PRICE_BF16 = 1, MEANT_PRICE_F64 = 2, MEANT_PRICE_F16 = 3 };
int meant_price_cols(const void* src, int price_dtype, float* out, int64_t ld_out, int64_t col_off, int64_t rows, int64_t cols,
                     void* stream);

/* ---- small elementwise helpers ---- */
/* y[r, :] = x[r, :] + v[(r mod period), :]  (temp_embedding add, meant/meant.py:141-142).  Any d > 0: 16-byte accesses where
 * d % 8 == 0 and x, y are 16-byte aligned, element by element otherwise; nothing is touched at or beyond column d of a row. */
int meant_add_rowvec(const void* x, const float* v, void* y, int64_t rows, int64_t d, int64_t period, int dtype,
                     void* stream);
/* dv[period, d] (float, overwritten) = sum over rows r = i mod period of dy[r, :]; any d > 0 (element access), ordered sums */
int meant_add_rowvec_bwd(const void* dy, float* dv, int64_t rows, int64_t d, int64_t period, int dtype, void* stream);
/* dx = dy * gelu'(pre) */
int meant_gelu_bwd(const void* dy, const void* pre, void* dx, int64_t n, int dtype, void* stream);
/* dx = dy * y * (1-y) */
int meant_sigmoid_bwd(const void* dy, const void* y, void* dx, int64_t n, int dtype, void* stream);
/* GEGLU ---------------------------------------------------- src/meant/timesformer_pytorch.py:60-63
 * h: act [rows, 2w] = [a | g]  ->  y: act [rows, w] = a * gelu(g);   dh = [dy * gelu(g) | dy * a * gelu'(g)].  Any w > 0: 16-byte
 * accesses at w % 8 == 0, element by element otherwise (element alignment; route "rows_elem"), the same gelu / gelu' evaluation. */
int meant_geglu_fwd(const void* h, void* y, int64_t rows, int64_t w, int dtype, void* stream);
int meant_geglu_bwd(const void* h, const void* dy, void* dh, int64_t rows, int64_t w, int dtype, void* stream);
/* y = a + b */
int meant_add(const void* a, const void* b, void* y, int64_t n, int dtype, void* stream);
/* dst(act dtype_dst) = src(dtype_src), n elements */
int meant_cast(const void* src, int dtype_src, void* dst, int dtype_dst, int64_t n, void* stream);
/* dst[c, r] (dtype_dst) = src[r, c] (dtype_src); src is [rows, cols] */
int meant_transpose2d(const void* src, int dtype_src, void* dst, int dtype_dst, int64_t rows, int64_t cols,
                      void* stream);
/* dst[r, c] (dtype_dst, row stride ld_dst) = src[r, c] (dtype_src, row stride ld_src) for c < min(cols_src, cols_dst),
 * 0 for cols_src <= c < cols_dst; columns of src at or beyond cols_dst are dropped.  Rows of src need element alignment
 * only (the operands of a Linear whose K is not a multiple of 8 are padded to ceil8(K) with it, and its dW is cut
 * back out of the padded accumulator); src is never read at or beyond column cols_src of a row. */
int meant_pad_copy2d(const void* src, int64_t ld_src, int64_t cols_src, int dtype_src, void* dst, int64_t ld_dst,
                     int64_t cols_dst, int dtype_dst, int64_t rows, void* stream);
/* embedding gather: out act [n, d] = table float [V, d] rows ids[n] (int64); and its scatter-add backward
 * into dtable float [V, d] (caller zeroes).            nn.Embedding at meant/meant.py:211
 * Both take any d > 0 (the gather element by element where d % 8 != 0; the scatter-add is float atomics per element). */
int meant_embedding_fwd(const float* table, const int64_t* ids, void* out, int64_t n, int64_t d, int64_t V, int dtype,
                        void* stream);
int meant_embedding_bwd(const void* dout, const int64_t* ids, float* dtable, int64_t n, int64_t d, int64_t V, int dtype,
                        void* stream);
/* same, over ids sorted by the caller: sorted_ids[j] ascending, order[j] = row of dout that carries it.  Rows of
 * equal id are summed on chip before one atomic row add, so repeated tokens do not contend (d <= 1024). */
int meant_embedding_bwd_sorted(const void* dout, const int64_t* sorted_ids, const int64_t* order, float* dtable,
                               int64_t n, int64_t d, int64_t V, int dtype, void* stream);
/* the rows of ids in [id_lo, id_hi) only: the table's gradient produced in row slices, so that a data-parallel caller can start
 * the all-reduce of a slice while the next one is still being summed (the 196 MB table is two thirds of the gradient bytes and
 * final only with the last kernel of backward).  The union over a partition of [0, V) equals meant_embedding_bwd_sorted. */
int meant_embedding_bwd_sorted_range(const void* dout, const int64_t* sorted_ids, const int64_t* order, float* dtable,
                                     int64_t n, int64_t d, int64_t V, int64_t id_lo, int64_t id_hi, int dtype, void* stream);
/* stable device sort of the ids, clamped into [0, V) as meant_embedding_fwd clamps them: sorted_ids[j] ascending (int64 [n]),
 * order[j] = original row of the j-th smallest id, equal ids in ascending row order -- the layout the two *_sorted calls above
 * and meant_embedding_bwd_seg read.  An LSD radix sort over 8-bit digits, ceil(bits(V - 1) / 8) passes; the result does not
 * depend on timing.  ids, sorted_ids and order must not overlap (MEANT_ERR_ARG).  n, V < 2^31 (beyond: MEANT_ERR_UNSUPPORTED).  workspace: meant_sort_ids_ws(n, V) bytes (host arithmetic). */
size_t meant_sort_ids_ws(int64_t n, int64_t V);
int meant_sort_ids(const int64_t* ids, int64_t n, int64_t V, int64_t* sorted_ids, int64_t* order, void* workspace,
                   size_t workspace_bytes, void* stream);
/* the scatter-add over sorted ids at any d % 8 == 0 (otherwise MEANT_ERR_UNSUPPORTED), rows of ids in [id_lo, id_hi) only, added
 * into dtable; no float atomics with or without the "deterministic" option: runs of equal ids that cross the 256-entry stretch of
 * a wave leave partial sums in the workspace, which two small kernels add in a fixed order that depends on the sorted ids alone.
 * Bit-reproducible for a given (sorted_ids, order, dout); the union over a partition of [0, V) equals one call over [0, V) bit
 * for bit.  workspace: meant_embedding_bwd_seg_ws(n, d) bytes (host arithmetic), 16-byte aligned. */
size_t meant_embedding_bwd_seg_ws(int64_t n, int64_t d);
int meant_embedding_bwd_seg(const void* dout, const int64_t* sorted_ids, const int64_t* order, float* dtable, int64_t n,
                            int64_t d, int64_t V, int64_t id_lo, int64_t id_hi, int dtype, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Backward of  x[t] = table[id[t]] -> n[t] = RMSNorm_gain(x[t]) -> qkv_pre[t] = W' n[t] + b'  once per vocabulary id instead of once per
 * token (bf16 tier): everything up to qkv_pre depends on id[t] alone and its backward is linear in the incoming gradients, so the token
 * gradients are summed by id first, D[v] = sum of dqkv[t] over the tokens with id v (fp32 sums over the sorted ids, no float atomics,
 * a function of (sorted_ids, order, dqkv) alone), and the GEMMs and the norm backward run on V rows:
 *   dw [N3, d] += D^T Ntab    db [N3] += colsum(dqkv)    dgain [d] = the norm gain's gradient (overwritten)
 *   dtable [V, d] += RMSNorm backward of (D W', table row)  +  the sum of dres[t] over the tokens with that id
 * dqkv: bf16 [n, N3], N3 = 3 H Dh, the gradient of the projection's output before the rotary map (what meant_attn_bwd returns with
 * its tables).  dres: bf16 [n, d] or NULL, the gradient of the residual branch that shares x.  sorted_ids / order: of meant_sort_ids
 * (ids clamped into [0, V) as meant_embedding_fwd clamps them).  table_bf16: the bf16 image [V, d] the lookup read.  wT: bf16 [d, N3],
 * W' transposed.  kv_lists: NULL, or the lists of meant_kv_live_rows of the attention that produced dqkv: the k | v columns of the rows
 * of dead 64-row blocks are exact zeros and are not read (needs n % 64 == 0).  D reaches the GEMMs as bf16 hi + lo images, D W' comes
 * back as two bf16 images, and the norm backward on the V rows is fp32: no tensor of V rows is rounded to bf16 once for all the tokens
 * of an id.
 * stage: MEANT_BY_ID_SHARED runs everything that does not depend on the id range (dw, db, dgain and the per-id rows kept in the
 * workspace); MEANT_BY_ID_TABLE adds rows [id_lo, id_hi) of the table's gradient from a workspace a SHARED stage filled.  Both bits:
 * one call does all.  Calls with TABLE over a partition of [0, V) give bit for bit what one call over [0, V) gives.
 * With option "deterministic" dw is an ordered sum and the whole result is bit-reproducible.
 * d % 8 == 0, H Dh % 64 == 0, n and V below 2^31.  workspace: meant_qkv_embed_bwd_by_id_ws(n, d, N3, V) bytes (host arithmetic; read
 * after option "deterministic" is set), 16-byte aligned.  Route name "qkv_by_id". */
enum meant_by_id_stage { MEANT_BY_ID_SHARED = 1, MEANT_BY_ID_TABLE = 2 };
size_t meant_qkv_embed_bwd_by_id_ws(int64_t n, int64_t d, int64_t N3, int64_t V);
/* The forward of the same chain once per vocabulary id (bf16 tier):  qkv[t] = bf16(rotary_{t mod S}(W' RMSNorm_gain(table[id[t]]) + b')).
 * In order: the norm forward on the bf16 table image (V rows, zero-padded to a multiple of 256), one NT GEMM of those rows with
 * unrounded float output into the workspace, and a gather over the sorted ids that reads an id's float row once per run of equal ids,
 * applies the rotary map of each token's position to the q and k heads (columns c < R of a head) and rounds once.  Every element has
 * the bits meant_rmsnorm_fwd followed by meant_qkv_proj_fwd_live gives it on the same operands.
 * table_bf16: the bf16 image [V, d] the lookup read.  w_bf16: W' [3 H Dh, d] in bf16, bias float [3 H Dh] or NULL.  sorted_ids / order:
 * of meant_sort_ids.  kv_lists: NULL, or the lists of meant_kv_live_rows(key mask, n / S, S, ...): the k | v columns of dead 256-row
 * panels are zeros on return and their float rows are not gathered.  qa .. kb: float [S, R] (or all NULL: no rotation), R % 8 == 0.
 * qkv: bf16 [n, 3 H Dh].  Entries of sorted_ids outside [0, V) or of order outside [0, n) are skipped.
 * meant_qkv_embed_fwd_by_id_ok: 1 where the route applies -- the streaming NT kernel takes both the [n, 3 H Dh] product it replaces and
 * the [V, 3 H Dh] product it runs (needs a current device: the rule counts compute units) --, else 0; the entry point fails with
 * MEANT_ERR_UNSUPPORTED where it is 0.  workspace: meant_qkv_embed_fwd_by_id_ws(n, d, N3 = 3 H Dh, V) bytes (host arithmetic: the
 * normed table, its row statistics, the float product [ceil256(V), N3] and a flag per 256-row panel, each rounded up to 256 bytes;
 * 0 for a shape the entry point rejects), 16-byte aligned.  Route name "qkv_fwd_by_id". */
size_t meant_qkv_embed_fwd_by_id_ws(int64_t n, int64_t d, int64_t N3, int64_t V);
int meant_qkv_embed_fwd_by_id_ok(int64_t n, int64_t d, int64_t N3, int64_t V);
int meant_qkv_embed_fwd_by_id(const void* table_bf16, const float* gain, float eps, const void* w_bf16, const float* bias,
                              const int64_t* sorted_ids, const int64_t* order, const void* kv_lists, const float* qa,
                              const float* qb, const float* ka, const float* kb, void* qkv, int64_t n, int64_t S, int64_t d,
                              int H, int Dh, int R, int64_t V, void* workspace, size_t workspace_bytes, void* stream);
int meant_qkv_embed_bwd_by_id(const void* dqkv, const void* dres, const int64_t* sorted_ids, const int64_t* order,
                              const void* table_bf16, const float* gain, float eps, const void* wT, const void* kv_lists,
                              float* dw, float* db, float* dgain, float* dtable, int64_t n, int64_t d, int64_t N3, int64_t V,
                              int64_t id_lo, int64_t id_hi, int stage, void* workspace, size_t workspace_bytes, void* stream);

/* ---- train-step tail ------------------------------------------- in_loop_train.py:232-238,547-548
 * CrossEntropyLoss (mean) applied to the model's probabilities [B, C] as the reference does: loss_accum[0] +=
 * loss (caller zeroes it), dprobs (optional) receives d loss / d probs.  A target outside [0, C) turns the loss and
 * that row of dprobs into NaN (no out-of-bounds access). */
int meant_ce_probs(const float* probs, const int64_t* target, float* loss_accum, float* dprobs, int64_t B, int C,
                   void* stream);
/* ---- large-vocabulary softmax cross-entropy (MLM pretrainer) ----------- pretrain_mlm.py:160,178
 * nn.CrossEntropyLoss() on logits act [T, ld] (V <= ld valid columns, the rest padding of the vocabulary GEMM),
 * target int64 [T] with `ignore_index` rows skipped: a row counts iff target != ignore_index && 0 <= target < V.  fwd:
 * row_loss[t] = logsumexp - logit[target] (0 if the row does not count, whatever it holds), lse float [T, 2] saved: the pair
 * (M, log S) with M the row maximum and S = sum_{j < V} exp(logit_j - M), so logsumexp = M + log S; the entries keep the two
 * apart (row_loss = log S + (M - logit[target]), softmax_j = exp((logit_j - M) - log S)) and no term grows with a shift of
 * the row.  A -inf logit is a masked column (probability 0); a row of nothing but -inf is NaN, as in torch.  bwd:
 * dlogits[t, j] = (softmax_j - [j == target]) * gscale[0] for j < V, exact zeros for rows that do not count (their logits are
 * not read) and for the padding columns, which the forward never reads; gscale is a device scalar (d loss / n_valid),
 * dlogits may alias logits. */
int meant_softmax_ce_fwd(const void* logits, int64_t ld, const int64_t* target, int64_t T, int64_t V, int64_t ignore_index,
                         float* row_loss, float* lse, int dtype, void* stream);
int meant_softmax_ce_bwd(const void* logits, int64_t ld, const int64_t* target, const float* lse, int64_t T, int64_t V,
                         int64_t ignore_index, const float* gscale, void* dlogits, int dtype, void* stream);
/* the rows that count, as lists: row t is labelled iff target[t] != ignore_index && 0 <= target[t] < V (the predicate of the two
 * calls above).  The reference's mlm_dataset labels 15 % of the positions and sets every other label to -100
 * (utils/custom_datasets.py:46-54, consumed at pretrain_mlm.py:160,178); the head is row-wise from its first op to the loss, so it
 * may run on the labelled rows alone.  count[0] = n, the number of labelled rows; idx int32 [T]: the labelled rows in ascending
 * order, -1 from place n on; inv int32 [T]: inv[t] = place of row t in that list, or -1; target_sel int64 [T]: target[idx[j]] for
 * j < n, ignore_index beyond.  With those tails a caller may round n up to any padded length m <= T and hand idx[0..m) to
 * meant_gather_rows (-1: a zero row) and target_sel[0..m) to the loss (ignored rows); inv gathers a gradient of the m rows back
 * to T rows with exact zeros elsewhere.  A stable compaction by prefix sums (wave ballots, per-workgroup counts, their scan,
 * the scatter): no atomics, two runs give the same bits.  T <= 0, V <= 0, a null pointer or buffers that overlap: MEANT_ERR_ARG;
 * T >= 2^31: MEANT_ERR_UNSUPPORTED before any launch.  workspace: meant_select_rows_ws(T) bytes (host arithmetic, monotone in T;
 * 0 for a T the call rejects). */
size_t meant_select_rows_ws(int64_t T);
int meant_select_rows(const int64_t* target, int64_t T, int64_t V, int64_t ignore_index, int32_t* idx, int32_t* inv,
                      int64_t* target_sel, int32_t* count, void* workspace, size_t workspace_bytes, void* stream);
/* ---- classification counts (utils/f1_metrics.py, fed per batch at in_loop_train.py:208-241, 281-319, 339-359) ----
 * Everything the reference's seven metrics (accuracy, F1 / precision / recall, macro and micro) are computed from, counted on the
 * device.  scores [B, ld], columns 0..C-1 are the classes (MEANT_F32 | MEANT_BF16; the columns C..ld-1, the padding of a
 * vocabulary GEMM, are never candidates and may hold anything); target int64 [B].
 * state int64 [3C + 4], zeroed once by the caller: tp[C], npred[C], ntarget[C], then n_rows, n_ignored, n_invalid, n_nan.
 * confusion: NULL or int64 [C, C], row = target, column = prediction.  The calls only ever ADD to both, and every counter is an
 * integer: any number of updates, in any order and with any workgroup arrival order, leaves bit-identical contents, and the
 * states of several devices may be summed.
 * Per row (the semantics of torch's scores.argmax(dim=1)): the prediction is the index of the greatest of the C columns, the
 * lowest index on a tie, a NaN counting as greater than everything (the first NaN's index).
 *   target == ignore_index            : n_ignored += 1 and nothing else
 *   target otherwise outside [0, C)   : n_invalid += 1 and nothing else (no address is formed from it)
 *   every other row                   : n_rows, npred[pred], ntarget[target] += 1; tp[pred] += 1 if pred == target;
 *                                       confusion[target * C + pred] += 1; n_nan += 1 if one of its C columns is a NaN
 * The scores of an ignored or invalid row are not read.  meant_metrics_update_labels does the same from predictions int64 [B];
 * one outside [0, C) makes the row invalid; it never adds to n_nan.
 * Forms (route names of meant_route_count): "metrics_rows" for C <= 16, a lane per row, the counters summed per workgroup in LDS,
 * one global integer atomic per non-zero counter and workgroup; "metrics_wave" above, a wave per row, 16-byte loads when scores
 * is 16-byte aligned and a row is a multiple of 16 bytes, element loads otherwise; "metrics_labels" counts every
 * meant_metrics_update_labels launch.  One launch each, no workspace.
 * A null scores / pred / target / state, B < 0, C <= 0, ld < C, an unknown dtype or a misaligned operand: MEANT_ERR_ARG;
 * B >= 2^40: MEANT_ERR_UNSUPPORTED; both before any launch.  B == 0: MEANT_OK without a launch. */
int meant_metrics_update(const void* scores, int64_t ld, int dtype, const int64_t* target, int64_t B, int C, int64_t ignore_index,
                         int64_t* state, int64_t* confusion, void* stream);
int meant_metrics_update_labels(const int64_t* pred, const int64_t* target, int64_t B, int C, int64_t ignore_index,
                                int64_t* state, int64_t* confusion, void* stream);
/* ---- AUROC (the paper's third number; utils/f1_metrics.py:3 imports torchmetrics' AUROC, train.py:63-65, 103-117) ----
 * The area under the ROC curve is a rank statistic, so the scores have to be kept: meant_score_capture appends a batch's scores
 * to device buffers (one launch per step, no host read), meant_auroc_rank sorts one class's scores and counts the statistic
 * exactly, in integers.
 * meant_score_capture: scores [B, ld] (MEANT_F32 | MEANT_BF16), columns col0 .. col0 + ncol - 1 are captured; target int64 [B].
 * keys uint32 [ncol, capacity], class-major; labels int32 [capacity].  Row i of the batch goes to slot offset + i (the caller's
 * running row count: host arithmetic).  The key is the order-preserving image of the score as float32 (bf16 widened exactly):
 * -0.0 is made +0.0 first, so that the two tie, then the sign bit is flipped for a non-negative value and all bits for a negative
 * one: key order = score order, -inf lowest, +inf highest.
 *   target == ignore_index            : n_ignored += 1
 *   target otherwise outside [0, C)   : n_invalid += 1 (no address is formed from it; the scores of these two kinds are not read)
 *   one of the captured columns a NaN : n_nan += 1
 *     ... and labels[slot] = -1, the row's keys = 0: the row is left out of every statistic
 *   every other row                   : n_rows += 1, labels[slot] = target, keys[c, slot] = key of column col0 + c
 * counters int64 [4] = n_rows, n_ignored, n_invalid, n_nan (the order of the tail of the meant_metrics_update state), zeroed once
 * by the caller, only ever added to: through LDS, then one global integer atomic per non-zero counter and workgroup.
 * One launch, no workspace; route name "score_capture".
 * A null pointer, B < 0, C <= 0, ncol <= 0, col0 < 0, col0 + ncol > ld, offset < 0, offset + B > capacity, an unknown dtype or
 * a misaligned operand: MEANT_ERR_ARG; capacity >= 2^31: MEANT_ERR_UNSUPPORTED; both before any launch.  B == 0: MEANT_OK
 * without a launch. */
int meant_score_capture(const void* scores, int64_t ld, int dtype, const int64_t* target, int64_t B, int C, int col0, int ncol,
                        int64_t ignore_index, uint32_t* keys, int32_t* labels, int64_t capacity, int64_t offset, int64_t* counters,
                        void* stream);
/* meant_auroc_rank: keys uint32 [n] (one class's slice), labels int32 [n]; out int64 [3] = (2U, P, N), overwritten.
 * P = entries with labels == positive, N = the other entries with labels >= 0; entries with labels < 0 take no part.
 * 2U = sum over (positive i, negative j) of 2 [key_j < key_i] + [key_j == key_i]: the Mann-Whitney statistic with ties at one
 * half, doubled so that it is an integer.  AUROC = 2U / (2 P N); 2U <= 2 P N < 2^63.
 * How: the library's radix sort (the one behind meant_sort_ids) over (key, class) pairs by the full 32-bit key, then, with NP / PP
 * the exclusive counts of negatives / positives before an entry and start(j) the first entry of j's run of equal keys,
 *   2U = sum over positives of NP[start(j)] + sum over negatives of (P - PP[start(j)])
 * by tile sums, one scan of the sums and a pass that applies them.  No position comes from an atomic and nothing waits on
 * another workgroup; every quantity is an integer, so the result depends neither on timing nor on the order of equal keys.  The
 * only atomics are integer adds into the total 2U, one per workgroup.  Route name "auroc_rank".
 * A null out, n < 0, (n > 0:) a null keys / labels or a misaligned operand: MEANT_ERR_ARG; n >= 2^31: MEANT_ERR_UNSUPPORTED;
 * a workspace that is null or smaller than meant_auroc_ws(n) (host arithmetic; 0 for n <= 0 and n >= 2^31), n > 0:
 * MEANT_ERR_WORKSPACE; all before any launch.  workspace 16-byte aligned.  n == 0: out = (0, 0, 0). */
size_t meant_auroc_ws(int64_t n);
int meant_auroc_rank(const uint32_t* keys, const int32_t* labels, int64_t n, int positive, int64_t* out, void* workspace,
                     size_t workspace_bytes, void* stream);
/* ---- soft-target cross-entropy and the VQA score (meant_vqa's own labels) ------ vqa.py:173,209,223; utils/custom_datasets.py:214-218
 * nn.CrossEntropyLoss() (mean over the rows) of probs [B, ldp] (C valid columns, f32) against class-probability targets
 * [B, ldt] (MEANT_F32 | MEANT_BF16).  row_loss[b] = sum_c t[b,c] * (logsumexp(probs[b,:]) - probs[b,c]);
 * loss[0] = (sum_b row_loss[b]) / B, OVERWRITTEN (no zero fill by the caller); dprobs (optional, [B, ldd], must not alias probs):
 * d loss / d probs = (T_b * softmax(probs[b,:])_c - t[b,c]) / B with T_b = sum_c t[b,c].  Targets are taken as they are: rows need
 * not sum to 1 and an all-zero row contributes 0 to the loss and a zero gradient row (what torch computes).
 * Evaluated per row as mx = max p, s = sum exp(p - mx), row = T log(s) + sum_c t_c (mx - p_c), softmax_c = exp(p_c - mx) / s: no
 * term grows with a shift of the row.  Nothing at or beyond column C of a row is addressed; rows may start at any element.
 * Forms (route names): "ce_soft_wave" for C <= 1024, a wave per row; "ce_soft_block" above, a 256-thread workgroup per row, the row
 * in registers up to C = 4096 (probs and target read once, the gradient written once) and read twice beyond.  A second launch of
 * one workgroup sums row_loss in an order fixed by B.  No atomics: the same call gives the same bits, whatever "deterministic" says.
 * A null probs / target / row_loss / loss, B <= 0, C <= 0, ldp / ldt (/ ldd with dprobs) below C, an unknown target_dtype, a
 * misaligned operand or dprobs == probs: MEANT_ERR_ARG; more than 2^31 - 1 workgroups (B in the block form, B / 4 in the wave form)
 * or C within 1024 of 2^31: MEANT_ERR_UNSUPPORTED; both before any launch. */
int meant_ce_probs_soft(const float* probs, int64_t ldp, const void* target, int64_t ldt, int target_dtype,
                        float* row_loss, float* loss, float* dprobs, int64_t ldd, int64_t B, int64_t C, void* stream);
/* ---- hard-label cross-entropy with class weights, label smoothing and ignore_index ---------------------------------------------
 * torch's F.cross_entropy(x, y, weight=w, label_smoothing=eps, ignore_index=) for integer targets y int64.  weight: NULL (w_c = 1)
 * or C floats; W = sum_c w_c (C without weights); eps in [0, 1].  A row counts iff y != ignore_index && 0 <= y < C (the predicate
 * of meant_softmax_ce_fwd and meant_select_rows).  For a row that counts, with logp = log_softmax(x):
 *   row_loss = (1 - eps) w_y (-logp_y) + (eps / C) sum_c w_c (-logp_c),   row_w = w_y (the same bits),
 *   d row_loss / d x_j = (1 - eps) w_y (p_j - [j == y]) + (eps / C) (W p_j - w_j),
 * and loss = sum row_loss / sum row_w over the rows that count; 0, with zero gradients, when no row counts or the denominator is 0
 * (this library's convention, not torch's NaN).  A row that does not count has row_loss = row_w = 0 and an exact-zero gradient row;
 * its logits are never read (they may hold NaN or inf) and no address is formed from its target.  Evaluated with M = max_c x_c,
 * S = sum_c exp(x_c - M), -logp_c = log S + (M - x_c): the smoothing term is W log S + sum_c w_c (M - x_c), and no term grows with a
 * shift of the row.  A -inf logit is a masked column (probability 0) at eps == 0; with eps > 0 a -inf column is outside the contract
 * (torch gives inf or NaN there, and so may these entries).  A negative or non-finite class weight is the caller's business: the
 * entries do not look for one and compute what the formulas give.
 * stats: a device block of MEANT_CE_STATS_BYTES, 8-byte aligned, OVERWRITTEN by every call that takes one:
 *   float loss @0, float gscale = 1 / den @4 (0 if den == 0), double num @8, double den @16, int64 n_counted @24 (rows that count),
 *   int64 n_ignored @32 (y == ignore_index), int64 n_invalid @40 (every other y outside [0, C)).
 * meant_ce_hard_reduce: the block from row_loss, row_w float [T] and target int64 [T]: one workgroup, the rows that count added in
 * double in an order fixed by T (the entries of the other rows are not read).  T == 0 gives zeros.
 * meant_ce_probs_hard: the class head's form on f32 rows probs [B, ldp]: row_loss, row_w [B], dprobs (optional, [B, ldd], must not
 * alias probs) = d row_loss / d probs, NOT yet divided by the denominator (multiply by stats' gscale), and the block, in two launches.
 * Forms (route names): "ce_hard_wave" for C <= 1024, a wave per row, four rows per workgroup; "ce_hard_block" above, a 256-thread
 * workgroup per row, the row in registers up to C = 4096 (read once, the gradient written once) and read twice beyond.  Nothing at
 * or beyond column C of a row is addressed; rows may start at any element.
 * meant_softmax_ce_hard_fwd / _bwd: the large-vocabulary form on logits act [T, ld] (V <= ld valid columns, ld % 8 == 0), the shape
 * of meant_softmax_ce_fwd / _bwd, which keep serving calls without weights and smoothing.  fwd: one read of each row that counts
 * into row_loss, row_w [T] and stat float [T, 4] = (M, log S, A = (1 - eps) w_y + eps W / V, a = (1 - eps) w_y), then the block;
 * route name "ce_hard_vocab".  bwd: dlogits[t, j] = (A softmax_j - a [j == y] - (eps / V) w_j) * gscale[0] for j < V, exact zeros
 * for the padding columns and for the rows that do not count; gscale is a device scalar (d loss * the block's gscale); dlogits may
 * alias logits.  weight, when given, is read per column by the forward and the backward at eps > 0 and at the target alone otherwise.
 * No atomics in any of the four: the same call gives the same bits, whatever "deterministic" says.
 * A null pointer (weight, and dprobs, may be null), eps outside [0, 1] or not finite, B <= 0 (T < 0), C <= 0, a row stride below C,
 * ld % 8 != 0, an unknown dtype, a misaligned operand (element size; stats 8 bytes; the large-vocabulary form: logits, dlogits,
 * weight and stat 16 bytes), dprobs == probs or row_w == row_loss: MEANT_ERR_ARG; more than 2^31 - 1 workgroups (B, T; B / 4 in the
 * wave form) or C within 1024 of 2^31: MEANT_ERR_UNSUPPORTED; both before any launch. */
enum meant_ce_stats_layout { MEANT_CE_STATS_BYTES = 48 };
int meant_ce_hard_reduce(const float* row_loss, const float* row_w, const int64_t* target, int64_t T, int64_t C,
                         int64_t ignore_index, void* stats, void* stream);
int meant_ce_probs_hard(const float* probs, int64_t ldp, const int64_t* target, const float* weight, float eps,
                        int64_t ignore_index, float* row_loss, float* row_w, float* dprobs, int64_t ldd, int64_t B, int64_t C,
                        void* stats, void* stream);
int meant_softmax_ce_hard_fwd(const void* logits, int64_t ld, const int64_t* target, const float* weight, float eps, int64_t T,
                              int64_t V, int64_t ignore_index, float* row_loss, float* row_w, float* stat, void* stats, int dtype,
                              void* stream);
int meant_softmax_ce_hard_bwd(const void* logits, int64_t ld, const int64_t* target, const float* weight, float eps,
                              const float* stat, int64_t T, int64_t V, int64_t ignore_index, const float* gscale, void* dlogits,
                              int dtype, void* stream);
/* VQA score counts.  For each row: j = argmax over the C score columns in torch's order (lowest index on a tie, a NaN above
 * everything: the rule of meant_metrics_update); w = target[b, j].  scores [B, lds], target [B, ldt], each MEANT_F32 | MEANT_BF16.
 * state = int64 [4], zeroed once by the caller, only ever added to: sum_fx += llrint((double)w * 2^32), rows += 1; a row whose w is
 * not finite or outside [0, 16] is counted in state[3] (invalid) and left out of sum_fx and rows; a row with a NaN among its scores
 * is scored by the rule above and also counted in state[2].  Only integers are added: any batching and any arrival order gives the
 * same bits.  The VQA score is sum_fx / 2^32 / rows.  A wave per row over a capped grid, the four counters through LDS, one 64-bit
 * integer atomic per non-zero counter and workgroup; route name "vqa_score".
 * A null scores / target / state, B < 0, C <= 0, lds or ldt below C, an unknown dtype or a misaligned operand: MEANT_ERR_ARG;
 * B >= 2^40 or C >= 2^31: MEANT_ERR_UNSUPPORTED; both before any launch.  B == 0: MEANT_OK without a launch. */
int meant_vqa_score_update(const void* scores, int64_t lds, int scores_dtype, const void* target, int64_t ldt, int target_dtype,
                           int64_t B, int64_t C, int64_t* state, void* stream);
/* ---- pretraining collators on the device ------ utils/custom_datasets.py:41-57 (mask_tokens), :116-126 (mask_image); pretrain_mim.py:198-204
 * One masking rule, in integers, shared by the four entries below.  With fin = the two xor-shift-multiply rounds and the last
 * xor-shift of the splitmix64 finaliser:
 *   bits(seed, stream, idx)   = fin(seed + (idx | (uint64)stream << 60) * 0x9E3779B97F4A7C15)
 *   draw24(seed, stream, idx) = bits >> 40
 *   idx = sample_id * E + e   (E = elements per sample: S tokens, or C*Hh*Ww; e = position in the sample's own storage order)
 * Element e of sample sample_id is CHOSEN iff draw24(seed, 0, idx) < threshold, threshold = floor(p * 2^24) computed by the caller
 * in double (at most 2^24): the device compares integers only.  sample_id = sample_ids[row] (int64 on the device), or
 * sample_base + row with sample_ids NULL: keyed by the dataset index, a sample's mask is the same in any batch, at any batch size and
 * on any number of ranks.  sample_id * E must stay below 2^60: checked before any launch against sample_base + rows, or against
 * id_bound (the caller's exclusive bound on the values of sample_ids); beyond: MEANT_ERR_UNSUPPORTED.  No atomics in any of them.
 *
 * meant_mlm_mask: ids int64 [B, S] -> ids_out, labels int64 [B, S], one launch.  A position is open when its id is none of the
 * n_special (0..16) values of special_ids (int64 on the device) and attention_mask (optional, [B, S] of meant_mask_dtype) is not 0
 * there; an open position that the rule chooses gets labels = its id, every other position ignore_index.  A chosen position's id is
 * replaced by a second draw r = draw24(seed, 1, idx): r < t_replace: mask_id; r < t_replace + t_random: bits(seed, 2, idx) % V;
 * otherwise kept (t_replace = 2^24, t_random = 0 is utils/custom_datasets.py:56; floor(0.8 * 2^24), floor(0.1 * 2^24) the BERT
 * recipe).  ids_out may be ids itself; labels must overlap neither.  More than 2^38 tokens: MEANT_ERR_UNSUPPORTED. */
int meant_mlm_mask(const int64_t* ids, const void* attention_mask, int mask_dtype, const int64_t* sample_ids, int64_t sample_base,
                   int64_t id_bound, const int64_t* special_ids, int n_special, int64_t B, int64_t S, uint64_t seed,
                   uint32_t threshold, uint32_t t_replace, uint32_t t_random, int64_t mask_id, int64_t V, int64_t ignore_index,
                   int64_t* ids_out, int64_t* labels, void* stream);
/* meant_patchify_raw with the rule applied on load: patch element = chosen ? mask_value : ((float)x - mean) * inv_std, the draw keyed
 * by the element's (c, y, x) place in the raw image (e = (c*Hh + y)*Ww + x), not by its place in the patch row; the mask comes after
 * the normalisation, as mask_image masks the transformed tensor.  Same raw and output dtypes, any C, any p dividing Hh and Ww.  No
 * masked image is written anywhere.  threshold = 0 gives meant_patchify_raw's output. */
int meant_patchify_raw_masked(const void* images, int raw_dtype, float mean, float inv_std, void* patches, int64_t G, int C, int Hh,
                              int Ww, int p, int dtype, uint64_t seed, uint32_t threshold, const int64_t* sample_ids,
                              int64_t sample_base, int64_t id_bound, float mask_value, void* stream);
/* nn.L1Loss() of out act [B, Co, Hh, Ww] (contiguous, Co <= C: pretrain_mim.py:204 compares against labels[:, 0:3]) against the
 * labels of mask_image, regenerated per element from the same raw images [B, C, Hh, Ww] and never stored:
 *   label = chosen ? ((float)x - mean) * inv_std : unmasked_label          (unmasked_label = -100 is the reference's fill)
 * fwd: loss[0] = sum |out - label| / N with N = B*Co*Hh*Ww, and count[0] = the chosen elements among the N; both OVERWRITTEN.  A
 * workgroup owns 4096 consecutive elements and leaves one partial sum and one count in the workspace (meant_mim_l1_ws(N) bytes), a
 * second launch of one workgroup adds them in an order fixed by N (in double): two runs give the same bits.
 * bwd: dout (act, must not be out) = sign(out - label) * g[0] / N, 0 where they are equal; g is read from the device.
 * on_masked = 1 (the SimMIM form): sum and divisor cover the chosen elements only -- the divisor is count[0] clamped to at least 1,
 * which bwd reads from the count fwd wrote -- and dout is 0 elsewhere.  More than 2^40 elements: MEANT_ERR_UNSUPPORTED. */
size_t meant_mim_l1_ws(int64_t N);
int meant_mim_l1_fwd(const void* out, int dtype, const void* images, int raw_dtype, float mean, float inv_std, int64_t B, int C, int Co,
                     int Hh, int Ww, uint64_t seed, uint32_t threshold, const int64_t* sample_ids, int64_t sample_base,
                     int64_t id_bound, float unmasked_label, int on_masked, float* loss, int64_t* count, void* workspace,
                     size_t workspace_bytes, void* stream);
int meant_mim_l1_bwd(const void* out, int dtype, const void* images, int raw_dtype, float mean, float inv_std, int64_t B, int C, int Co,
                     int Hh, int Ww, uint64_t seed, uint32_t threshold, const int64_t* sample_ids, int64_t sample_base,
                     int64_t id_bound, float unmasked_label, int on_masked, const float* g, const int64_t* count, void* dout,
                     void* stream);
/* out_accum[0] += sum(x^2) over a flat float buffer (global gradient norm; caller zeroes the scalar) */
int meant_sumsq_f32(const float* x, int64_t n, float* out_accum, void* stream);
/* One AdamW step (torch.optim.AdamW semantics, `step` >= 1 for the bias corrections) over flat float buffers.
 * Gradients are read as g * grad_scale * clip with clip = min(1, max_norm / (sqrt(*sumsq) * |grad_scale| + 1e-6))
 * (torch.nn.utils.clip_grad_norm_), taken from the device scalar sumsq: no host round trip.  sumsq NULL or
 * max_norm <= 0 disables clipping. */
int meant_adamw_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int64_t step, const float* sumsq, float max_norm,
                    float grad_scale, void* stream);
/* ---- guarded optimizer tail ------ in_loop_train.py:202-239 (GradScaler, clip_grad_norm_, scaler.step / update), :548-550 (-o)
 * A second tail beside the two entries above, which stay as they are: the gradient statistics, the decision to skip a step with a
 * non-finite gradient, the step count and the loss scale live in a state block on the device, and the host reads none of them.
 * The caller owns MEANT_OPTIM_STATE_BYTES of device memory, 8-byte aligned, zero-filled once (and then, for loss scaling, its scale):
 *   offset  type    content
 *        0  double  sumsq: sum of the squares of the finite gradient elements of the step in flight
 *        8  int64   nonfinite: inf / NaN gradient elements of the step in flight
 *       16  int64   steps taken
 *       24  int64   steps skipped
 *       32  float   loss scale; a stored 0 reads as 1
 *       36  int32   growth_tracker: finite steps since the scale last changed
 *       40  float   global norm of the unscaled gradients of the last step taken, sqrt(sumsq) / scale: its clip coefficient is
 *                   min(1, max_norm / (norm + 1e-6)).  (The coefficient itself cannot be kept here: meant_optim_step_f32 must not
 *                   write the block, and meant_optim_finish is not told max_norm.)
 *       44  int32   1 when the last step was skipped, else 0
 *    48-63          reserved
 * One step: meant_grad_stats_f32 over every bucket (first != 0 on the first), meant_optim_step_f32 over every bucket,
 * meant_optim_finish once.  With data parallelism the statistics are taken from the REDUCED buckets, so every rank decides alike.
 *
 * meant_grad_stats_f32: a finite element of g [n] adds its square to sumsq, a non-finite one adds 1 to nonfinite and nothing to sumsq;
 * first != 0 overwrites the two fields (a new step), first == 0 adds to them (the next bucket).  Two launches, no atomics: every
 * span of consecutive elements (4096, more only beyond 2^28 elements: a function of n alone, never of the grid or the device) leaves
 * one double partial and one count in the workspace, then one workgroup adds the partials in an order fixed by n, in double.  The
 * same call gives the same bits on every run, whatever "deterministic" says.  16-byte loads, element loads on the n % 4 tail.
 * Unlike torch, sumsq is a DOUBLE sum of the finite squares: a norm that would overflow float32 while every element is finite
 * still clips correctly, where clip_grad_norm_ would scale such gradients to zero.  Route name "grad_stats".
 * workspace: meant_grad_stats_ws(n) bytes (host arithmetic, monotone in n, 0 for n <= 0), 16-byte aligned.
 *
 * meant_optim_step_f32: one Adam / AdamW step over flat buffers.  Reads the state and never writes it, so every bucket of a step
 * sees the same values.  nonfinite != 0: returns without storing to p, m or v.  Otherwise t = steps + 1, the bias corrections
 * 1 - beta^t computed on the device in double, inv = 1 / scale, and with max_norm > 0 the clip coefficient
 *   clip_scaled == 0:  c = min(1, max_norm / (sqrt(sumsq) * inv + 1e-6))      unscale, then clip
 *   clip_scaled != 0:  c = min(1, max_norm / (sqrt(sumsq) + 1e-6))            clip what backward left, then unscale (the reference)
 * (c = 1 with max_norm <= 0); the gradient is read as g * c * inv.  MEANT_OPTIM_ADAMW: the arithmetic of meant_adamw_f32 (decoupled
 * decay).  MEANT_OPTIM_ADAM: torch.optim.Adam, weight_decay * p added to the gradient and no decoupled decay.  Route name "optim_step".
 *
 * meant_optim_finish: one tiny launch after the last bucket.  nonfinite != 0: skipped += 1 and, with dynamic != 0, scale *=
 * backoff_factor, growth_tracker = 0.  Otherwise steps += 1 and, with dynamic != 0, torch's _amp_update_scale_: growth_tracker += 1;
 * when it reaches growth_interval (>= 1), scale *= growth_factor only if the product is finite, and growth_tracker = 0.  Writes the
 * words at offsets 40 (finite steps only) and 44.
 *
 * A null pointer, n < 0, a misaligned operand or an unknown kind: MEANT_ERR_ARG; a workspace that is too small: MEANT_ERR_WORKSPACE;
 * both before any launch.  n == 0: MEANT_OK without a launch. */
enum meant_optim_kind { MEANT_OPTIM_ADAMW = 0, MEANT_OPTIM_ADAM = 1 };
enum meant_optim_state_layout { MEANT_OPTIM_STATE_BYTES = 64 };
size_t meant_grad_stats_ws(int64_t n);
int meant_grad_stats_f32(const float* g, int64_t n, void* state, int first, void* workspace, size_t workspace_bytes, void* stream);
int meant_optim_step_f32(float* p, const float* g, float* m, float* v, int64_t n, int kind, float lr, float beta1, float beta2,
                         float eps, float weight_decay, float max_norm, int clip_scaled, const void* state, void* stream);
int meant_optim_finish(void* state, float growth_factor, float backoff_factor, int growth_interval, int dynamic, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MEANT_HIP_H */
