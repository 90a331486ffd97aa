// Library-wide plumbing: thread-local error message, version, per-device properties, runtime options and
// launch-route counters.
//
// Contract: the library is re-entrant and holds no mutable globals beyond (i) a per-DEVICE table filled
// under a mutex (CU count, which kernels already had their dynamic-LDS limit raised on that device), (ii) the option
// table (atomics, initialised once from the environment), (iii) the route counters (atomics, diagnostics only).
// Everything keyed by device is looked up with hipGetDevice() at every call: a process that drives several GPUs
// (nn.DataParallel in the reference's pretrain_mlm.py:329) gets the right state on each.
#include "common.h"
#include <stdarg.h>
#include <string.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <unordered_map>

static thread_local char g_err[512] = "";

void meant_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* meant_last_error(void) { return g_err; }

extern "C" int meant_version(void) { return 200; /* 0.2.0 */ }

// ---- per-device table ---------------------------------------------------------------------------
namespace {
struct DeviceState {
  int cus = -1;                                   // -1: not queried yet
  std::unordered_map<const void*, int> lds_raised; // kernel -> the MaxDynamicSharedMemorySize it was raised to on this device
};
std::mutex g_dev_mu;
DeviceState g_dev[MEANT_MAX_DEVICES];
}  // namespace

int meant_current_device(void) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MEANT_MAX_DEVICES) return -1;
  return dev;
}

extern "C" int meant_num_cus(void) {
  const int dev = meant_current_device();
  if (dev < 0) return 0;
  std::lock_guard<std::mutex> lock(g_dev_mu);
  DeviceState& st = g_dev[dev];
  if (st.cus < 0) {
    hipDeviceProp_t p;
    st.cus = hipGetDeviceProperties(&p, dev) == hipSuccess ? p.multiProcessorCount : 0;
  }
  return st.cus;
}

int meant_raise_dyn_lds(const void* kernel, int bytes) {
  const int dev = meant_current_device();
  MEANT_REQUIRE(dev >= 0, MEANT_ERR_LAUNCH, "no current HIP device (or device index >= %d)", MEANT_MAX_DEVICES);
  std::lock_guard<std::mutex> lock(g_dev_mu);
  DeviceState& st = g_dev[dev];
  const auto it = st.lds_raised.find(kernel);
  if (it != st.lds_raised.end() && it->second >= bytes) return MEANT_OK;    // a later, larger request raises it again
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  MEANT_REQUIRE(e == hipSuccess, MEANT_ERR_LAUNCH, "hipFuncSetAttribute(%d bytes of LDS) failed on device %d: %s", bytes, dev,
                hipGetErrorString(e));
  st.lds_raised[kernel] = bytes;
  return MEANT_OK;
}

// ---- runtime options ------------------------------------------------------------------------------
namespace {
struct OptionDef { const char* name; const char* env; int dflt; };
// order == enum meant_option_id (common.h)
const OptionDef k_options[MEANT_OPT_COUNT] = {
    {"nt_stream", "MEANT_NT_STREAM", 1},           // 0: one-tile-per-workgroup 256x256 NT kernel instead of the streaming one
    {"nt_dynamic", "MEANT_NT_DYNAMIC", 1},         // 0: fixed persistent tile walk; 1: per-XCD counters; 3: steal-only (tests)
    {"deterministic", "MEANT_DETERMINISTIC", 0},   // 1: dW / dbias, the embedding gradient (d % 8 == 0) are bit-reproducible (ordered reductions, no float atomics); the norm gains are in either mode
    {"nt_grid_cap", "MEANT_NT_GRID_CAP", 0},       // tests: cap the streaming GEMM's grid (0 = one workgroup per CU)
    {"attn_short", "MEANT_ATTN_SHORT", 1},         // 0: sequences of <= 16 tokens take the tiled flash kernels instead of attn_short.hip
    {"nt_ragged", "MEANT_NT_RAGGED", 1},           // 0: ragged M as streaming head + 128 x 128 tail launch instead of the overlapped last row tile
    {"attn_bwd1", "MEANT_ATTN_BWD1", 1},           // 0: attention backward always as two passes (dQ, then dK / dV) instead of the single-pass kernel where it applies
    {"temporal_long", "MEANT_TEMPORAL_LONG", 0},   // 1: the temporal core runs the long-lag kernels at every lag (tools/probe_temporal_lag.py's like-for-like row); 0: only for L > 64
    {"kv_skip", "MEANT_KV_SKIP", 3},               // bits: which GEMMs around a key-masked attention leave out the rows of padded key blocks (1: the k|v weight gradient, 2: the forward projection); 0: none
    {"qkv_by_id", "MEANT_QKV_BY_ID", 1},           // first text layer's projection / norm / embedding gradients once per vocabulary id (meant_qkv_embed_bwd_by_id): 0 never, 1 where tokens outnumber ids enough (the callers' rule), 2 wherever it applies
    {"qkv_fwd_by_id", "MEANT_QKV_FWD_BY_ID", 1},   // the same node's forward: norm and q|k|v projection on the table's rows, then a gather (meant_qkv_embed_fwd_by_id): 0 never, 1 where tokens outnumber ids enough (the callers' rule), 2 wherever the shape rule holds
};
// "nt_pp" (the streaming GEMM in its ping-pong form) is no longer a choice: it reads 1 and cannot be set to anything else
bool is_nt_pp(const char* name) { return name && !strcmp(name, "nt_pp"); }
std::atomic<int> g_opt[MEANT_OPT_COUNT];
std::once_flag g_opt_once;
void options_init() {
  std::call_once(g_opt_once, [] {
    for (int i = 0; i < MEANT_OPT_COUNT; ++i) {
      const char* v = getenv(k_options[i].env);
      g_opt[i].store(v && *v ? atoi(v) : k_options[i].dflt, std::memory_order_relaxed);
    }
  });
}
int option_index(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < MEANT_OPT_COUNT; ++i)
    if (!strcmp(name, k_options[i].name)) return i;
  return -1;
}
}  // namespace

int meant_opt(int id) {
  options_init();
  return g_opt[id].load(std::memory_order_relaxed);
}

extern "C" int meant_set_option(const char* name, int value) {
  options_init();
  if (is_nt_pp(name)) {
    MEANT_REQUIRE(value == 1, MEANT_ERR_UNSUPPORTED, "meant_set_option: nt_pp is always 1 (the lock-step kernel was removed)");
    return MEANT_OK;
  }
  const int i = option_index(name);
  MEANT_REQUIRE(i >= 0, MEANT_ERR_ARG, "meant_set_option: unknown option '%s'", name ? name : "(null)");
  g_opt[i].store(value, std::memory_order_relaxed);
  return MEANT_OK;
}

extern "C" int meant_get_option(const char* name, int* value) {
  options_init();
  if (is_nt_pp(name) && value) { *value = 1; return MEANT_OK; }
  const int i = option_index(name);
  MEANT_REQUIRE(i >= 0 && value, MEANT_ERR_ARG, "meant_get_option: unknown option '%s'", name ? name : "(null)");
  *value = g_opt[i].load(std::memory_order_relaxed);
  return MEANT_OK;
}

// ---- launch-route counters (diagnostics: tests assert that a shape reaches the kernel it is meant to test) ----------
namespace {
const char* const k_routes[MEANT_ROUTE_COUNT] = {
    "nt128", "nt256", "nt256s", "nt256s_rot", "nt_split", "tn128", "tn256", "tn256_det", "tn_tail", "gemm_f32",
    "attn_fwd", "attn_fwd_d128", "attn_fwd_d96", "attn_bwd", "attn_bwd_d128", "attn_bwd_d96",
    "attn_generic", "attn_cls", "attn_short", "nt_overlap", "attn_bwd1",
    "attn_fwd_d160", "attn_fwd_d192", "attn_fwd_d256", "attn_bwd_d160", "attn_bwd_d192", "attn_bwd_d256",
    "temporal_long", "emb_seg", "sort_ids", "nt128k", "nt256k", "select_rows",
    "rotary_qk", "rotary_pairs",   // every meant_rotary_qk launch; those of the pair-by-pair kernel (Dh % 8 != 0 or an unaligned base)
    "nt_rot",                       // every bf16 NT GEMM launched with the rotary epilogue, whichever nt* route it takes
    "metrics_rows", "metrics_wave", "metrics_labels",   // meant_metrics_update by form (C <= 16 / above); every meant_metrics_update_labels launch
    "tn256_rows",                   // the 256 x 256 dW kernel reducing over a list of live 64-row blocks (meant_linear_bwd_dw_rows)
    "attn_cls_split",               // every meant_attn_cls_split_fwd / _bwd call (the cls query's attention over key segments)
    "rows_elem",                    // the element-access forms of gather_rows, token_shift, geglu_fwd / _bwd and dropout (rows off the 16-byte grid)
    "score_capture", "auroc_rank",  // every meant_score_capture launch; every meant_auroc_rank call with n > 0
    "ce_soft_wave", "ce_soft_block",   // meant_ce_probs_soft by form (C <= 1024: a wave per row / above: a workgroup per row)
    "vqa_score",                    // every meant_vqa_score_update launch
    "grad_stats", "optim_step",     // every meant_grad_stats_f32 call with n > 0; every meant_optim_step_f32 launch
    "qkv_by_id",                    // every meant_qkv_embed_bwd_by_id call that runs its shared (per-id) stage
    "qkv_fwd_by_id",                // every meant_qkv_embed_fwd_by_id call
    "ce_hard_wave", "ce_hard_block",   // meant_ce_probs_hard by form (C <= 1024: a wave per row / above: a workgroup per row)
    "ce_hard_vocab",                // every meant_softmax_ce_hard_fwd launch
    "ce_probs", "softmax_ce",       // every meant_ce_probs launch; every meant_softmax_ce_fwd launch (the routes calls without options keep)
};
std::atomic<long long> g_route[MEANT_ROUTE_COUNT];
}  // namespace

void meant_route_hit(int route) { g_route[route].fetch_add(1, std::memory_order_relaxed); }
const char* meant_route_name(int route) { return k_routes[route]; }

extern "C" int64_t meant_route_count(const char* route) {
  if (!route) return -1;
  for (int i = 0; i < MEANT_ROUTE_COUNT; ++i)
    if (!strcmp(route, k_routes[i])) return (int64_t)g_route[i].load(std::memory_order_relaxed);
  return -1;
}

extern "C" void meant_route_reset(void) {
  for (int i = 0; i < MEANT_ROUTE_COUNT; ++i) g_route[i].store(0, std::memory_order_relaxed);
}
