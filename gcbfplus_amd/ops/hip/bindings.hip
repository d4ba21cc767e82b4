// Host-side launchers + pybind for the gcbfplus_amd._C extension (gfx950).
#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPException.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <mutex>

#include "crazyflie_consts.h"
#include "dw_group.h"
#include "loss_prep_envs.h"  // PrepArgs, the env structs, env_loss_prep_*_kernel decls

// kernel decls (defined in the .hip TUs)
typedef __bf16 bf16_t_;
// (the trailing const int* of the GEMM family is m_dev: null, or the device
// row count of an edge-compacted call, common.h live_rows)
template <int ACT, bool BT, int ACTIN>
__global__ void gemm_bias_act_kernel(const bf16_t_*, const bf16_t_*, const float*, bf16_t_*, const bf16_t_*, int, int, int, const int*);
template <int ACT, bool BT, int ACTIN>
__global__ void gemm_bias_act_sm_kernel(const bf16_t_*, const bf16_t_*, const float*, bf16_t_*, const bf16_t_*, int, int, int, const int*);
template <int ACT, bool BT, int NCH>
__global__ void gemm_bias_act_panel_kernel(const bf16_t_*, const bf16_t_*, const float*, bf16_t_*, int, int, int, int, const int*);
__global__ void reduce_dw_db_kernel(const float*, const float*, float*, float*, float*, long, int, int, int, int, int);
template <int ACT, typename OutT>
__global__ void gemv_bias_act_kernel(const bf16_t_*, const bf16_t_*, const float*, OutT*, int, int, int, const int*);
template <int ACT>
__global__ void dot_bias_act_kernel(const bf16_t_*, const bf16_t_*, const float*, float*, long, int, const int*);
__global__ void act_bwd_kernel(const bf16_t_*, const bf16_t_*, bf16_t_*, long, int);
template <int ACT>
__global__ void gemm_tn_partial_kernel(const bf16_t_*, const bf16_t_*, const bf16_t_*, const bool*, float*, float*, int, int, int, int, int, const int*, const int*, int);
__global__ void gemm_tn_partial_grouped_kernel(const TnPartialGroup);
__global__ void reduce_dw_db_grouped_kernel(const DwReduceGroup);
template <int ACT>
__global__ void gemm_tn_partial2_kernel(const bf16_t_*, const bf16_t_*, const bf16_t_*, float*, float*, int, int, int, int, int);
template <int ACT>
__global__ void gemm_tn_partial3_kernel(const bf16_t_*, const bf16_t_*, const bf16_t_*, const bool*, float*, float*, int, int, int, int, int, const int*, const int*, int);
template <int ACT>
__global__ void gemm_tn_partial3_map_kernel(const bf16_t_*, const bf16_t_*, const bf16_t_*, const bool*, float*, float*, int, int, int, int, int, const int*, int);
template <int ACT>
__global__ void gemm_tn_partial4_kernel(const bf16_t_*, const bf16_t_*, const bf16_t_*, float*, float*, int, int, int, int, int);
__global__ void softmax_aggr_fwd_kernel(const float*, const bf16_t_*, const bool*, bf16_t_*, float*, int, int);
__global__ void softmax_aggr_bwd_kernel(const bf16_t_*, const float*, const bf16_t_*, float*, bf16_t_*, int, int);
__global__ void edge_count_kernel(const bool*, int*, int, int);
__global__ void edge_scan_kernel(const int*, int*, int*, int, int, int);
__global__ void edge_fill_kernel(const bool*, const int*, const bool*, int*, int*, bool*, int, int);
__global__ void gather_rows_kernel(const uint4*, const int*, const int*, uint4*, long, long, int);
__global__ void gather_rows_bwd_kernel(const uint4*, const int*, uint4*, long, long, int);
typedef __bf16 bf16x8_ __attribute__((ext_vector_type(8)));
__global__ void add_rows_bf16_kernel(const bf16x8_*, const bf16x8_*, const int*, bf16x8_*, long, int);
__global__ void softmax_aggr_c_fwd_kernel(const float*, const bf16_t_*, const int*, const int*,
                                          bf16_t_*, float*, int, int, int);
__global__ void softmax_aggr_c_bwd_kernel(const bf16_t_*, const float*, const bf16_t_*, const int*,
                                          const int*, const int*, float*, bf16_t_*, int, int, int,
                                          int);
__global__ void raytrace_rect_kernel(const float*, const float*, float*, int, int, int, float);
__global__ void raytrace_sphere_topk_kernel(const float*, const float*, const float*, float*,
                                            float*, bool*, int, int,
                                            int, int, int, int, float);
__global__ void mb_gather_kernel(const float*, const bool*, const bool*, const bool*,
                                 const float*, const long*, float*, bool*, bool*, bool*,
                                 float*, int, int, int, int);
__global__ void grad_norm_sq_partial_kernel(const float*, long, float*);
__global__ void reduce_norm_kernel(const float*, int, float*);
__global__ void adamw_flat_kernel(float*, const float*, float*, float*, bf16_t_*, const float*, const int*,
                                  float, float, float, float, float, float, long);
__global__ void advance_step_kernel(int*, const float*);
template <int MAXNV, int MAXK>
__global__ void proxqp_kernel(const float*, const float*, const float*, const float*, const float*,
                              const float*, float*, int, int, int, int, float, float, float);
__global__ void edge_msg_in_fwd_kernel(const float*, bf16_t_*, int, int, int, int, int, int, float, int);
__global__ void edge_msg_in_fwd_s4_kernel(const float*, bf16_t_*, int, int, int, float);
__global__ void edge_msg_in_bwd_s4_kernel(const float*, const bf16_t_*, float*, int, int, int, float);
__global__ void edge_msg_in_bwd_kernel(const float*, const bf16_t_*, float*, int, int, int, int, int, int, float, int);
__global__ void crazyflie_edge_state_kernel(const float*, float*, long);
__global__ void edge_msg_in_fwd_cf_kernel(const float*, bf16_t_*, int, int, int, float);
__global__ void edge_msg_in_bwd_cf_kernel(const float*, const float*, const bf16_t_*, float*, int, int, int, float);
__global__ void crazyflie_edge_jac_kernel(const float*, const float*, const float*, float*, int, int, int, float);
template <int W>
__global__ void node_msg_in_fwd_kernel(const bf16_t_*, const bf16_t_*, const float*, bf16_t_*, long, int, int, int, int, int, int);
template <int W>
__global__ void node_msg_in_bwd_dx0_kernel(const bf16_t_*, bf16_t_*, long, int, int, int);
template <int W>
__global__ void node_msg_in_bwd_gather_kernel(const bf16_t_*, float*, float*, long, int, int, int, int, int);
__global__ void node_msg_in_dc_reduce_kernel(const float*, float*, long, int);
__global__ void gcbf_loss_fwd_kernel(const float*, const float*, const float*, const float*, const float*, const bool*, const bool*, float*, long, int, float, float, float, float, float, float, float);
__global__ void di_loss_prep_fwd_kernel(const float*, const float*, const float*, float*, float*,
                                        int, int, int, float, float, float, float);
__global__ void di_loss_prep_bwd_kernel(const float*, const float*, const float*, const float*,
                                        const float*, const float*, float*, int, int, int,
                                        float, float, float, float);
__global__ void crazyflie_loss_prep_fwd_kernel(const float*, const float*, const float*, float*,
                                               float*, int, int, int);
__global__ void crazyflie_loss_prep_bwd_kernel(const float*, const float*, const float*,
                                               const float*, const float*, float*, int, int,
                                               int);
template <int DYN>
__global__ void env_step2d_kernel(const float*, const float*, const float*, const float*,
                                  float*, bool*, float*, float*, int, int, int, float,
                                  float, float, float, float);
__global__ void drone3d_step_kernel(const float*, const float*, const float*, const float*,
                                    const float*, const float*, float*, bool*, float*,
                                    float*, int, int, int, float, float, float, float,
                                    float);
__global__ void crazyflie_step_kernel(const float*, const float*, const float*, const float*,
                                      const float*, float*, bool*, float*, float*, int,
                                      int, int);
__global__ void gcbf_loss_bwd_kernel(const float*, const float*, const float*, const float*, const float*, const bool*, const bool*, const float*, const float*, float*, float*, float*, float*, long, int, float, float, float, float, float, float, float);

#define CHECK_IN(x) TORCH_CHECK(x.is_cuda() && x.is_contiguous(), #x " must be contiguous on GPU")

static inline hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

static inline const bf16_t_* bfp(const torch::Tensor& t) {
  return reinterpret_cast<const bf16_t_*>(t.data_ptr<at::BFloat16>());
}
static inline bf16_t_* bfp_mut(torch::Tensor& t) {
  return reinterpret_cast<bf16_t_*>(t.data_ptr<at::BFloat16>());
}

// Optional device row count of a GEMM-family call (one int32, never read on
// the host): the kernels take min(*m_dev, M) as their M. Shapes, plans and
// grids stay those of the static M, so a captured graph replays with any count.
typedef c10::optional<torch::Tensor> MDev;
static inline const int* mdev_ptr(const MDev& m_dev) {
  if (!m_dev) return nullptr;
  TORCH_CHECK(m_dev->is_cuda() && m_dev->dtype() == torch::kInt32 && m_dev->numel() == 1,
              "m_dev must be one int32 on the GPU");
  return m_dev->data_ptr<int>();
}

// ---------------------------------------------------------------------------
// GEMM-family kernel selection. ONE host function decides, from shapes and
// the per-call env toggles, which kernel a launcher runs, its dynamic LDS
// request and (dW) the split-M geometry; the launchers below and the
// launch-free `gemm_path` query both go through it, so a test can assert
// the path a shape takes and a threshold change cannot silently leave a
// kernel uncovered.
// ---------------------------------------------------------------------------
enum GemmOp { GEMM_FWD = 0, GEMM_BT = 1, GEMM_TN = 2 };
enum GemmKernel {
  GK_DOT, GK_GEMV, GK_SM, GK_GLDS, GK_BASE,  // Y = act(X W + b) / dX = dZ W^T
  GK_TN1, GK_TN2, GK_TN3, GK_TN4                       // dW = X^T dZ partial variants
};

struct GemmPlan {
  GemmKernel kernel;
  long Kp;     // fwd: reduction length after the %32 pad (== K when unpadded)
  size_t lds;  // dynamic LDS request in bytes (0: static only)
  long gk, gn, S;  // dW: output tile grid and split-M slab count
  bool remap;      // dW: XCD-aware 1-D launch decode
  int wbufs;       // row-panel kernel: W tile buffers in LDS (2, or 1 when 2 do not fit)
  // dW through gemm_tn_defer: partial and reduce wait in the queue for the
  // grouped launches of dw_flush (tn1), or both run at once as in gemm_tn_acc.
  // Queueing the large-M (tn3) reduces as well measured 1.2% faster, inside
  // three times the run-to-run spread, and was not kept (profiles/PROFILES.md
  // "Round 5").
  bool defer;
};

// Dynamic LDS a workgroup may request on the current device, as the runtime
// reports it (64 KiB, the project's stated assumption, when there is no
// device to ask).
static size_t gemm_lds_limit() {
  static size_t cached[64] = {0};  // per device ordinal; 0 = not asked yet
  int dev = 0, v = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return 64 * 1024;
  }
  const bool slot = dev >= 0 && dev < 64;
  if (slot && cached[dev] != 0) return cached[dev];
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
      v <= 0) {
    (void)hipGetLastError();
    return 64 * 1024;
  }
  if (slot) cached[dev] = (size_t)v;
  return (size_t)v;
}

static GemmPlan gemm_plan(GemmOp op, long M, long K, long N, long actin, bool gated) {
  GemmPlan p{GK_BASE, K, 0, 0, 0, 0, false, 0};
  if (op == GEMM_TN) {
    // kernel variants: 1 = 64x64 transposed-X stage (scalar LDS writes),
    // 2 = 128x128 tile (slower: same scalar staging), 3 = dW^T orientation
    // (vector-only LDS staging; measured 154 vs 121 TF on the big training
    // shape). Shape-deterministic: 3 for large M, 1 for small/launch-bound M.
    // GCBF_TN_KERNEL overrides for experiments.
    static int forced = [] {
      const char* e = getenv("GCBF_TN_KERNEL");
      return e ? atoi(e) : 0;
    }();
    int variant = forced ? forced : (M >= 16384 ? 3 : 1);
    if (gated && (variant == 2 || variant == 4)) variant = 3;  // gate: 1/3 only
    bool big = (variant == 2 || variant == 4) && (K >= 128) && (N >= 128);
    long tk = big ? 128 : 64, tn = big ? 128 : 64;
    p.gk = (K + tk - 1) / tk;
    p.gn = (N + tn - 1) / tn;
    // deterministic split count: aim for ~1024 blocks, depends on shapes only
    long S = std::min<long>(128, std::max<long>(1, 1024 / std::max<long>(1, p.gk * p.gn)));
    // keep >= 128 rows per split so small-M dW calls don't pay 64x partial
    // traffic (S still a pure function of shapes: deterministic)
    S = std::min<long>(S, std::max<long>(1, (M + 127) / 128));
    // XCD-aware 1-D launch requires S % 8 == 0 (extra slabs see empty row
    // ranges and write zero partials — harmless, still deterministic)
    p.remap = S >= 8;
    if (p.remap) S = (S + 7) / 8 * 8;
    p.S = S;
    p.kernel = big ? (variant == 4 ? GK_TN4 : GK_TN2) : (variant == 3 ? GK_TN3 : GK_TN1);
    p.defer = p.kernel == GK_TN1;
    return p;
  }
  const size_t b_image = (size_t)(K / 8) * 64 * 8 * sizeof(uint16_t);  // [K/8][64][8]
  // row-panel kernel: [128][K] X panel, one or two [64][K] W tiles and the
  // bias (padded to whole 64-column tiles) in LDS; K/64 <= 6 instantiated
  const size_t panel = (size_t)128 * K * sizeof(uint16_t) + (size_t)((N + 63) / 64) * 64 * sizeof(float);
  const size_t wtile = (size_t)64 * K * sizeof(uint16_t);
  const int wbufs = panel + 2 * wtile <= gemm_lds_limit() ? 2 : 1;
  const bool glds_ok = M % 128 == 0 && K % 64 == 0 && getenv("GCBF_GEMM_NOGLDS") == nullptr &&
                       K <= 384 && panel + wbufs * wtile <= gemm_lds_limit();
  if (op == GEMM_FWD) {
    if (N == 1) {  // thread-per-row dot: gate / CBF head
      p.kernel = GK_DOT;
      return p;
    }
    if (N <= 16) {
      p.kernel = GK_GEMV;
      p.lds = (size_t)K * N * sizeof(uint16_t);
      return p;
    }
    if ((K % 32) != 0) {  // zero-pad K for the MFMA path, then select again
      GemmPlan q = gemm_plan(op, M, (K + 31) / 32 * 32, N, actin, gated);
      q.Kp = (K + 31) / 32 * 32;
      return q;
    }
    if (M <= 16384) {
      // small-M tile: 32x64 so mid-size layers still fill 256 CUs
      p.kernel = GK_SM;
      p.lds = b_image + 32 * 40 * sizeof(uint16_t);
    } else if (glds_ok) {
      // row-panel path: X read once, everything staged direct-to-LDS
      p.kernel = GK_GLDS;
      p.wbufs = wbufs;
      p.lds = panel + wbufs * wtile;
    } else {
      p.kernel = GK_BASE;
      p.lds = b_image + 128 * 40 * sizeof(uint16_t);
    }
    return p;
  }
  // GEMM_BT: K is the reduction dim (dZ cols), N the output width (W rows)
  if (M <= 16384) {
    p.kernel = GK_SM;
    p.lds = b_image + 32 * 40 * sizeof(uint16_t);
  } else if (actin == 0 && glds_ok) {
    p.kernel = GK_GLDS;
    p.wbufs = wbufs;
    p.lds = panel + wbufs * wtile;
  } else {
    p.kernel = GK_BASE;
    p.lds = b_image + 128 * 40 * sizeof(uint16_t);
  }
  return p;
}

static const char* gemm_kernel_name(GemmKernel k) {
  switch (k) {
    case GK_DOT: return "dot";
    case GK_GEMV: return "gemv";
    case GK_SM: return "sm";
    case GK_GLDS: return "glds";
    case GK_BASE: return "base";
    case GK_TN1: return "tn1";
    case GK_TN2: return "tn2";
    case GK_TN3: return "tn3";
    case GK_TN4: return "tn4";
  }
  return "?";
}

// Refuse a launch whose dynamic LDS request the device cannot serve: the
// runtime would reject it and the output would be uninitialised memory.
static void check_lds(const char* what, const GemmPlan& p, long M, long K, long N) {
  const size_t limit = gemm_lds_limit();
  TORCH_CHECK(p.lds <= limit, what, ": M=", M, " K=", K, " N=", N, " (", gemm_kernel_name(p.kernel),
              " kernel) needs ", p.lds, " bytes of LDS, device limit ", limit);
}

// Launch-free dispatch query: which kernel `op` ("fwd" gemm_bias_act, "bt"
// gemm_bt, "tn" gemm_tn/_acc/_acc2) runs for this shape under the current
// env toggles. fwd: "dot" | "gemv" | "sm" | "glds" | "base",
// prefixed "pad->" when K is zero-padded to %32 first; bt: the same names
// with a "_bt" suffix; tn: "tn<variant> S=<slabs> remap=<0|1>".
std::string gemm_path(const std::string& op, long M, long K, long N, long actin, bool gated) {
  TORCH_CHECK(M > 0 && K > 0 && N > 0, "gemm_path: M, K, N must be positive");
  if (op == "fwd") {
    GemmPlan p = gemm_plan(GEMM_FWD, M, K, N, 0, false);
    return std::string(p.Kp != K ? "pad->" : "") + gemm_kernel_name(p.kernel);
  }
  if (op == "bt") {
    TORCH_CHECK(K % 32 == 0, "BT path needs reduction dim % 32 == 0");
    return std::string(gemm_kernel_name(gemm_plan(GEMM_BT, M, K, N, actin, false).kernel)) + "_bt";
  }
  TORCH_CHECK(op == "tn", "gemm_path: op must be \"fwd\", \"bt\" or \"tn\"");
  GemmPlan p = gemm_plan(GEMM_TN, M, K, N, actin, gated);
  return std::string(gemm_kernel_name(p.kernel)) + " S=" + std::to_string(p.S) +
         " remap=" + (p.remap ? "1" : "0");
}

// Every path a default environment (no GCBF_* toggle set) can select, in
// `gemm_path` spelling with the dW slab count left out.
std::vector<std::string> gemm_default_paths() {
  return {"dot",   "gemv",    "sm",      "glds",         "base",         "pad->sm",
          "pad->glds", "pad->base", "sm_bt", "glds_bt", "base_bt",
          "tn1 remap=0", "tn1 remap=1", "tn3 remap=1"};
}

long gemm_lds_limit_bytes() { return (long)gemm_lds_limit(); }

// A dW call with a row map: tn3 runs the sparse-staged kernel
// (gemm_tn_partial3_map_kernel) on the same plan. The choice depends on the
// presence of a map, never on the shape; GCBF_NO_TN_SPARSE=1 (read once)
// keeps gemm_tn_partial3_kernel's map path as the in-build reference arm.
static bool tn_sparse_enabled() {
  static const bool on = [] {
    const char* e = getenv("GCBF_NO_TN_SPARSE");
    return !(e && atoi(e) != 0);
  }();
  return on;
}

// Launch-free query for a dW call through a row map of M entries:
// "tn3map S=.. remap=..", "tn3 .." under GCBF_NO_TN_SPARSE, or "tn1 ..".
std::string gemm_tn_map_path(long M, long K, long N, long actin, bool gated) {
  TORCH_CHECK(M > 0 && K > 0 && N > 0, "gemm_tn_map_path: M, K, N must be positive");
  GemmPlan p = gemm_plan(GEMM_TN, M, K, N, actin, gated);
  TORCH_CHECK(p.kernel == GK_TN1 || p.kernel == GK_TN3,
              "dW with row_map: only the tn1 and tn3 kernels take one");
  const bool sparse = p.kernel == GK_TN3 && tn_sparse_enabled();
  return std::string(sparse ? "tn3map" : gemm_kernel_name(p.kernel)) + " S=" +
         std::to_string(p.S) + " remap=" + (p.remap ? "1" : "0");
}

// Row-panel kernel launch ("glds" / "glds_bt"). Its LDS request exceeds
// 64 KiB from K = 192 on, so each instantiation raises its dynamic-LDS
// ceiling once per device: a function attribute, not a stream operation, so
// the launcher stays legal inside a stream capture.
template <int ACT, bool BT, int NCH>
static void launch_panel_nch(const GemmPlan& plan, hipStream_t stream, const bf16_t_* x,
                             const bf16_t_* w, const float* bias, bf16_t_* y, long M, long N,
                             bool wvec, const int* md) {
  static bool opted[64] = {false};  // per device ordinal
  int dev = 0;
  C10_HIP_CHECK(hipGetDevice(&dev));
  const bool slot = dev >= 0 && dev < 64;
  if (!slot || !opted[dev]) {
    C10_HIP_CHECK(hipFuncSetAttribute((const void*)gemm_bias_act_panel_kernel<ACT, BT, NCH>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)gemm_lds_limit()));
    if (slot) opted[dev] = true;
  }
  hipLaunchKernelGGL((gemm_bias_act_panel_kernel<ACT, BT, NCH>), dim3(M / 128), dim3(256),
                     plan.lds, stream, x, w, bias, y, (int)M, (int)N, plan.wbufs, (int)wvec, md);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

template <int ACT, bool BT>
static void launch_panel(const GemmPlan& plan, hipStream_t stream, const bf16_t_* x,
                         const bf16_t_* w, const float* bias, bf16_t_* y, long M, long N, long K,
                         bool wvec, const int* md) {
  switch (K / 64) {
    case 1: return launch_panel_nch<ACT, BT, 1>(plan, stream, x, w, bias, y, M, N, wvec, md);
    case 2: return launch_panel_nch<ACT, BT, 2>(plan, stream, x, w, bias, y, M, N, wvec, md);
    case 3: return launch_panel_nch<ACT, BT, 3>(plan, stream, x, w, bias, y, M, N, wvec, md);
    case 4: return launch_panel_nch<ACT, BT, 4>(plan, stream, x, w, bias, y, M, N, wvec, md);
    case 5: return launch_panel_nch<ACT, BT, 5>(plan, stream, x, w, bias, y, M, N, wvec, md);
    case 6: return launch_panel_nch<ACT, BT, 6>(plan, stream, x, w, bias, y, M, N, wvec, md);
  }
  TORCH_CHECK(false, "row-panel GEMM: no instantiation for K=", K);
}

// the caller's output buffer (tests: shows which rows a call writes), or a
// fresh one
static torch::Tensor out_or_empty(const c10::optional<torch::Tensor>& out, long M, long N,
                                  const torch::TensorOptions& opts) {
  if (!out) return torch::empty({M, N}, opts);
  TORCH_CHECK(out->is_cuda() && out->is_contiguous() && out->dim() == 2 && out->size(0) == M &&
                  out->size(1) == N && out->dtype() == opts.dtype(),
              "out must be a contiguous (M, N) tensor of the output dtype on the GPU");
  return *out;
}

// m_dev: rows >= *m_dev of y are neither computed nor written (the row-panel
// kernel works in whole 128-row panels: hand it a multiple of 128).
torch::Tensor gemm_bias_act(torch::Tensor x, torch::Tensor w, torch::Tensor bias, long act,
                            MDev m_dev = c10::nullopt,
                            c10::optional<torch::Tensor> out = c10::nullopt) {
  CHECK_IN(x);
  CHECK_IN(w);
  CHECK_IN(bias);
  TORCH_CHECK(x.dtype() == torch::kBFloat16 && w.dtype() == torch::kBFloat16);
  TORCH_CHECK(bias.dtype() == torch::kFloat32);
  long M = x.size(0), K = x.size(1), N = w.size(1);
  TORCH_CHECK(w.size(0) == K, "K mismatch");
  const int* md = mdev_ptr(m_dev);

  const GemmPlan plan = gemm_plan(GEMM_FWD, M, K, N, 0, false);
  // pad K to a multiple of 32 for the MFMA path (the gather op emits padded
  // inputs on the hot path; this is the generic fallback)
  if (plan.Kp != K) {
    TORCH_CHECK(md == nullptr && !out, "gemm_bias_act: m_dev / out need K % 32 == 0 (no pad copy)");
    long Kp = plan.Kp;
    auto xp = torch::zeros({M, Kp}, x.options());
    xp.narrow(1, 0, K).copy_(x);
    auto wp = torch::zeros({Kp, N}, w.options());
    wp.narrow(0, 0, K).copy_(w);
    return gemm_bias_act(xp, wp, bias, act);
  }
  check_lds("gemm_bias_act", plan, M, K, N);

  auto stream = cur_stream();
  const size_t smem = plan.lds;
  if (plan.kernel == GK_DOT || plan.kernel == GK_GEMV) {
    // small-N head/gate outputs come out in f32: the CBF h enters the
    // h_dot = (h_next - h)/dt finite difference where bf16 storage would
    // cancel catastrophically (bf16 ulp at |h|~1 is 0.008, signal ~0.03h)
    auto y = out_or_empty(out, M, N, x.options().dtype(torch::kFloat32));
    if (M == 0) return y;
    if (plan.kernel == GK_DOT) {  // thread-per-row dot: gate / CBF head
      dim3 grid((M + 255) / 256);
      auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, bfp(x), bfp(w),
                           bias.data_ptr<float>(), y.data_ptr<float>(), M, (int)K, md);
        C10_HIP_KERNEL_LAUNCH_CHECK();
      };
      if (act == 0) launch(dot_bias_act_kernel<0>);
      else if (act == 1) launch(dot_bias_act_kernel<1>);
      else launch(dot_bias_act_kernel<2>);
      return y;
    }
    dim3 grid((M + 3) / 4);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), smem, stream, bfp(x), bfp(w),
                         bias.data_ptr<float>(), y.data_ptr<float>(), (int)M, (int)N, (int)K, md);
      C10_HIP_KERNEL_LAUNCH_CHECK();
    };
    if (act == 0) launch(gemv_bias_act_kernel<0, float>);
    else if (act == 1) launch(gemv_bias_act_kernel<1, float>);
    else launch(gemv_bias_act_kernel<2, float>);
    return y;
  }
  auto y = out_or_empty(out, M, N, x.options());
  if (M == 0) return y;
  if (plan.kernel == GK_SM) {
    dim3 grid((M + 31) / 32, (N + 63) / 64);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), smem, stream, bfp(x), bfp(w),
                         bias.data_ptr<float>(), bfp_mut(y), (const bf16_t_*)nullptr,
                         (int)M, (int)N, (int)K, md);
      C10_HIP_KERNEL_LAUNCH_CHECK();
    };
    if (act == 0) launch(gemm_bias_act_sm_kernel<0, false, 0>);
    else if (act == 1) launch(gemm_bias_act_sm_kernel<1, false, 0>);
    else launch(gemm_bias_act_sm_kernel<2, false, 0>);
  } else if (plan.kernel == GK_GLDS) {
    // DMA of a W tile needs 16-byte-aligned rows: N % 8 == 0 and an aligned W
    const bool wvec = N % 8 == 0 && ((uintptr_t)w.data_ptr() & 15) == 0;
    if (act == 0) launch_panel<0, false>(plan, stream, bfp(x), bfp(w), bias.data_ptr<float>(), bfp_mut(y), M, N, K, wvec, md);
    else if (act == 1) launch_panel<1, false>(plan, stream, bfp(x), bfp(w), bias.data_ptr<float>(), bfp_mut(y), M, N, K, wvec, md);
    else launch_panel<2, false>(plan, stream, bfp(x), bfp(w), bias.data_ptr<float>(), bfp_mut(y), M, N, K, wvec, md);
  } else {
    dim3 grid((M + 127) / 128, (N + 63) / 64);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), smem, stream, bfp(x), bfp(w),
                         bias.data_ptr<float>(), bfp_mut(y), (const bf16_t_*)nullptr,
                         (int)M, (int)N, (int)K, md);
      C10_HIP_KERNEL_LAUNCH_CHECK();
    };
    if (act == 0) launch(gemm_bias_act_kernel<0, false, 0>);
    else if (act == 1) launch(gemm_bias_act_kernel<1, false, 0>);
    else launch(gemm_bias_act_kernel<2, false, 0>);
  }
  return y;
}

torch::Tensor act_bwd(torch::Tensor dy, torch::Tensor y, long act) {
  CHECK_IN(dy);
  CHECK_IN(y);
  if (act == 0) return dy;
  auto dz = torch::empty_like(dy);
  long n = dy.numel();
  if (n == 0) return dz;
  hipLaunchKernelGGL(act_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, cur_stream(),
                     bfp(dy), bfp(y), bfp_mut(dz), n, (int)act);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dz;
}

// (S,K,N) + (S,N) partials -> dW, db: dW blocks first (16-byte accesses when
// K*N, the partial and dW allow), then the scalar db blocks
static DwReduceProblem reduce_problem(const float* pw, const float* pb, float* dw, float* db,
                                      float* db2, long K, long N, long S, bool acc,
                                      long* nblocks) {
  const long KN = K * N;
  const bool vec = (KN & 3) == 0 && ((size_t)pw & 15) == 0 && ((size_t)dw & 15) == 0;
  const long per = vec ? 256 : 64;
  const long nbw = (KN + per - 1) / per, nbb = (N + 63) / 64;
  TORCH_CHECK(nbw + nbb <= INT_MAX, "reduce_dw_db: K*N too large");
  *nblocks = nbw + nbb;
  return DwReduceProblem{pw, pb, dw, db, db2, KN, (int)N, (int)S, acc ? 1 : 0, vec ? 1 : 0,
                         (int)nbw, 0};
}

static void launch_reduce_dw_db(const float* pw, const float* pb, float* dw, float* db,
                                float* db2, long K, long N, long S, bool acc,
                                hipStream_t stream) {
  long nb = 0;
  const DwReduceProblem r = reduce_problem(pw, pb, dw, db, db2, K, N, S, acc, &nb);
  hipLaunchKernelGGL(reduce_dw_db_kernel, dim3(nb), dim3(256), 0, stream, r.pw, r.pb, r.dW,
                     r.db, r.db2, r.KN, r.N, r.S, r.acc, r.vec, r.nbw);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// the reduction half of gemm_tn on caller-supplied partials
void reduce_dw_db(torch::Tensor partial, torch::Tensor db_partial, torch::Tensor dw,
                  torch::Tensor db, c10::optional<torch::Tensor> db2 = c10::nullopt,
                  bool acc = false) {
  auto f32 = [](const torch::Tensor& t) {
    return t.is_cuda() && t.is_contiguous() && t.dtype() == torch::kFloat32;
  };
  TORCH_CHECK(f32(partial) && f32(db_partial) && f32(dw) && f32(db));
  TORCH_CHECK(partial.dim() == 3 && db_partial.dim() == 2);
  const long S = partial.size(0), K = partial.size(1), N = partial.size(2);
  TORCH_CHECK(S >= 1 && db_partial.size(0) == S && db_partial.size(1) == N);
  TORCH_CHECK(dw.numel() == K * N && db.numel() == N);
  TORCH_CHECK(!db2 || (f32(*db2) && db2->numel() == N));
  launch_reduce_dw_db(partial.data_ptr<float>(), db_partial.data_ptr<float>(),
                      dw.data_ptr<float>(), db.data_ptr<float>(),
                      db2 ? db2->data_ptr<float>() : nullptr, K, N, S, acc, cur_stream());
}

// What gemm_tn_impl and gemm_tn_defer share: checks, plan and the partials.
struct TnCall {
  long M, K, N;
  GemmPlan plan;
  torch::Tensor partial, db_partial;  // (S, K, N), (S, N) f32
  const bf16_t_* ya;
  const bool* rg;
  const int* md;  // device row count, or null
  const int* rmap;  // dense slot row -> row of x / dz (tn_map_row), or null
  int xrows;
};

static TnCall tn_prepare(const torch::Tensor& x, const torch::Tensor& dz,
                         const torch::Tensor& yact, long actin,
                         const c10::optional<torch::Tensor>& rowgate,
                         const MDev& m_dev = c10::nullopt, const MDev& row_map = c10::nullopt) {
  CHECK_IN(x);
  CHECK_IN(dz);
  TnCall c;
  c.M = x.size(0), c.K = x.size(1), c.N = dz.size(1);
  TORCH_CHECK(dz.size(0) == c.M);
  const long xrows = c.M;
  c.rmap = nullptr;
  c.xrows = (int)xrows;
  if (row_map) {
    // M, the plan and the slabs are those of the dense rows the map covers
    TORCH_CHECK(row_map->is_cuda() && row_map->is_contiguous() &&
                    row_map->dtype() == torch::kInt32 && row_map->numel() >= 1 && !m_dev,
                "row_map must be contiguous int32 on the GPU, without m_dev");
    c.rmap = row_map->data_ptr<int>();
    c.M = row_map->numel();
  }
  c.plan = gemm_plan(GEMM_TN, c.M, c.K, c.N, actin, rowgate.has_value());
  c.md = mdev_ptr(m_dev);
  TORCH_CHECK((c.md == nullptr && c.rmap == nullptr) || c.plan.kernel == GK_TN1 ||
                  c.plan.kernel == GK_TN3,
              "dW with m_dev / row_map: only the tn1 and tn3 kernels take them");
  auto opts = x.options().dtype(torch::kFloat32);
  c.partial = torch::empty({c.plan.S, c.K, c.N}, opts);
  c.db_partial = torch::empty({c.plan.S, c.N}, opts);
  c.ya = actin ? bfp(yact) : nullptr;
  c.rg = nullptr;
  if (rowgate) {
    TORCH_CHECK(rowgate->is_contiguous() && rowgate->numel() == xrows
                && rowgate->dtype() == torch::kBool);
    c.rg = rowgate->data_ptr<bool>();
  }
  return c;
}

static void tn_launch_partial(TnCall& c, const torch::Tensor& x, const torch::Tensor& dz,
                              long actin, hipStream_t stream) {
  const GemmPlan& plan = c.plan;
  const long gk = plan.gk, gn = plan.gn, S = plan.S;
  const bool remap = plan.remap;
  const long M = c.M, N = c.N, K = c.K;
  const bf16_t_* ya = c.ya;
  const bool* rg = c.rg;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, remap ? dim3(gk * gn * S) : dim3(gk, gn, S), dim3(256), 0,
                       stream, bfp(x), bfp(dz), ya, rg, c.partial.data_ptr<float>(),
                       c.db_partial.data_ptr<float>(), (int)M, (int)N, (int)K, (int)S,
                       remap ? 1 : 0, c.md, c.rmap, c.xrows);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  };
  auto launch24 = [&](auto kernel) {  // kernels 2/4: no rowgate param
    hipLaunchKernelGGL(kernel, remap ? dim3(gk * gn * S) : dim3(gk, gn, S), dim3(256), 0,
                       stream, bfp(x), bfp(dz), ya, c.partial.data_ptr<float>(),
                       c.db_partial.data_ptr<float>(), (int)M, (int)N, (int)K, (int)S,
                       remap ? 1 : 0);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  };
  if (plan.kernel == GK_TN4) {
    if (actin == 1) launch24(gemm_tn_partial4_kernel<1>);
    else if (actin == 2) launch24(gemm_tn_partial4_kernel<2>);
    else launch24(gemm_tn_partial4_kernel<0>);
  } else if (plan.kernel == GK_TN2) {
    if (actin == 1) launch24(gemm_tn_partial2_kernel<1>);
    else if (actin == 2) launch24(gemm_tn_partial2_kernel<2>);
    else launch24(gemm_tn_partial2_kernel<0>);
  } else if (plan.kernel == GK_TN3 && c.rmap != nullptr && tn_sparse_enabled()) {
    const size_t limit = gemm_lds_limit();
    TORCH_CHECK((size_t)TN3MAP_LDS <= limit, "gemm_tn with row_map: M=", M, " K=", K, " N=", N,
                " (tn3map kernel) needs ", (size_t)TN3MAP_LDS, " bytes of LDS, device limit ", limit);
    auto launch_map = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, remap ? dim3(gk * gn * S) : dim3(gk, gn, S), dim3(256), 0,
                         stream, bfp(x), bfp(dz), ya, rg, c.partial.data_ptr<float>(),
                         c.db_partial.data_ptr<float>(), (int)M, (int)N, (int)K, (int)S,
                         remap ? 1 : 0, c.rmap, c.xrows);
      C10_HIP_KERNEL_LAUNCH_CHECK();
    };
    if (actin == 1) launch_map(gemm_tn_partial3_map_kernel<1>);
    else if (actin == 2) launch_map(gemm_tn_partial3_map_kernel<2>);
    else launch_map(gemm_tn_partial3_map_kernel<0>);
  } else if (plan.kernel == GK_TN3) {
    if (actin == 1) launch(gemm_tn_partial3_kernel<1>);
    else if (actin == 2) launch(gemm_tn_partial3_kernel<2>);
    else launch(gemm_tn_partial3_kernel<0>);
  } else {
    if (actin == 1) launch(gemm_tn_partial_kernel<1>);
    else if (actin == 2) launch(gemm_tn_partial_kernel<2>);
    else launch(gemm_tn_partial_kernel<0>);
  }
}

std::vector<torch::Tensor> gemm_tn_impl(torch::Tensor x, torch::Tensor dz,
                                        torch::Tensor yact, long actin,
                                        torch::Tensor dw, torch::Tensor db, bool acc,
                                        c10::optional<torch::Tensor> db2 = c10::nullopt,
                                        c10::optional<torch::Tensor> rowgate = c10::nullopt,
                                        MDev m_dev = c10::nullopt,
                                        MDev row_map = c10::nullopt) {
  TnCall c = tn_prepare(x, dz, yact, actin, rowgate, m_dev, row_map);
  auto stream = cur_stream();
  tn_launch_partial(c, x, dz, actin, stream);
  launch_reduce_dw_db(c.partial.data_ptr<float>(), c.db_partial.data_ptr<float>(),
                      dw.data_ptr<float>(), db.data_ptr<float>(),
                      db2 ? db2->data_ptr<float>() : nullptr, c.K, c.N, c.plan.S, acc, stream);
  return {dw, db};
}

std::vector<torch::Tensor> gemm_tn(torch::Tensor x, torch::Tensor dz, torch::Tensor yact,
                                   long actin,
                                   c10::optional<torch::Tensor> rowgate = c10::nullopt,
                                   MDev m_dev = c10::nullopt, MDev row_map = c10::nullopt) {
  auto opts = x.options().dtype(torch::kFloat32);
  auto dw = torch::empty({x.size(1), dz.size(1)}, opts);
  auto db = torch::empty({dz.size(1)}, opts);
  return gemm_tn_impl(x, dz, yact, actin, dw, db, false, c10::nullopt, rowgate, m_dev, row_map);
}

void gemm_tn_acc(torch::Tensor x, torch::Tensor dz, torch::Tensor yact, long actin,
                 torch::Tensor dw, torch::Tensor db,
                 c10::optional<torch::Tensor> rowgate = c10::nullopt,
                 MDev m_dev = c10::nullopt, MDev row_map = c10::nullopt) {
  TORCH_CHECK(dw.is_cuda() && dw.is_contiguous() && db.is_contiguous());
  TORCH_CHECK(dw.size(0) == x.size(1) && dw.size(1) == dz.size(1) && db.size(0) == dz.size(1));
  gemm_tn_impl(x, dz, yact, actin, dw, db, true, c10::nullopt, rowgate, m_dev, row_map);
}

// one-hot fold backward: dw += X^T dZ into a kernel.grad row-slice, db +=
// into BOTH bias.grad and kernel.grad[oh_row] in the same reduction pass
void gemm_tn_acc2(torch::Tensor x, torch::Tensor dz, torch::Tensor yact, long actin,
                  torch::Tensor dw, torch::Tensor db, torch::Tensor db2,
                  c10::optional<torch::Tensor> rowgate = c10::nullopt,
                  MDev m_dev = c10::nullopt, MDev row_map = c10::nullopt) {
  TORCH_CHECK(dw.is_cuda() && dw.is_contiguous() && db.is_contiguous() && db2.is_contiguous());
  TORCH_CHECK(dw.size(0) == x.size(1) && dw.size(1) == dz.size(1) && db.size(0) == dz.size(1));
  TORCH_CHECK(db2.numel() == db.numel());
  gemm_tn_impl(x, dz, yact, actin, dw, db, true, db2, rowgate, m_dev, row_map);
}

// ---------------------------------------------------------------------------
// Deferred dW. The small-M (`tn1`) dW problems of one backward do not depend
// on each other, yet as immediate calls each pays a partial launch and a
// reduce launch that do almost no work. gemm_tn_defer queues them; dw_flush
// runs the queue as grouped launches (gemm.hip), at most DW_GROUP_MAX
// problems each: every partial kernel first, then every reduce.
// The queue is process-global behind a mutex (backward of a device tensor
// runs on the autograd engine's device thread, the flush on the caller's).
// It keeps every operand, both partials and the destinations alive until the
// flush; holding dz also keeps autograd from accumulating into it in place.
// ---------------------------------------------------------------------------
struct DwEntry {
  TnPartialProblem tp;
  long tp_blocks;
  DwReduceProblem rp;
  long rp_blocks;
  std::vector<torch::Tensor> keep;
  uintptr_t dst_lo[3], dst_hi[3];  // destination byte ranges (dW, db, db2)
  int ndst;
};

static std::mutex g_dw_mutex;
static std::vector<DwEntry> g_dw_queue;
static hipStream_t g_dw_stream = nullptr;
static long g_dw_launches[2] = {0, 0};  // grouped partial, grouped reduce

// caller holds g_dw_mutex
static void dw_flush_locked() {
  if (g_dw_queue.empty()) return;
  std::vector<DwEntry> q;
  q.swap(g_dw_queue);  // a failed launch below still leaves the queue empty
  const hipStream_t stream = g_dw_stream;
  {
    TnPartialGroup g{};
    long nb = 0;
    auto fire = [&]() {
      if (g.n == 0) return;
      g.start[g.n] = (int)nb;
      hipLaunchKernelGGL(gemm_tn_partial_grouped_kernel, dim3(nb), dim3(256), 0, stream, g);
      C10_HIP_KERNEL_LAUNCH_CHECK();
      ++g_dw_launches[0];
      g = TnPartialGroup{};
      nb = 0;
    };
    for (const DwEntry& e : q) {
      g.start[g.n] = (int)nb;
      g.nblk[g.n] = (int)e.tp_blocks;
      g.p[g.n] = e.tp;
      // every problem starts at a multiple of 8, so a block's id within its
      // problem keeps deciding its XCD (tn1_decode_remap)
      nb += (e.tp_blocks + 7) / 8 * 8;
      if (++g.n == DW_GROUP_MAX) fire();
    }
    fire();
  }
  {
    DwReduceGroup g{};
    long nb = 0;
    auto fire = [&]() {
      if (g.n == 0) return;
      g.start[g.n] = (int)nb;
      hipLaunchKernelGGL(reduce_dw_db_grouped_kernel, dim3(nb), dim3(256), 0, stream, g);
      C10_HIP_KERNEL_LAUNCH_CHECK();
      ++g_dw_launches[1];
      g = DwReduceGroup{};
      nb = 0;
    };
    for (const DwEntry& e : q) {
      g.start[g.n] = (int)nb;
      g.nblk[g.n] = (int)e.rp_blocks;
      g.p[g.n] = e.rp;
      nb += e.rp_blocks;
      if (++g.n == DW_GROUP_MAX) fire();
    }
    fire();
  }
}

void dw_flush() {
  std::lock_guard<std::mutex> lock(g_dw_mutex);
  dw_flush_locked();
}

long dw_pending() {
  std::lock_guard<std::mutex> lock(g_dw_mutex);
  return (long)g_dw_queue.size();
}

std::vector<long> dw_launch_counts() {
  std::lock_guard<std::mutex> lock(g_dw_mutex);
  return {g_dw_launches[0], g_dw_launches[1]};
}

// drop the queue without running it (the deferred gradients are lost)
void dw_discard() {
  std::lock_guard<std::mutex> lock(g_dw_mutex);
  g_dw_queue.clear();
}

// gemm_tn_acc (db2 absent) / gemm_tn_acc2 with the launches deferred to
// dw_flush where the plan says so; the rest runs immediately as there.
void gemm_tn_defer(torch::Tensor x, torch::Tensor dz, torch::Tensor yact, long actin,
                   torch::Tensor dw, torch::Tensor db,
                   c10::optional<torch::Tensor> db2 = c10::nullopt,
                   c10::optional<torch::Tensor> rowgate = c10::nullopt,
                   MDev m_dev = c10::nullopt, MDev row_map = c10::nullopt) {
  auto f32 = [](const torch::Tensor& t) {
    return t.is_cuda() && t.is_contiguous() && t.dtype() == torch::kFloat32;
  };
  TORCH_CHECK(f32(dw) && f32(db), "gemm_tn_defer: dw, db must be contiguous f32 on GPU");
  TORCH_CHECK(x.dim() == 2 && dz.dim() == 2 && dw.dim() == 2);
  TORCH_CHECK(dw.size(0) == x.size(1) && dw.size(1) == dz.size(1) && db.numel() == dz.size(1));
  TORCH_CHECK(!db2 || (f32(*db2) && db2->numel() == db.numel()));
  TORCH_CHECK(x.dtype() == torch::kBFloat16 && dz.dtype() == torch::kBFloat16);
  TORCH_CHECK(actin >= 0 && actin <= 2);
  if (actin) {
    CHECK_IN(yact);
    TORCH_CHECK(yact.dtype() == torch::kBFloat16 && yact.numel() == dz.numel());
  }
  TnCall c = tn_prepare(x, dz, yact, actin, rowgate, m_dev, row_map);
  const GemmPlan& plan = c.plan;
  const hipStream_t stream = cur_stream();
  // a call with a device row count is edge-level: it runs at once, the
  // grouped kernels stay without one
  const bool defer = plan.defer && c.md == nullptr && c.rmap == nullptr;

  DwEntry e;
  e.ndst = 0;
  auto add_dst = [&](const torch::Tensor& t) {
    const uintptr_t lo = (uintptr_t)t.data_ptr<float>();
    e.dst_lo[e.ndst] = lo;
    e.dst_hi[e.ndst] = lo + (uintptr_t)t.numel() * sizeof(float);
    ++e.ndst;
  };
  add_dst(dw);
  add_dst(db);
  if (db2) add_dst(*db2);

  std::lock_guard<std::mutex> lock(g_dw_mutex);
  if (!g_dw_queue.empty()) {
    TORCH_CHECK(stream == g_dw_stream,
                "gemm_tn_defer: entries are pending on another stream; dw_flush() first");
    // accumulations into one destination keep the order of the calls
    bool overlap = false;
    for (const DwEntry& o : g_dw_queue)
      for (int i = 0; i < o.ndst; ++i)
        for (int j = 0; j < e.ndst; ++j)
          overlap |= o.dst_lo[i] < e.dst_hi[j] && e.dst_lo[j] < o.dst_hi[i];
    if (overlap) dw_flush_locked();
  }
  if (!defer) {
    tn_launch_partial(c, x, dz, actin, stream);
    launch_reduce_dw_db(c.partial.data_ptr<float>(), c.db_partial.data_ptr<float>(),
                        dw.data_ptr<float>(), db.data_ptr<float>(),
                        db2 ? db2->data_ptr<float>() : nullptr, c.K, c.N, plan.S, true, stream);
    return;
  }
  e.tp = TnPartialProblem{bfp(x), bfp(dz), c.ya, c.rg, c.partial.data_ptr<float>(),
                          c.db_partial.data_ptr<float>(), (int)c.M, (int)c.N, (int)c.K,
                          (int)plan.S, plan.remap ? 1 : 0, (int)actin, (int)plan.gk,
                          (int)plan.gn};
  e.tp_blocks = plan.gk * plan.gn * plan.S;
  e.rp = reduce_problem(c.partial.data_ptr<float>(), c.db_partial.data_ptr<float>(),
                        dw.data_ptr<float>(), db.data_ptr<float>(),
                        db2 ? db2->data_ptr<float>() : nullptr, c.K, c.N, plan.S, true,
                        &e.rp_blocks);
  e.keep = {x, dz, c.partial, c.db_partial, dw, db};
  if (actin) e.keep.push_back(yact);
  if (rowgate) e.keep.push_back(*rowgate);
  if (db2) e.keep.push_back(*db2);
  if (g_dw_queue.empty()) g_dw_stream = stream;
  g_dw_queue.push_back(std::move(e));
}


// dX = dZ @ W^T with W the original forward weight (N, K): no transpose
// copy. actin != 0 folds dZ = dY * act'(Y) into the A-operand stage (dz is
// then dY and yact the saved activation) — kills the act_bwd pass.
torch::Tensor gemm_bt(torch::Tensor dz, torch::Tensor w, torch::Tensor yact, long actin,
                      MDev m_dev = c10::nullopt,
                      c10::optional<torch::Tensor> out = c10::nullopt) {
  CHECK_IN(dz);
  CHECK_IN(w);
  const int* md = mdev_ptr(m_dev);
  TORCH_CHECK(dz.dtype() == torch::kBFloat16 && w.dtype() == torch::kBFloat16);
  long M = dz.size(0), K = dz.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "W cols must equal dZ cols");
  TORCH_CHECK(K % 32 == 0, "BT path needs reduction dim % 32 == 0");
  auto y = out_or_empty(out, M, N, dz.options());
  auto stream = cur_stream();
  static torch::Tensor zb;  // zero bias cache (per device lifetime)
  if (!zb.defined() || zb.numel() < N || zb.device() != dz.device())
    zb = torch::zeros({std::max<long>(N, 512)}, dz.options().dtype(torch::kFloat32));
  const float* bias = zb.data_ptr<float>();
  const bf16_t_* ya = actin ? bfp(yact) : nullptr;
  if (M == 0) return y;
  const GemmPlan plan = gemm_plan(GEMM_BT, M, K, N, actin, false);
  check_lds("gemm_bt", plan, M, K, N);
  const size_t smem = plan.lds;
  if (plan.kernel == GK_SM) {
    dim3 grid((M + 31) / 32, (N + 63) / 64);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), smem, stream, bfp(dz), bfp(w), bias,
                         bfp_mut(y), ya, (int)M, (int)N, (int)K, md);
      C10_HIP_KERNEL_LAUNCH_CHECK();
    };
    if (actin == 1) launch(gemm_bias_act_sm_kernel<0, true, 1>);
    else if (actin == 2) launch(gemm_bias_act_sm_kernel<0, true, 2>);
    else launch(gemm_bias_act_sm_kernel<0, true, 0>);
  } else if (plan.kernel == GK_GLDS) {
    const bool wvec = ((uintptr_t)w.data_ptr() & 15) == 0;  // rows: K % 64 == 0
    launch_panel<0, true>(plan, stream, bfp(dz), bfp(w), bias, bfp_mut(y), M, N, K, wvec, md);
  } else {
    dim3 grid((M + 127) / 128, (N + 63) / 64);
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, dim3(256), smem, stream, bfp(dz), bfp(w), bias,
                         bfp_mut(y), ya, (int)M, (int)N, (int)K, md);
      C10_HIP_KERNEL_LAUNCH_CHECK();
    };
    if (actin == 1) launch(gemm_bias_act_kernel<0, true, 1>);
    else if (actin == 2) launch(gemm_bias_act_kernel<0, true, 2>);
    else launch(gemm_bias_act_kernel<0, true, 0>);
  }
  return y;
}

void mb_gather(torch::Tensor states, torch::Tensor masks, torch::Tensor safe,
               torch::Tensor unsafe, torch::Tensor u_qp, torch::Tensor idx,
               torch::Tensor o_states, torch::Tensor o_masks, torch::Tensor o_safe,
               torch::Tensor o_unsafe, torch::Tensor o_uqp) {
  CHECK_IN(states);
  CHECK_IN(idx);
  long mb = idx.numel();
  long n_state = states.size(1) * states.size(2);
  long n_mask = masks.size(1) * masks.size(2);
  long n_flag = safe.size(1);
  long n_uqp = u_qp.size(1) * u_qp.size(2);
  TORCH_CHECK(n_state % 4 == 0 && idx.dtype() == torch::kInt64);
  hipLaunchKernelGGL(mb_gather_kernel, dim3(mb), dim3(256), 0, cur_stream(),
                     states.data_ptr<float>(), masks.data_ptr<bool>(),
                     safe.data_ptr<bool>(), unsafe.data_ptr<bool>(),
                     u_qp.data_ptr<float>(), idx.data_ptr<long>(),
                     o_states.data_ptr<float>(), o_masks.data_ptr<bool>(),
                     o_safe.data_ptr<bool>(), o_unsafe.data_ptr<bool>(),
                     o_uqp.data_ptr<float>(), (int)n_state, (int)n_mask,
                     (int)n_flag, (int)n_uqp);
}

std::vector<torch::Tensor> softmax_aggr_fwd(torch::Tensor gate, torch::Tensor msg,
                                            torch::Tensor mask) {
  CHECK_IN(gate);
  CHECK_IN(msg);
  CHECK_IN(mask);
  TORCH_CHECK(gate.dtype() == torch::kFloat32 && msg.dtype() == torch::kBFloat16);
  TORCH_CHECK(mask.dtype() == torch::kBool);
  auto sizes = gate.sizes();  // (B, N, D)
  long rows = gate.numel() / sizes.back();
  int D = sizes.back();
  int C = msg.size(-1);
  auto aggr_sizes = msg.sizes().vec();
  aggr_sizes.erase(aggr_sizes.end() - 2);  // drop D
  auto aggr = torch::empty(aggr_sizes, msg.options());
  auto attn = torch::empty_like(gate);
  size_t smem = (size_t)D * sizeof(float);
  hipLaunchKernelGGL(softmax_aggr_fwd_kernel, dim3(rows), dim3(256), smem, cur_stream(),
                     gate.data_ptr<float>(), bfp(msg), mask.data_ptr<bool>(), bfp_mut(aggr),
                     attn.data_ptr<float>(), D, C);
  return {aggr, attn};
}

std::vector<torch::Tensor> softmax_aggr_bwd(torch::Tensor daggr, torch::Tensor attn,
                                            torch::Tensor msg, torch::Tensor mask) {
  CHECK_IN(daggr);
  CHECK_IN(attn);
  CHECK_IN(msg);
  long rows = attn.numel() / attn.size(-1);
  int D = attn.size(-1);
  int C = msg.size(-1);
  auto dgate = torch::empty_like(attn);
  auto dmsg = torch::empty_like(msg);
  size_t smem = (size_t)D * sizeof(float);
  hipLaunchKernelGGL(softmax_aggr_bwd_kernel, dim3(rows), dim3(256), smem, cur_stream(),
                     bfp(daggr), attn.data_ptr<float>(), bfp(msg), dgate.data_ptr<float>(),
                     bfp_mut(dmsg), D, C);
  return {dgate, dmsg};
}

// ---------------------------------------------------------------------------
// Edge compaction (edge_compact.hip). Everything is capturable: no count is
// read on the host, outputs have the static capacity.
// ---------------------------------------------------------------------------
static inline const int* i32p(const torch::Tensor& t, const char* name, long min_numel) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dtype() == torch::kInt32 &&
                  t.numel() >= min_numel,
              name, " must be contiguous int32 on the GPU with at least ", min_numel, " elements");
  return t.data_ptr<int>();
}

// mask (..., D) bool, receivers R = numel / D -> {rows (cap,), inv (R*D,),
// off (R+1,), cnt (4,) [, gate_c (cap,) bool = gate[receiver of the row]]}:
// cnt = {count, ceil_align(count), count of the first prefix_recv receivers,
// its ceil_align}; cap = ceil_align(R*D). rows[j >= count] is unspecified.
std::vector<torch::Tensor> edge_compact(torch::Tensor mask, long align, long prefix_recv,
                                        c10::optional<torch::Tensor> gate) {
  CHECK_IN(mask);
  TORCH_CHECK(mask.dtype() == torch::kBool && mask.dim() >= 1 && mask.numel() > 0);
  TORCH_CHECK(align >= 1 && align <= 65536);
  const long D = mask.size(-1), M = mask.numel(), R = M / D;
  const long cap = (M + align - 1) / align * align;
  TORCH_CHECK(cap <= INT_MAX, "edge_compact: too many slots");
  if (prefix_recv < 0) prefix_recv = R;
  TORCH_CHECK(prefix_recv <= R, "edge_compact: prefix_recv past the receivers");
  const bool* gp = nullptr;
  if (gate) {
    TORCH_CHECK(gate->is_cuda() && gate->is_contiguous() && gate->dtype() == torch::kBool &&
                    gate->numel() == R,
                "edge_compact: gate must be one bool per receiver");
    gp = gate->data_ptr<bool>();
  }
  auto iopts = mask.options().dtype(torch::kInt32);
  auto rows = torch::empty({cap}, iopts);
  auto inv = torch::empty({M}, iopts);
  auto off = torch::empty({R + 1}, iopts);
  auto cnt = torch::empty({4}, iopts);
  auto cnt_r = torch::empty({R}, iopts);
  torch::Tensor gate_c;
  if (gate) gate_c = torch::empty({cap}, mask.options());
  auto stream = cur_stream();
  const dim3 grid((R + 3) / 4);
  hipLaunchKernelGGL(edge_count_kernel, grid, dim3(256), 0, stream, mask.data_ptr<bool>(),
                     cnt_r.data_ptr<int>(), (int)R, (int)D);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  hipLaunchKernelGGL(edge_scan_kernel, dim3(1), dim3(1024), 0, stream, cnt_r.data_ptr<int>(),
                     off.data_ptr<int>(), cnt.data_ptr<int>(), (int)R, (int)prefix_recv,
                     (int)align);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  hipLaunchKernelGGL(edge_fill_kernel, grid, dim3(256), 0, stream, mask.data_ptr<bool>(),
                     off.data_ptr<int>(), gp, rows.data_ptr<int>(), inv.data_ptr<int>(),
                     gate ? gate_c.data_ptr<bool>() : nullptr, (int)R, (int)D);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  if (gate) return {rows, inv, off, cnt, gate_c};
  return {rows, inv, off, cnt};
}

static int row_chunks16(const torch::Tensor& t, const char* who) {
  const long bytes = t.size(1) * (long)t.element_size();
  TORCH_CHECK(t.dim() == 2 && bytes % 16 == 0 && ((uintptr_t)t.data_ptr() & 15) == 0, who,
              ": rows must be whole 16-byte pieces of an aligned 2-D tensor");
  return (int)(bytes / 16);
}

// Xc (cap, K): X[rows[j]] for j < cnt[0], zeros up to cnt[1], untouched past it
torch::Tensor gather_rows(torch::Tensor X, torch::Tensor rows, torch::Tensor cnt, long cap) {
  CHECK_IN(X);
  const int chunks = row_chunks16(X, "gather_rows");
  TORCH_CHECK(cap >= 1 && cap % 8 == 0);
  const int* rp = i32p(rows, "rows", cap);
  const int* cp = i32p(cnt, "cnt", 2);
  auto Xc = torch::empty({cap, X.size(1)}, X.options());
  const long total = cap * chunks;
  hipLaunchKernelGGL(gather_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, cur_stream(),
                     (const uint4*)X.data_ptr(), rp, cp, (uint4*)Xc.data_ptr(), X.size(0), cap,
                     chunks);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return Xc;
}

// dX (M, K): dXc[inv[m]], or zeros where inv[m] < 0
torch::Tensor gather_rows_bwd(torch::Tensor dXc, torch::Tensor inv, long M) {
  CHECK_IN(dXc);
  const int chunks = row_chunks16(dXc, "gather_rows_bwd");
  const int* ip = i32p(inv, "inv", M);
  auto dX = torch::empty({M, dXc.size(1)}, dXc.options());
  const long total = M * chunks;
  if (total == 0) return dX;
  hipLaunchKernelGGL(gather_rows_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     cur_stream(), (const uint4*)dXc.data_ptr(), ip, (uint4*)dX.data_ptr(), M,
                     dXc.size(0), chunks);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dX;
}

// a + b (bf16, f32 add, one rounding) over rows < cnt[1]; other rows untouched
torch::Tensor add_rows_bf16(torch::Tensor a, torch::Tensor b, torch::Tensor cnt) {
  CHECK_IN(a);
  CHECK_IN(b);
  TORCH_CHECK(a.dtype() == torch::kBFloat16 && b.dtype() == torch::kBFloat16 &&
              a.sizes() == b.sizes());
  const int chunks = row_chunks16(a, "add_rows_bf16");
  row_chunks16(b, "add_rows_bf16");
  const int* cp = i32p(cnt, "cnt", 2);
  auto out = torch::empty_like(a);
  const long cap = a.size(0), total = cap * chunks;
  if (total == 0) return out;
  hipLaunchKernelGGL(add_rows_bf16_kernel, dim3((total + 255) / 256), dim3(256), 0, cur_stream(),
                     (const bf16x8_*)a.data_ptr(), (const bf16x8_*)b.data_ptr(), cp,
                     (bf16x8_*)out.data_ptr(), cap, chunks);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

// compact gate_c (cap,) f32, msg_c (cap, C) bf16 -> aggr (R, C) bf16, attn_c (cap,) f32
std::vector<torch::Tensor> softmax_aggr_c_fwd(torch::Tensor gate_c, torch::Tensor msg_c,
                                              torch::Tensor off, torch::Tensor inv, long D) {
  CHECK_IN(gate_c);
  CHECK_IN(msg_c);
  TORCH_CHECK(gate_c.dtype() == torch::kFloat32 && msg_c.dtype() == torch::kBFloat16);
  TORCH_CHECK(msg_c.dim() == 2 && gate_c.numel() == msg_c.size(0));
  const long R = off.numel() - 1, C = msg_c.size(1);
  TORCH_CHECK(R >= 1 && D >= 1 && R * D <= msg_c.size(0), "softmax_aggr_c_fwd: capacity");
  const int* op = i32p(off, "off", R + 1);
  const int* ip = i32p(inv, "inv", R * D);
  auto aggr = torch::empty({R, C}, msg_c.options());
  auto attn_c = torch::empty_like(gate_c);
  hipLaunchKernelGGL(softmax_aggr_c_fwd_kernel, dim3(R), dim3(256), 2 * D * sizeof(float),
                     cur_stream(), gate_c.data_ptr<float>(), bfp(msg_c), op, ip, bfp_mut(aggr),
                     attn_c.data_ptr<float>(), (int)D, (int)C, (int)msg_c.size(0));
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {aggr, attn_c};
}

// -> dgate_c (cap,) f32, dmsg_c (cap, C) bf16; rows [cnt[0], cnt[1]) zeroed
std::vector<torch::Tensor> softmax_aggr_c_bwd(torch::Tensor daggr, torch::Tensor attn_c,
                                              torch::Tensor msg_c, torch::Tensor off,
                                              torch::Tensor rows, torch::Tensor cnt, long D) {
  CHECK_IN(daggr);
  CHECK_IN(attn_c);
  CHECK_IN(msg_c);
  TORCH_CHECK(daggr.dtype() == torch::kBFloat16 && attn_c.dtype() == torch::kFloat32 &&
              msg_c.dtype() == torch::kBFloat16);
  const long R = off.numel() - 1, C = msg_c.size(1), cap = msg_c.size(0);
  TORCH_CHECK(R >= 1 && D >= 1 && R * D <= cap && attn_c.numel() == cap &&
                  daggr.numel() == R * C,
              "softmax_aggr_c_bwd: shapes");
  const int* op = i32p(off, "off", R + 1);
  const int* rp = i32p(rows, "rows", R * D);
  const int* cp = i32p(cnt, "cnt", 2);
  auto dgate_c = torch::empty_like(attn_c);
  auto dmsg_c = torch::empty_like(msg_c);
  hipLaunchKernelGGL(softmax_aggr_c_bwd_kernel, dim3(R + 1), dim3(256), 3 * D * sizeof(float),
                     cur_stream(), bfp(daggr), attn_c.data_ptr<float>(), bfp(msg_c), op, rp, cp,
                     dgate_c.data_ptr<float>(), bfp_mut(dmsg_c), (int)R, (int)D, (int)C, (int)cap);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dgate_c, dmsg_c};
}

torch::Tensor raytrace_rect(torch::Tensor pos, torch::Tensor points, long n_rays, double range) {
  CHECK_IN(pos);
  CHECK_IN(points);
  long B = pos.size(0), N = pos.size(1), K = points.size(1);
  auto hits = torch::empty({B, N, (long)n_rays, 2}, pos.options());
  size_t smem = (size_t)K * 8 * sizeof(float);
  hipLaunchKernelGGL(raytrace_rect_kernel, dim3(B), dim3(256), smem, cur_stream(),
                     pos.data_ptr<float>(), points.data_ptr<float>(), hits.data_ptr<float>(),
                     (int)N, (int)K, (int)n_rays, (float)range);
  return hits;
}

torch::Tensor raytrace_sphere_topk(torch::Tensor pos, torch::Tensor centers,
                                   torch::Tensor radii, long n_beams, long topk,
                                   double range) {
  CHECK_IN(pos);
  CHECK_IN(centers);
  CHECK_IN(radii);
  long B = pos.size(0), N = pos.size(1), K = centers.size(1);
  const int nt = (int)n_beams / 2;
  const int R = nt * (int)n_beams + 2;
  auto hits = torch::empty({B, N, topk, 3}, pos.options());
  size_t smem = ((size_t)K * 4 + ((R + 1) & ~1)) * sizeof(float)
                + 256 * sizeof(unsigned long long);
  hipLaunchKernelGGL(raytrace_sphere_topk_kernel, dim3(B * N), dim3(256), smem, cur_stream(),
                     pos.data_ptr<float>(), centers.data_ptr<float>(),
                     radii.data_ptr<float>(), hits.data_ptr<float>(),
                     (float*)nullptr, (bool*)nullptr, 0, 0,
                     (int)N, (int)K, (int)n_beams, (int)topk, (float)range);
  return hits;
}

void raytrace_sphere_graph(torch::Tensor pos, torch::Tensor centers, torch::Tensor radii,
                           torch::Tensor states_out, torch::Tensor mask_out,
                           long n_beams, long topk, double range) {
  CHECK_IN(pos);
  CHECK_IN(centers);
  CHECK_IN(radii);
  CHECK_IN(states_out);
  CHECK_IN(mask_out);
  long B = pos.size(0), N = pos.size(1), K = centers.size(1);
  long S = states_out.size(2), D = mask_out.size(2);
  const int nt = (int)n_beams / 2;
  const int R = nt * (int)n_beams + 2;
  size_t smem = ((size_t)K * 4 + ((R + 1) & ~1)) * sizeof(float)
                + 256 * sizeof(unsigned long long);
  hipLaunchKernelGGL(raytrace_sphere_topk_kernel, dim3(B * N), dim3(256), smem, cur_stream(),
                     pos.data_ptr<float>(), centers.data_ptr<float>(),
                     radii.data_ptr<float>(), (float*)nullptr,
                     states_out.data_ptr<float>(), mask_out.data_ptr<bool>(),
                     (int)S, (int)D,
                     (int)N, (int)K, (int)n_beams, (int)topk, (float)range);
}

torch::Tensor fused_adamw_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                               torch::Tensor v, torch::Tensor pbf, torch::Tensor t,
                               double lr, double b1, double b2, double eps, double wd,
                               double max_norm) {
  CHECK_IN(p);
  CHECK_IN(g);
  CHECK_IN(m);
  CHECK_IN(v);
  // a forgotten dw_flush must not drop gradients silently: the update reads g
  dw_flush();
  long n = p.numel();
  auto stream = cur_stream();
  const int nb = 256;
  auto partial = torch::empty({nb}, p.options());
  auto norm = torch::empty({1}, p.options());
  hipLaunchKernelGGL(grad_norm_sq_partial_kernel, dim3(nb), dim3(256), 0, stream,
                     g.data_ptr<float>(), n, partial.data_ptr<float>());
  hipLaunchKernelGGL(reduce_norm_kernel, dim3(1), dim3(256), 0, stream,
                     partial.data_ptr<float>(), nb, norm.data_ptr<float>());
  hipLaunchKernelGGL(adamw_flat_kernel, dim3(512), dim3(256), 0, stream,
                     p.data_ptr<float>(), g.data_ptr<float>(), m.data_ptr<float>(),
                     v.data_ptr<float>(), bfp_mut(pbf), norm.data_ptr<float>(),
                     t.data_ptr<int>(), (float)lr, (float)b1, (float)b2, (float)eps,
                     (float)wd, (float)max_norm, n);
  hipLaunchKernelGGL(advance_step_kernel, dim3(1), dim3(1), 0, stream,
                     t.data_ptr<int>(), norm.data_ptr<float>());
  return norm;
}

// K11 dispatch. ONE host function maps (nv, k) to the proxqp_kernel
// instantiation; the launcher, the launch-free `proxqp_path` query and the
// Python gate in ops/qp.py all go through it, so the limits cannot drift and
// a test can assert the path a shape takes.
enum ProxqpPath { PQ_NONE, PQ_W32X16, PQ_W64X32 };

static ProxqpPath proxqp_plan(long nv, long k) {
  if (nv < 1 || k < 0) return PQ_NONE;
  if (nv <= 32 && k <= 16) return PQ_W32X16;
  if (nv <= 64 && k <= 32) return PQ_W64X32;
  return PQ_NONE;  // caller takes the torch float64 path
}

std::string proxqp_path(long nv, long k) {
  switch (proxqp_plan(nv, k)) {
    case PQ_W32X16: return "w32x16";
    case PQ_W64X32: return "w64x32";
    default: return "none";
  }
}

torch::Tensor proxqp_solve_hip(torch::Tensor H, torch::Tensor g, torch::Tensor C,
                               torch::Tensor b, torch::Tensor l, torch::Tensor u,
                               long iters, double rho, double sigma, double alpha) {
  CHECK_IN(H);
  CHECK_IN(g);
  CHECK_IN(C);
  CHECK_IN(b);
  CHECK_IN(l);
  CHECK_IN(u);
  TORCH_CHECK(g.dim() == 2 && b.dim() == 2, "proxqp_solve_hip: g must be (M, nv), b (M, k)");
  long M = g.size(0), nv = g.size(1), k = b.size(1);
  TORCH_CHECK(H.numel() == M * nv * nv && C.numel() == M * k * nv && b.size(0) == M &&
                  l.numel() == M * nv && u.numel() == M * nv,
              "proxqp_solve_hip: operand shapes do not match M=", M, " nv=", nv, " k=", k);
  const ProxqpPath path = proxqp_plan(nv, k);
  TORCH_CHECK(path != PQ_NONE, "proxqp_solve_hip: nv=", nv, " k=", k,
              " too large for the kernel path");
  auto x = torch::empty({M, nv}, g.options());
  if (M == 0) return x;
  auto stream = cur_stream();
  if (path == PQ_W32X16) {
    hipLaunchKernelGGL((proxqp_kernel<32, 16>), dim3(M), dim3(64), 0, stream,
                       H.data_ptr<float>(), g.data_ptr<float>(), C.data_ptr<float>(),
                       b.data_ptr<float>(), l.data_ptr<float>(), u.data_ptr<float>(),
                       x.data_ptr<float>(), (int)M, (int)nv, (int)k, (int)iters,
                       (float)rho, (float)sigma, (float)alpha);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  } else {
    hipLaunchKernelGGL((proxqp_kernel<64, 32>), dim3(M), dim3(64), 0, stream,
                       H.data_ptr<float>(), g.data_ptr<float>(), C.data_ptr<float>(),
                       b.data_ptr<float>(), l.data_ptr<float>(), u.data_ptr<float>(),
                       x.data_ptr<float>(), (int)M, (int)nv, (int)k, (int)iters,
                       (float)rho, (float)sigma, (float)alpha);
    C10_HIP_KERNEL_LAUNCH_CHECK();
  }
  return x;
}

// grid of a grid-stride kernel over `total` items, 256 threads per block
static inline dim3 edge_grid(long total) {
  return dim3((unsigned)std::min<long>(std::max<long>((total + 255) / 256, 1), 1L << 20));
}

// the CrazyFlie kernels read 48 B / 64 B rows with b128 accesses
static inline bool b128_aligned(const torch::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// mode 2 (CrazyFlie) operand contract, checked before any launch
static void check_crazyflie_edge(const torch::Tensor& states, long N, long R,
                                 const char* who) {
  TORCH_CHECK(states.is_cuda() && states.is_contiguous() &&
                  states.scalar_type() == torch::kFloat32 && states.dim() == 3,
              who, ": states must be a contiguous f32 (B, V, 12) GPU tensor");
  TORCH_CHECK(states.size(2) == 12, who, ": CrazyFlie states have S == 12, got ",
              states.size(2));
  TORCH_CHECK(b128_aligned(states), who, ": states must be 16 B aligned");
  TORCH_CHECK(N >= 1 && R >= 0 && states.size(1) == 2 * N + N * R, who, ": V = ",
              states.size(1), " is not 2N + N*R for N = ", N, ", R = ", R);
}

// node pre-pass: es = edge-state transform of every node, f32 (B, V, 12).
// Allocated through torch on the current stream (capture-safe).
static torch::Tensor crazyflie_edge_states(const torch::Tensor& states) {
  auto es = torch::empty_like(states);
  long nodes = states.size(0) * states.size(1);
  if (nodes == 0) return es;
  hipLaunchKernelGGL(crazyflie_edge_state_kernel, edge_grid(nodes), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(), es.data_ptr<float>(), nodes);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return es;
}

torch::Tensor edge_msg_in_fwd(torch::Tensor states, long N, long R, long pdim, long KP,
                              double comm, long mode) {
  TORCH_CHECK(mode >= 0 && mode <= 2, "edge_msg_in_fwd: unknown mode ", mode);
  if (mode == 2) {
    check_crazyflie_edge(states, N, R, "edge_msg_in_fwd(mode 2)");
    TORCH_CHECK(pdim == 3 && KP == 32, "edge_msg_in_fwd(mode 2): needs pdim == 3 and KP == 32,"
                " got pdim = ", pdim, ", KP = ", KP);
    long B = states.size(0), D = N + 1 + R;
    auto X = torch::empty({B, N, D, KP}, states.options().dtype(torch::kBFloat16));
    long total = B * N * D;
    if (total == 0) return X;
    auto es = crazyflie_edge_states(states);
    hipLaunchKernelGGL(edge_msg_in_fwd_cf_kernel, edge_grid(total), dim3(256), 0,
                       cur_stream(), es.data_ptr<float>(), bfp_mut(X), (int)B, (int)N, (int)R,
                       (float)comm);
    C10_HIP_KERNEL_LAUNCH_CHECK();
    return X;
  }
  CHECK_IN(states);
  long B = states.size(0), V = states.size(1), S = states.size(2);
  long D = N + 1 + R;
  TORCH_CHECK(S <= 16 && KP <= 64);
  auto X = torch::empty({B, N, D, KP}, states.options().dtype(torch::kBFloat16));
  long total = B * N * D;
  if (mode == 0 && S == 4 && pdim == 2 && KP == 32) {
    hipLaunchKernelGGL(edge_msg_in_fwd_s4_kernel, dim3((total + 255) / 256), dim3(256), 0,
                       cur_stream(), states.data_ptr<float>(), bfp_mut(X), (int)B, (int)N,
                       (int)R, (float)comm);
    C10_HIP_KERNEL_LAUNCH_CHECK();
    return X;
  }
  hipLaunchKernelGGL(edge_msg_in_fwd_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(), bfp_mut(X), (int)B, (int)N,
                     (int)R, (int)S, (int)pdim, (int)KP, (float)comm, (int)mode);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return X;
}

torch::Tensor edge_msg_in_bwd(torch::Tensor states, torch::Tensor dX, long N, long R,
                              long pdim, double comm, long mode) {
  TORCH_CHECK(mode >= 0 && mode <= 2, "edge_msg_in_bwd: unknown mode ", mode);
  if (mode == 2) {
    check_crazyflie_edge(states, N, R, "edge_msg_in_bwd(mode 2)");
    long B = states.size(0), V = states.size(1), D = N + 1 + R;
    TORCH_CHECK(pdim == 3, "edge_msg_in_bwd(mode 2): needs pdim == 3, got ", pdim);
    TORCH_CHECK(dX.is_cuda() && dX.is_contiguous() && dX.scalar_type() == torch::kBFloat16 &&
                    dX.dim() == 4 && dX.size(0) == B && dX.size(1) == N && dX.size(2) == D &&
                    dX.size(3) == 32 && b128_aligned(dX),
                "edge_msg_in_bwd(mode 2): dX must be a contiguous bf16 (B, N, D, 32) GPU "
                "tensor matching the states");
    auto dstates = torch::empty_like(states);
    if (B * V == 0) return dstates;
    auto es = crazyflie_edge_states(states);
    hipLaunchKernelGGL(edge_msg_in_bwd_cf_kernel, edge_grid(B * V), dim3(256), 0,
                       cur_stream(), states.data_ptr<float>(), es.data_ptr<float>(), bfp(dX),
                       dstates.data_ptr<float>(), (int)B, (int)N, (int)R, (float)comm);
    C10_HIP_KERNEL_LAUNCH_CHECK();
    return dstates;
  }
  CHECK_IN(states);
  CHECK_IN(dX);
  long B = states.size(0), V = states.size(1), S = states.size(2);
  long KP = dX.size(-1);
  auto dstates = torch::empty_like(states);
  long total = B * V;
  if (mode == 0 && S == 4 && pdim == 2 && KP == 32) {
    hipLaunchKernelGGL(edge_msg_in_bwd_s4_kernel, dim3((total + 255) / 256), dim3(256), 0,
                       cur_stream(), states.data_ptr<float>(), bfp(dX),
                       dstates.data_ptr<float>(), (int)B, (int)N, (int)R, (float)comm);
    C10_HIP_KERNEL_LAUNCH_CHECK();
    return dstates;
  }
  hipLaunchKernelGGL(edge_msg_in_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(), bfp(dX),
                     dstates.data_ptr<float>(), (int)B, (int)N, (int)R, (int)S, (int)pdim,
                     (int)KP, (float)comm, (int)mode);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return dstates;
}

// h_x (M, N, N, 12) = dh_i / dx_j from ge (M, N, D, 12) = dh / d(edge feats)
torch::Tensor crazyflie_edge_jac(torch::Tensor states, torch::Tensor ge, long N, long R,
                                 double comm) {
  check_crazyflie_edge(states, N, R, "crazyflie_edge_jac");
  long M = states.size(0), D = N + 1 + R;
  TORCH_CHECK(ge.is_cuda() && ge.is_contiguous() && ge.scalar_type() == torch::kFloat32 &&
                  ge.dim() == 4 && ge.size(0) == M && ge.size(1) == N && ge.size(2) == D &&
                  ge.size(3) == 12 && b128_aligned(ge),
              "crazyflie_edge_jac: ge must be a contiguous f32 (M, N, D, 12) GPU tensor "
              "matching the states");
  auto hx = torch::empty({M, N, N, 12}, states.options());
  if (M == 0) return hx;
  auto es = crazyflie_edge_states(states);
  hipLaunchKernelGGL(crazyflie_edge_jac_kernel, edge_grid(M * N * N), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(), es.data_ptr<float>(),
                     ge.data_ptr<float>(), hx.data_ptr<float>(), (int)M, (int)N, (int)R,
                     (float)comm);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return hx;
}

// ---------------------------------------------------------------------------
// node_msg_in: fused GNN input of layer >= 1 (node_msg.hip). Every operand is
// checked before any launch; no host sync, no descriptor buffers (both
// directions are legal inside a stream capture).
// ---------------------------------------------------------------------------
static void check_node_msg_dims(long N, long D, long R, long E, long F, long KP0, long KP1,
                                const char* who) {
  TORCH_CHECK(N >= 1 && R >= 0 && D == N + 1 + R, who, ": D = ", D,
              " is not N + 1 + R for N = ", N, ", R = ", R);
  TORCH_CHECK(F >= 8 && F % 8 == 0, who, ": F must be a positive multiple of 8, got ", F);
  TORCH_CHECK(KP0 >= 32 && KP0 % 32 == 0, who, ": KP0 must be a multiple of 32, got ", KP0);
  TORCH_CHECK(KP1 >= 32 && KP1 % 32 == 0, who, ": KP1 must be a multiple of 32, got ", KP1);
  TORCH_CHECK(E >= 1 && E <= KP0, who, ": need 1 <= E <= KP0, got E = ", E, ", KP0 = ", KP0);
  TORCH_CHECK(E + 2 * F <= KP1 && KP1 < E + 2 * F + 32, who, ": KP1 = ", KP1,
              " is not E + 2F = ", E + 2 * F, " padded to the next multiple of 32");
  TORCH_CHECK(std::max(std::max(N, D), std::max(KP0, KP1)) <= INT_MAX, who,
              ": dimension exceeds int range");
}

static void check_node_msg_bf16(const torch::Tensor& t, const char* name, const char* who) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == torch::kBFloat16 &&
                  b128_aligned(t),
              who, ": ", name, " must be a contiguous, 16 B aligned bf16 GPU tensor");
}

torch::Tensor node_msg_in_fwd(torch::Tensor X0, torch::Tensor xa, torch::Tensor c, long E,
                              long R, long KP1) {
  const char* who = "node_msg_in_fwd";
  check_node_msg_bf16(X0, "X0", who);
  check_node_msg_bf16(xa, "xa", who);
  TORCH_CHECK(c.is_cuda() && c.is_contiguous() && c.scalar_type() == torch::kFloat32, who,
              ": c must be a contiguous f32 GPU tensor");
  TORCH_CHECK(xa.device() == X0.device() && c.device() == X0.device(), who,
              ": operands on different devices");
  TORCH_CHECK(X0.dim() == 4 && xa.dim() == 3, who, ": X0 must be (B, N, D, KP0), xa (B, N, F)");
  long B = X0.size(0), N = X0.size(1), D = X0.size(2), KP0 = X0.size(3), F = xa.size(2);
  TORCH_CHECK(xa.size(0) == B && xa.size(1) == N, who, ": xa is not (B, N, F) of X0's B, N");
  TORCH_CHECK(c.dim() == 2 && c.size(0) == 2 && c.size(1) == F, who, ": c must be (2, F)");
  check_node_msg_dims(N, D, R, E, F, KP0, KP1, who);
  auto X1 = torch::empty({B, N, D, KP1}, X0.options());
  long rows = B * N * D;
  if (rows == 0) return X1;
  long total = rows * (KP1 / 8);
  if (E % 2 == 0) {
    hipLaunchKernelGGL(node_msg_in_fwd_kernel<2>, edge_grid(total), dim3(256), 0, cur_stream(),
                       bfp(X0), bfp(xa), c.data_ptr<float>(), bfp_mut(X1), rows, (int)N,
                       (int)D, (int)E, (int)F, (int)KP0, (int)KP1);
  } else {
    hipLaunchKernelGGL(node_msg_in_fwd_kernel<1>, edge_grid(total), dim3(256), 0, cur_stream(),
                       bfp(X0), bfp(xa), c.data_ptr<float>(), bfp_mut(X1), rows, (int)N,
                       (int)D, (int)E, (int)F, (int)KP0, (int)KP1);
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return X1;
}

// dX1 (B,N,D,KP1) bf16 -> (dX0 (B,N,D,KP0) bf16, dxa (B,N,F) f32, dc (2,F) f32)
std::vector<torch::Tensor> node_msg_in_bwd(torch::Tensor dX1, long E, long F, long R,
                                           long KP0) {
  const char* who = "node_msg_in_bwd";
  check_node_msg_bf16(dX1, "dX1", who);
  TORCH_CHECK(dX1.dim() == 4, who, ": dX1 must be (B, N, D, KP1)");
  long B = dX1.size(0), N = dX1.size(1), D = dX1.size(2), KP1 = dX1.size(3);
  check_node_msg_dims(N, D, R, E, F, KP0, KP1, who);
  auto f32 = dX1.options().dtype(torch::kFloat32);
  auto dX0 = torch::empty({B, N, D, KP0}, dX1.options());
  auto dxa = torch::empty({B, N, F}, f32);
  long BN = B * N, rows = BN * D;
  if (rows == 0) return {dX0, dxa, torch::zeros({2, F}, f32)};
  auto dc = torch::empty({2, F}, f32);
  auto part = torch::empty({BN, 2, F}, f32);
  const int W = (E % 2 == 0) ? 2 : 1;
  long t0 = rows * (KP0 / 8), t1 = BN * (F / W);
  if (W == 2) {
    hipLaunchKernelGGL(node_msg_in_bwd_dx0_kernel<2>, edge_grid(t0), dim3(256), 0,
                       cur_stream(), bfp(dX1), bfp_mut(dX0), rows, (int)E, (int)KP0, (int)KP1);
    C10_HIP_KERNEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(node_msg_in_bwd_gather_kernel<2>, edge_grid(t1), dim3(256), 0,
                       cur_stream(), bfp(dX1), dxa.data_ptr<float>(), part.data_ptr<float>(),
                       BN, (int)N, (int)D, (int)E, (int)F, (int)KP1);
  } else {
    hipLaunchKernelGGL(node_msg_in_bwd_dx0_kernel<1>, edge_grid(t0), dim3(256), 0,
                       cur_stream(), bfp(dX1), bfp_mut(dX0), rows, (int)E, (int)KP0, (int)KP1);
    C10_HIP_KERNEL_LAUNCH_CHECK();
    hipLaunchKernelGGL(node_msg_in_bwd_gather_kernel<1>, edge_grid(t1), dim3(256), 0,
                       cur_stream(), bfp(dX1), dxa.data_ptr<float>(), part.data_ptr<float>(),
                       BN, (int)N, (int)D, (int)E, (int)F, (int)KP1);
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  hipLaunchKernelGGL(node_msg_in_dc_reduce_kernel, dim3((unsigned)((2 * F + 15) / 16)),
                     dim3(256), 0, cur_stream(), part.data_ptr<float>(), dc.data_ptr<float>(),
                     BN, (int)(2 * F));
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {dX0, dxa, dc};
}

torch::Tensor gcbf_loss_fwd(torch::Tensor h, torch::Tensor h_next, torch::Tensor h_ng,
                            torch::Tensor action, torch::Tensor u_qp, torch::Tensor safe,
                            torch::Tensor unsafe, double dt, double alpha, double eps,
                            double c_act, double c_unsafe, double c_safe, double c_hdot) {
  CHECK_IN(h);
  CHECK_IN(h_next);
  CHECK_IN(h_ng);
  CHECK_IN(action);
  CHECK_IN(u_qp);
  long n = h.numel();
  int nu = action.numel() / n;
  auto out = torch::empty({11}, h.options());
  hipLaunchKernelGGL(gcbf_loss_fwd_kernel, dim3(1), dim3(256), 0, cur_stream(),
                     h.data_ptr<float>(), h_next.data_ptr<float>(), h_ng.data_ptr<float>(),
                     action.data_ptr<float>(), u_qp.data_ptr<float>(),
                     safe.data_ptr<bool>(), unsafe.data_ptr<bool>(), out.data_ptr<float>(),
                     n, nu, (float)dt, (float)alpha, (float)eps, (float)c_act,
                     (float)c_unsafe, (float)c_safe, (float)c_hdot);
  return out;
}

std::vector<torch::Tensor> gcbf_loss_bwd(torch::Tensor h, torch::Tensor h_next,
                                         torch::Tensor h_ng, torch::Tensor action,
                                         torch::Tensor u_qp, torch::Tensor safe,
                                         torch::Tensor unsafe, torch::Tensor out,
                                         torch::Tensor gscale, double dt, double alpha,
                                         double eps, double c_act, double c_unsafe,
                                         double c_safe, double c_hdot) {
  long n = h.numel();
  int nu = action.numel() / n;
  auto dh = torch::empty_like(h);
  auto dh_next = torch::empty_like(h);
  auto dh_ng = torch::empty_like(h);
  auto daction = torch::empty_like(action);
  hipLaunchKernelGGL(gcbf_loss_bwd_kernel, dim3(32), dim3(256), 0, cur_stream(),
                     h.data_ptr<float>(), h_next.data_ptr<float>(), h_ng.data_ptr<float>(),
                     action.data_ptr<float>(), u_qp.data_ptr<float>(),
                     safe.data_ptr<bool>(), unsafe.data_ptr<bool>(), out.data_ptr<float>(),
                     gscale.data_ptr<float>(), dh.data_ptr<float>(),
                     dh_next.data_ptr<float>(), dh_ng.data_ptr<float>(),
                     daction.data_ptr<float>(), n, nu, (float)dt, (float)alpha, (float)eps,
                     (float)c_act, (float)c_unsafe, (float)c_safe, (float)c_hdot);
  return {dh, dh_next, dh_ng, daction};
}

std::vector<torch::Tensor> di_env_step(torch::Tensor states, torch::Tensor action,
                                       torch::Tensor points, torch::Tensor Kmat, long N,
                                       long R, double dt, double inv_m, double comm,
                                       double car_r, double vmax, long dyn) {
  CHECK_IN(states);
  CHECK_IN(action);
  CHECK_IN(points);
  CHECK_IN(Kmat);
  long B = states.size(0), V = states.size(1), K = points.size(1);
  long D = N + 1 + R;
  auto nxt = torch::empty_like(states);
  auto mask = torch::empty({B, N, D}, states.options().dtype(torch::kBool));
  auto reward = torch::empty({B}, states.options());
  auto cost = torch::empty({B}, states.options());
  size_t smem = (size_t)(N * 4 + N * 2 + K * 8) * sizeof(float);
  if (dyn == 0)
    hipLaunchKernelGGL(env_step2d_kernel<0>, dim3(B), dim3(256), smem, cur_stream(),
                       states.data_ptr<float>(), action.data_ptr<float>(),
                       points.data_ptr<float>(), Kmat.data_ptr<float>(),
                       nxt.data_ptr<float>(), mask.data_ptr<bool>(),
                       reward.data_ptr<float>(), cost.data_ptr<float>(), (int)N, (int)K,
                       (int)R, (float)dt, (float)inv_m, (float)comm, (float)car_r,
                       (float)vmax);
  else
    hipLaunchKernelGGL(env_step2d_kernel<1>, dim3(B), dim3(256), smem, cur_stream(),
                       states.data_ptr<float>(), action.data_ptr<float>(),
                       points.data_ptr<float>(), Kmat.data_ptr<float>(),
                       nxt.data_ptr<float>(), mask.data_ptr<bool>(),
                       reward.data_ptr<float>(), cost.data_ptr<float>(), (int)N, (int)K,
                       (int)R, (float)dt, (float)inv_m, (float)comm, (float)car_r,
                       (float)vmax);
  return {nxt, mask, reward, cost};
}

std::vector<torch::Tensor> drone3d_step(torch::Tensor states, torch::Tensor action,
                                        torch::Tensor centers, torch::Tensor radii,
                                        torch::Tensor Kmat, torch::Tensor Amat, long N,
                                        long R, double dt, double bgain, double comm,
                                        double drone_r, double vmax) {
  CHECK_IN(states);
  CHECK_IN(action);
  CHECK_IN(centers);
  CHECK_IN(radii);
  CHECK_IN(Kmat);
  CHECK_IN(Amat);
  long B = states.size(0), K = centers.size(1);
  long D = N + 1 + R;
  auto nxt = torch::empty_like(states);
  auto mask = torch::empty({B, N, D}, states.options().dtype(torch::kBool));
  auto reward = torch::empty({B}, states.options());
  auto cost = torch::empty({B}, states.options());
  size_t smem = (size_t)(N * 6 + N * 3 + K * 4) * sizeof(float);
  hipLaunchKernelGGL(drone3d_step_kernel, dim3(B), dim3(256), smem, cur_stream(),
                     states.data_ptr<float>(), action.data_ptr<float>(),
                     centers.data_ptr<float>(), radii.data_ptr<float>(),
                     Kmat.data_ptr<float>(), Amat.data_ptr<float>(),
                     nxt.data_ptr<float>(), mask.data_ptr<bool>(),
                     reward.data_ptr<float>(), cost.data_ptr<float>(), (int)N, (int)K,
                     (int)R, (float)dt, (float)bgain, (float)comm, (float)drone_r,
                     (float)vmax);
  return {nxt, mask, reward, cost};
}

// LDS request of crazyflie_step for N agents / K spheres fits the default
// per-workgroup limit (env.step falls back to the eager path otherwise)
bool crazyflie_step_fits(long N, long K) {
  return crazyflie_step_lds_bytes(N, K) <= CF_LDS_LIMIT;
}

std::vector<torch::Tensor> crazyflie_step(torch::Tensor states, torch::Tensor action,
                                          torch::Tensor centers, torch::Tensor radii,
                                          torch::Tensor consts, long N, long R) {
  CHECK_IN(states);
  CHECK_IN(action);
  CHECK_IN(centers);
  CHECK_IN(radii);
  CHECK_IN(consts);
  TORCH_CHECK(states.dim() == 3 && N > 0 && R >= 0 && states.size(1) == 2 * N + N * R &&
                  states.size(2) == 12,
              "states must be (B, 2N + N*R, 12)");
  long B = states.size(0), K = centers.size(1);
  TORCH_CHECK(action.dim() == 3 && action.size(0) == B && action.size(1) == N &&
                  action.size(2) == 4,
              "action must be (B, N, 4)");
  TORCH_CHECK(centers.dim() == 3 && centers.size(0) == B && centers.size(2) == 3 &&
                  radii.dim() == 2 && radii.size(0) == B && radii.size(1) == K,
              "centers must be (B, K, 3) and radii (B, K)");
  TORCH_CHECK(consts.numel() == CF_NCONST, "consts must hold ", (int)CF_NCONST, " floats");
  TORCH_CHECK(crazyflie_step_fits(N, K), "crazyflie_step: N=", N, " K=", K, " needs ",
              crazyflie_step_lds_bytes(N, K), " bytes of LDS, limit ", CF_LDS_LIMIT);
  long D = N + 1 + R;
  auto nxt = torch::empty_like(states);
  auto mask = torch::empty({B, N, D}, states.options().dtype(torch::kBool));
  auto reward = torch::empty({B}, states.options());
  auto cost = torch::empty({B}, states.options());
  if (B == 0) return {nxt, mask, reward, cost};
  hipLaunchKernelGGL(crazyflie_step_kernel, dim3(B), dim3(256),
                     crazyflie_step_lds_bytes(N, K), cur_stream(),
                     states.data_ptr<float>(), action.data_ptr<float>(),
                     centers.data_ptr<float>(), radii.data_ptr<float>(),
                     consts.data_ptr<float>(), nxt.data_ptr<float>(),
                     mask.data_ptr<bool>(), reward.data_ptr<float>(),
                     cost.data_ptr<float>(), (int)N, (int)K, (int)R);
  return {nxt, mask, reward, cost};
}

std::vector<torch::Tensor> di_loss_prep_fwd(torch::Tensor states, torch::Tensor raw,
                                            torch::Tensor Kmat, long N, double dt,
                                            double inv_m, double comm, double vmax) {
  CHECK_IN(states);
  CHECK_IN(raw);
  long B = states.size(0), V = states.size(1);
  auto action = torch::empty({B, N, 2}, states.options());
  auto big = torch::empty({2 * B, V, 4}, states.options());
  long rows = 2 * B * V;
  hipLaunchKernelGGL(di_loss_prep_fwd_kernel, dim3((rows + 255) / 256), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(), raw.data_ptr<float>(),
                     Kmat.data_ptr<float>(), action.data_ptr<float>(), big.data_ptr<float>(),
                     (int)B, (int)V, (int)N, (float)dt, (float)inv_m, (float)comm,
                     (float)vmax);
  return {action, big};
}

torch::Tensor di_loss_prep_bwd(torch::Tensor states, torch::Tensor raw, torch::Tensor Kmat,
                               torch::Tensor action, torch::Tensor daction,
                               torch::Tensor dbig, long N, double dt, double inv_m,
                               double comm, double vmax) {
  long B = states.size(0), V = states.size(1);
  auto draw = torch::empty_like(raw);
  long total = B * N;
  hipLaunchKernelGGL(di_loss_prep_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(), raw.data_ptr<float>(),
                     Kmat.data_ptr<float>(), action.data_ptr<float>(),
                     daction.data_ptr<float>(), dbig.data_ptr<float>(),
                     draw.data_ptr<float>(), (int)B, (int)V, (int)N, (float)dt,
                     (float)inv_m, (float)comm, (float)vmax);
  return draw;
}

// CrazyFlie loss prologue: contiguous f32 on the GPU, shapes that the kernels
// index by, the whole constant block
// (rows are moved as float4: 16-byte aligned base)
#define CHECK_F32(x) \
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.scalar_type() == torch::kFloat32 && \
                  reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, \
              #x " must be a contiguous, 16-byte aligned float32 GPU tensor")

static void crazyflie_loss_prep_check(const torch::Tensor& states, const torch::Tensor& consts,
                                      long N) {
  CHECK_F32(states);
  CHECK_F32(consts);
  TORCH_CHECK(states.dim() == 3 && states.size(2) == 12, "states must be (B, V, 12)");
  TORCH_CHECK(N > 0 && states.size(1) >= 2 * N, "states must hold N agent and N goal rows");
  TORCH_CHECK(consts.numel() == CF_NCONST, "consts must hold ", (int)CF_NCONST, " floats");
  TORCH_CHECK(consts.device() == states.device(), "consts must be on the device of states");
  TORCH_CHECK(states.size(0) <= INT_MAX / 2 && states.size(1) <= INT_MAX,
              "states batch too large");
}

static void crazyflie_loss_prep_check_bn4(const torch::Tensor& t, const char* name,
                                          const torch::Tensor& states, long N) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == torch::kFloat32 &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, " must be a contiguous, 16-byte aligned float32 GPU tensor");
  TORCH_CHECK(t.dim() == 3 && t.size(0) == states.size(0) && t.size(1) == N && t.size(2) == 4,
              name, " must be (B, N, 4)");
  TORCH_CHECK(t.device() == states.device(), name, " must be on the device of states");
}

std::vector<torch::Tensor> crazyflie_loss_prep_fwd(torch::Tensor states, torch::Tensor raw,
                                                   torch::Tensor consts, long N) {
  crazyflie_loss_prep_check(states, consts, N);
  crazyflie_loss_prep_check_bn4(raw, "raw", states, N);
  long B = states.size(0), V = states.size(1);
  auto action = torch::empty({B, N, 4}, states.options());
  auto big = torch::empty({2 * B, V, 12}, states.options());
  long rows = 2 * B * V;
  if (rows == 0) return {action, big};
  hipLaunchKernelGGL(crazyflie_loss_prep_fwd_kernel, dim3((rows + 255) / 256), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(), raw.data_ptr<float>(),
                     consts.data_ptr<float>(), action.data_ptr<float>(),
                     big.data_ptr<float>(), (int)B, (int)V, (int)N);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {action, big};
}

torch::Tensor crazyflie_loss_prep_bwd(torch::Tensor states, torch::Tensor consts,
                                      torch::Tensor action, torch::Tensor daction,
                                      torch::Tensor dbig, long N) {
  crazyflie_loss_prep_check(states, consts, N);
  crazyflie_loss_prep_check_bn4(action, "action", states, N);
  crazyflie_loss_prep_check_bn4(daction, "daction", states, N);
  CHECK_F32(dbig);
  long B = states.size(0), V = states.size(1);
  TORCH_CHECK(dbig.dim() == 3 && dbig.size(0) == 2 * B && dbig.size(1) == V &&
                  dbig.size(2) == 12 && dbig.device() == states.device(),
              "dbig must be (2B, V, 12) on the device of states");
  auto draw = torch::empty_like(action);
  long total = B * N * 4;
  if (total == 0) return draw;
  hipLaunchKernelGGL(crazyflie_loss_prep_bwd_kernel, dim3((total + 255) / 256), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(), consts.data_ptr<float>(),
                     action.data_ptr<float>(), daction.data_ptr<float>(),
                     dbig.data_ptr<float>(), draw.data_ptr<float>(), (int)B, (int)V, (int)N);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return draw;
}

// DubinsCar / LinearDrone / SingleIntegrator loss prologue (env struct E of
// loss_prep_envs.h). Every check runs before the launch.
static void env_prep_check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == torch::kFloat32 &&
                  reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
              name, " must be a contiguous, 16-byte aligned float32 GPU tensor");
}

static void env_prep_check_mat(const torch::Tensor& t, const char* name,
                               const torch::Tensor& states, long r, long c) {
  env_prep_check_f32(t, name);
  TORCH_CHECK(t.dim() == 2 && t.size(0) == r && t.size(1) == c, name, " must be (", r, ", ", c,
              ")");
  TORCH_CHECK(t.device() == states.device(), name, " must be on the device of states");
}

template <class E>
static void env_prep_check_bnu(const torch::Tensor& t, const char* name,
                               const torch::Tensor& states, long N) {
  env_prep_check_f32(t, name);
  TORCH_CHECK(t.dim() == 3 && t.size(0) == states.size(0) && t.size(1) == N &&
                  t.size(2) == E::NU,
              name, " must be (B, N, ", (int)E::NU, ")");
  TORCH_CHECK(t.device() == states.device(), name, " must be on the device of states");
}

// states (B, V, S) with N agent and N goal rows, the limits, dt and comm
template <class E>
static typename E::Args env_prep_args(const torch::Tensor& states, long N, double dt,
                                      double comm, const std::vector<double>& act_lo,
                                      const std::vector<double>& act_hi,
                                      const std::vector<double>& st_lo,
                                      const std::vector<double>& st_hi) {
  env_prep_check_f32(states, "states");
  TORCH_CHECK(states.dim() == 3 && states.size(2) == E::S, "states must be (B, V, ", (int)E::S,
              ")");
  TORCH_CHECK(N > 0 && states.size(1) >= 2 * N, "states must hold N agent and N goal rows");
  TORCH_CHECK(states.size(0) <= INT_MAX / 2 && states.size(1) <= INT_MAX,
              "states batch too large");
  TORCH_CHECK((long)act_lo.size() == E::NU && (long)act_hi.size() == E::NU,
              "action limits must hold ", (int)E::NU, " values each");
  TORCH_CHECK((long)st_lo.size() == E::S && (long)st_hi.size() == E::S,
              "state limits must hold ", (int)E::S, " values each");
  typename E::Args p;
  for (int c = 0; c < E::NU; ++c) p.alo[c] = (float)act_lo[c], p.ahi[c] = (float)act_hi[c];
  for (int s = 0; s < E::S; ++s) p.slo[s] = (float)st_lo[s], p.shi[s] = (float)st_hi[s];
  p.dt = (float)dt;
  p.comm = (float)comm;
  p.stop_r = -1.f;
  p.K = p.A = p.Bm = nullptr;
  return p;
}

template <class E>
static std::vector<torch::Tensor> env_loss_prep_fwd(const torch::Tensor& states,
                                                    const torch::Tensor& raw, long N,
                                                    const typename E::Args& p) {
  env_prep_check_bnu<E>(raw, "raw", states, N);
  long B = states.size(0), V = states.size(1);
  torch::Tensor action = torch::empty({B, N, E::NU}, states.options());
  torch::Tensor big = torch::empty({2 * B, V, E::S}, states.options());
  long rows = 2 * B * V;
  if (rows == 0) return {action, big};
  // two trips of the grid-stride loop per thread: most rows are 8- to 24-byte
  // copies, and half the blocks move them just as well
  hipLaunchKernelGGL(env_loss_prep_fwd_kernel<E>, dim3((rows + 511) / 512), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(), raw.data_ptr<float>(),
                     action.data_ptr<float>(), big.data_ptr<float>(), (int)B, (int)V, (int)N,
                     p);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return {action, big};
}

template <class E>
static torch::Tensor env_loss_prep_bwd(const torch::Tensor& states, const torch::Tensor& action,
                                       const torch::Tensor& daction, const torch::Tensor& dbig,
                                       long N, const typename E::Args& p) {
  env_prep_check_bnu<E>(action, "action", states, N);
  env_prep_check_bnu<E>(daction, "daction", states, N);
  env_prep_check_f32(dbig, "dbig");
  long B = states.size(0), V = states.size(1);
  TORCH_CHECK(dbig.dim() == 3 && dbig.size(0) == 2 * B && dbig.size(1) == V &&
                  dbig.size(2) == E::S && dbig.device() == states.device(),
              "dbig must be (2B, V, ", (int)E::S, ") on the device of states");
  auto draw = torch::empty_like(action);
  long total = B * N;
  if (total == 0) return draw;
  hipLaunchKernelGGL(env_loss_prep_bwd_kernel<E>, dim3((total + 255) / 256), dim3(256), 0,
                     cur_stream(), states.data_ptr<float>(), action.data_ptr<float>(),
                     daction.data_ptr<float>(), dbig.data_ptr<float>(),
                     draw.data_ptr<float>(), (int)B, (int)V, (int)N, p);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return draw;
}

typedef std::vector<double> Lim;

static DubinsPrep::Args dubins_prep_args(const torch::Tensor& states, long N, double dt,
                                         double comm, double stop_r, bool enable_stop,
                                         const Lim& alo, const Lim& ahi, const Lim& slo,
                                         const Lim& shi) {
  auto p = env_prep_args<DubinsPrep>(states, N, dt, comm, alo, ahi, slo, shi);
  TORCH_CHECK(stop_r >= 0, "stop_r must not be negative");
  p.stop_r = enable_stop ? (float)stop_r : -1.f;
  return p;
}

std::vector<torch::Tensor> dubins_loss_prep_fwd(torch::Tensor states, torch::Tensor raw, long N,
                                                double dt, double comm, double stop_r,
                                                bool enable_stop, Lim alo, Lim ahi, Lim slo,
                                                Lim shi) {
  auto p = dubins_prep_args(states, N, dt, comm, stop_r, enable_stop, alo, ahi, slo, shi);
  return env_loss_prep_fwd<DubinsPrep>(states, raw, N, p);
}

torch::Tensor dubins_loss_prep_bwd(torch::Tensor states, torch::Tensor action,
                                   torch::Tensor daction, torch::Tensor dbig, long N, double dt,
                                   double comm, double stop_r, bool enable_stop, Lim alo,
                                   Lim ahi, Lim slo, Lim shi) {
  auto p = dubins_prep_args(states, N, dt, comm, stop_r, enable_stop, alo, ahi, slo, shi);
  return env_loss_prep_bwd<DubinsPrep>(states, action, daction, dbig, N, p);
}

static DronePrep::Args drone_prep_args(const torch::Tensor& states, const torch::Tensor& Kmat,
                                       const torch::Tensor& A, const torch::Tensor& Bm, long N,
                                       double dt, double comm, const Lim& alo, const Lim& ahi,
                                       const Lim& slo, const Lim& shi) {
  auto p = env_prep_args<DronePrep>(states, N, dt, comm, alo, ahi, slo, shi);
  env_prep_check_mat(Kmat, "K", states, 3, 6);
  env_prep_check_mat(A, "A", states, 6, 6);
  env_prep_check_mat(Bm, "Bm", states, 6, 3);
  p.K = Kmat.data_ptr<float>();
  p.A = A.data_ptr<float>();
  p.Bm = Bm.data_ptr<float>();
  return p;
}

std::vector<torch::Tensor> drone_loss_prep_fwd(torch::Tensor states, torch::Tensor raw,
                                               torch::Tensor Kmat, torch::Tensor A,
                                               torch::Tensor Bm, long N, double dt, double comm,
                                               Lim alo, Lim ahi, Lim slo, Lim shi) {
  auto p = drone_prep_args(states, Kmat, A, Bm, N, dt, comm, alo, ahi, slo, shi);
  return env_loss_prep_fwd<DronePrep>(states, raw, N, p);
}

torch::Tensor drone_loss_prep_bwd(torch::Tensor states, torch::Tensor Kmat, torch::Tensor A,
                                  torch::Tensor Bm, torch::Tensor action, torch::Tensor daction,
                                  torch::Tensor dbig, long N, double dt, double comm, Lim alo,
                                  Lim ahi, Lim slo, Lim shi) {
  auto p = drone_prep_args(states, Kmat, A, Bm, N, dt, comm, alo, ahi, slo, shi);
  return env_loss_prep_bwd<DronePrep>(states, action, daction, dbig, N, p);
}

static SiPrep::Args si_prep_args(const torch::Tensor& states, const torch::Tensor& Kmat, long N,
                                 double dt, double comm, const Lim& alo, const Lim& ahi,
                                 const Lim& slo, const Lim& shi) {
  auto p = env_prep_args<SiPrep>(states, N, dt, comm, alo, ahi, slo, shi);
  env_prep_check_mat(Kmat, "K", states, 2, 2);
  p.K = Kmat.data_ptr<float>();
  return p;
}

std::vector<torch::Tensor> si_loss_prep_fwd(torch::Tensor states, torch::Tensor raw,
                                            torch::Tensor Kmat, long N, double dt, double comm,
                                            Lim alo, Lim ahi, Lim slo, Lim shi) {
  auto p = si_prep_args(states, Kmat, N, dt, comm, alo, ahi, slo, shi);
  return env_loss_prep_fwd<SiPrep>(states, raw, N, p);
}

torch::Tensor si_loss_prep_bwd(torch::Tensor states, torch::Tensor Kmat, torch::Tensor action,
                               torch::Tensor daction, torch::Tensor dbig, long N, double dt,
                               double comm, Lim alo, Lim ahi, Lim slo, Lim shi) {
  auto p = si_prep_args(states, Kmat, N, dt, comm, alo, ahi, slo, shi);
  return env_loss_prep_bwd<SiPrep>(states, action, daction, dbig, N, p);
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("dubins_loss_prep_fwd", &dubins_loss_prep_fwd,
        "fused DubinsCar loss prologue: (action unclamped, [states; next_states])",
        py::arg("states"), py::arg("raw"), py::arg("N"), py::arg("dt"), py::arg("comm"),
        py::arg("stop_r"), py::arg("enable_stop"), py::arg("act_lo"), py::arg("act_hi"),
        py::arg("st_lo"), py::arg("st_hi"));
  m.def("dubins_loss_prep_bwd", &dubins_loss_prep_bwd,
        "gradient of the DubinsCar loss prologue w.r.t. raw",
        py::arg("states"), py::arg("action"), py::arg("daction"), py::arg("dbig"),
        py::arg("N"), py::arg("dt"), py::arg("comm"), py::arg("stop_r"),
        py::arg("enable_stop"), py::arg("act_lo"), py::arg("act_hi"), py::arg("st_lo"),
        py::arg("st_hi"));
  m.def("drone_loss_prep_fwd", &drone_loss_prep_fwd,
        "fused LinearDrone loss prologue: (action unclamped, [states; next_states])",
        py::arg("states"), py::arg("raw"), py::arg("K"), py::arg("A"), py::arg("Bm"),
        py::arg("N"), py::arg("dt"), py::arg("comm"), py::arg("act_lo"), py::arg("act_hi"),
        py::arg("st_lo"), py::arg("st_hi"));
  m.def("drone_loss_prep_bwd", &drone_loss_prep_bwd,
        "gradient of the LinearDrone loss prologue w.r.t. raw",
        py::arg("states"), py::arg("K"), py::arg("A"), py::arg("Bm"), py::arg("action"),
        py::arg("daction"), py::arg("dbig"), py::arg("N"), py::arg("dt"), py::arg("comm"),
        py::arg("act_lo"), py::arg("act_hi"), py::arg("st_lo"), py::arg("st_hi"));
  m.def("si_loss_prep_fwd", &si_loss_prep_fwd,
        "fused SingleIntegrator loss prologue: (action unclamped, [states; next_states])",
        py::arg("states"), py::arg("raw"), py::arg("K"), py::arg("N"), py::arg("dt"),
        py::arg("comm"), py::arg("act_lo"), py::arg("act_hi"), py::arg("st_lo"),
        py::arg("st_hi"));
  m.def("si_loss_prep_bwd", &si_loss_prep_bwd,
        "gradient of the SingleIntegrator loss prologue w.r.t. raw",
        py::arg("states"), py::arg("K"), py::arg("action"), py::arg("daction"),
        py::arg("dbig"), py::arg("N"), py::arg("dt"), py::arg("comm"), py::arg("act_lo"),
        py::arg("act_hi"), py::arg("st_lo"), py::arg("st_hi"));
  m.def("di_loss_prep_fwd", &di_loss_prep_fwd);
  m.def("di_loss_prep_bwd", &di_loss_prep_bwd);
  m.def("crazyflie_loss_prep_fwd", &crazyflie_loss_prep_fwd,
        "fused CrazyFlie loss prologue: (action unclamped, [states; next_states])",
        py::arg("states"), py::arg("raw"), py::arg("consts"), py::arg("N"));
  m.def("crazyflie_loss_prep_bwd", &crazyflie_loss_prep_bwd,
        "gradient of the CrazyFlie loss prologue w.r.t. raw (dual-number RK4)",
        py::arg("states"), py::arg("consts"), py::arg("action"), py::arg("daction"),
        py::arg("dbig"), py::arg("N"));
  m.def("di_env_step", &di_env_step,
        "fused 2D env step, dyn=0 DI / dyn=1 Dubins (K5-K8)",
        py::arg("states"), py::arg("action"), py::arg("points"),
        py::arg("Kmat"), py::arg("N"), py::arg("R"), py::arg("dt"),
        py::arg("inv_m"), py::arg("comm"), py::arg("car_r"),
        py::arg("vmax"), py::arg("dyn") = 0);
  m.def("drone3d_step", &drone3d_step, "fused LinearDrone step part A");
  m.def("crazyflie_step", &crazyflie_step, "fused CrazyFlie step part A (RK4 + LL LQR)",
        py::arg("states"), py::arg("action"), py::arg("centers"), py::arg("radii"),
        py::arg("consts"), py::arg("N"), py::arg("R"));
  m.def("crazyflie_step_fits", &crazyflie_step_fits, py::arg("N"), py::arg("K"));
  m.def("reduce_dw_db", &reduce_dw_db, py::arg("partial"), py::arg("db_partial"),
        py::arg("dw"), py::arg("db"), py::arg("db2") = py::none(), py::arg("acc") = false);
  m.def("gemm_tn_acc2", &gemm_tn_acc2, py::arg("x"), py::arg("dz"), py::arg("yact"),
        py::arg("actin"), py::arg("dw"), py::arg("db"), py::arg("db2"),
        py::arg("rowgate") = py::none(), py::arg("m_dev") = py::none(), py::arg("row_map") = py::none());
  m.def("gcbf_loss_fwd", &gcbf_loss_fwd);
  m.def("gcbf_loss_bwd", &gcbf_loss_bwd);
  m.def("edge_msg_in_fwd", &edge_msg_in_fwd);
  m.def("edge_msg_in_bwd", &edge_msg_in_bwd);
  m.def("crazyflie_edge_jac", &crazyflie_edge_jac);
  m.def("node_msg_in_fwd", &node_msg_in_fwd,
        "layer >= 1 GNN input [X0[:E] | sender | recv | 0 pad], bf16 (B, N, D, KP1)",
        py::arg("X0"), py::arg("xa"), py::arg("c"), py::arg("E"), py::arg("R"),
        py::arg("KP1"));
  m.def("node_msg_in_bwd", &node_msg_in_bwd,
        "dX1 -> (dX0 bf16, dxa f32, dc f32), fixed summation order, no atomics",
        py::arg("dX1"), py::arg("E"), py::arg("F"), py::arg("R"), py::arg("KP0"));
  m.def("fused_adamw_step", &fused_adamw_step,
        "flat-buffer global-norm-clip AdamW with finite guard (K13)");
  m.def("proxqp_solve", &proxqp_solve_hip, "batched dense QP, one wave per problem (K11)");
  m.def("proxqp_path", &proxqp_path,
        "proxqp_kernel instantiation for (nv, k): w32x16 | w64x32 | none (torch path)");
  m.def("gemm_bias_act", &gemm_bias_act, "Y = act(X@W + b), MFMA bf16", py::arg("x"),
        py::arg("w"), py::arg("bias"), py::arg("act"), py::arg("m_dev") = py::none(),
        py::arg("out") = py::none());
  m.def("gemm_path", &gemm_path, "kernel a GEMM-family op selects for a shape (no launch)",
        py::arg("op"), py::arg("M"), py::arg("K"), py::arg("N"), py::arg("actin") = 0,
        py::arg("gated") = false);
  m.def("gemm_default_paths", &gemm_default_paths,
        "every gemm_path a default environment can select (dW slab count left out)");
  m.def("gemm_tn_map_path", &gemm_tn_map_path,
        "kernel a dW call through a row map of M entries selects (no launch)",
        py::arg("M"), py::arg("K"), py::arg("N"), py::arg("actin") = 0, py::arg("gated") = false);
  m.def("gemm_lds_limit", &gemm_lds_limit_bytes,
        "dynamic LDS bytes a workgroup may request on the current device");
  m.def("act_bwd", &act_bwd, "dZ = dY * act'(Y)");
  m.def("gemm_bt", &gemm_bt, "dX = dZ @ W^T (transposed B-stage, no copy)", py::arg("dz"),
        py::arg("w"), py::arg("yact"), py::arg("actin"), py::arg("m_dev") = py::none(),
        py::arg("out") = py::none());
  m.def("gemm_tn", &gemm_tn, "dW = X^T dZ, db = colsum dZ (deterministic)",
        py::arg("x"), py::arg("dz"), py::arg("yact"), py::arg("actin"),
        py::arg("rowgate") = py::none(), py::arg("m_dev") = py::none(), py::arg("row_map") = py::none());
  m.def("gemm_tn_acc", &gemm_tn_acc, py::arg("x"), py::arg("dz"), py::arg("yact"),
        py::arg("actin"), py::arg("dw"), py::arg("db"),
        py::arg("rowgate") = py::none(), py::arg("m_dev") = py::none(), py::arg("row_map") = py::none());
  m.def("gemm_tn_defer", &gemm_tn_defer,
        "gemm_tn_acc / gemm_tn_acc2 with the small-M launches queued for dw_flush",
        py::arg("x"), py::arg("dz"), py::arg("yact"), py::arg("actin"), py::arg("dw"),
        py::arg("db"), py::arg("db2") = py::none(), py::arg("rowgate") = py::none(),
        py::arg("m_dev") = py::none(), py::arg("row_map") = py::none());
  m.def("dw_flush", &dw_flush, "run the deferred dW queue as grouped launches");
  m.def("dw_pending", &dw_pending, "entries in the deferred dW queue");
  m.def("dw_discard", &dw_discard, "drop the deferred dW queue without running it");
  m.def("dw_launch_counts", &dw_launch_counts,
        "(grouped partial, grouped reduce) launches issued by this process so far");
  m.def("softmax_aggr_fwd", &softmax_aggr_fwd);
  m.def("softmax_aggr_bwd", &softmax_aggr_bwd);
  m.def("edge_compact", &edge_compact,
        "bool mask (..., D) -> [rows, inv, off, cnt(, gate_c)]: active slots in ascending order",
        py::arg("mask"), py::arg("align") = 128, py::arg("prefix_recv") = -1,
        py::arg("gate") = py::none());
  m.def("gather_rows", &gather_rows, "compact rows of X: X[rows[j]], zero padding rows",
        py::arg("X"), py::arg("rows"), py::arg("cnt"), py::arg("cap"));
  m.def("gather_rows_bwd", &gather_rows_bwd, "dense gradient of gather_rows",
        py::arg("dXc"), py::arg("inv"), py::arg("M"));
  m.def("add_rows_bf16", &add_rows_bf16, "a + b over the live compact rows",
        py::arg("a"), py::arg("b"), py::arg("cnt"));
  m.def("softmax_aggr_c_fwd", &softmax_aggr_c_fwd, py::arg("gate_c"), py::arg("msg_c"),
        py::arg("off"), py::arg("inv"), py::arg("D"));
  m.def("softmax_aggr_c_bwd", &softmax_aggr_c_bwd, py::arg("daggr"), py::arg("attn_c"),
        py::arg("msg_c"), py::arg("off"), py::arg("rows"), py::arg("cnt"), py::arg("D"));
  m.def("mb_gather", &mb_gather, "fused 5-tensor minibatch gather (K18)");
  m.def("raytrace_rect", &raytrace_rect);
  m.def("raytrace_sphere_topk", &raytrace_sphere_topk);
  m.def("raytrace_sphere_graph", &raytrace_sphere_graph);
}
