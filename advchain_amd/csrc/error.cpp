// Error reporting + version + the process-wide deterministic switch of the advchain C ABI.
#include <string.h>

#include <atomic>

static thread_local char g_last_error[512] = "";

extern "C" void advchain_set_error_(const char* msg) {
  strncpy(g_last_error, msg ? msg : "", sizeof(g_last_error) - 1);
  g_last_error[sizeof(g_last_error) - 1] = 0;
}

extern "C" const char* advchain_last_error(void) { return g_last_error; }

// Deterministic mode (include/advchain_hip.h): read by the scatter launchers and by advchain_scatter_workspace.
static std::atomic<int> g_deterministic{0};
extern "C" void advchain_set_deterministic(int on) { g_deterministic.store(on ? 1 : 0, std::memory_order_relaxed); }
extern "C" int advchain_get_deterministic(void) { return g_deterministic.load(std::memory_order_relaxed); }

// Which formulation the last sampler backward of this thread took (ADVCHAIN_ROUTE_* of include/advchain_hip.h): written by the
// launchers on the host, nothing on the device.
static thread_local int g_last_bwd_route = 0;
extern "C" void advchain_set_route_(int route) { g_last_bwd_route = route; }
extern "C" int advchain_last_bwd_route(void) { return g_last_bwd_route; }

extern "C" int advchain_version(void) { return 200; }  // 0.2.0: bias_rows_per_wg, bias_field_fwd_rows / bwd_rows, bias_field_bwd_reduced (rows per workgroup of the bias kernels, the adjoint's x pass inside the backward); 0.1.9: grid_sample_bwd_staged + window_stage_workspace (deterministic 2D window scatter without the int64 image), last_bwd_route; 0.1.8: grid_sample_bicubic2d_bwd_det + bicubic2d_det_workspace, tp_interp_sumsq_ordered + tp_interp_sumsq_partials, consistency_{fwd,fused_fwd,wide_fwd,lp_fwd}_ord + their _partials queries, consistency_finish_ord (deterministic mode: bicubic backward, step-count norm, loss value); 0.1.7: det_warp_workspace, grid_sample_bwd_det, affine_warp_bwd_det (deterministic general warps); 0.1.6: consistency_cw_fwd / cw_bwd / cw_ref_bwd (class weights); 0.1.5: consistency_lp_fwd / lp_bwd / lp_ref_bwd (bf16 storage); 0.1.4: consistency_ref_bwd; 0.1.3: deterministic mode; 0.1.2: kl term; slot_rows_max reset; gauss_small_pair, sign_axpy, nonzero_mask, consistency_finish
