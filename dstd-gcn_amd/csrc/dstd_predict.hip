// Autoregressive rollout of the eval forward (include/dstd_gcn_predict.h):
// K windows of dstd_model_fwd_ex chained on the device, with the frame
// shuffling between two forwards in one launch.
//
// The window kernels are csrc/dstd_window.h's (shared with dstd_rollout.hip).
#include "../../include/dstd_gcn.h"
#include "../../include/dstd_gcn_predict.h"
#include "dstd_common.h"
#include "dstd_host.h"
#include "dstd_window.h"

using namespace dstd;

extern "C" {

size_t dstd_model_predict_workspace_bytes(int B, int T, int V, int num_feature, int num_layers) {
  return rup256(dstd_model_workspace_bytes(B, T, V, num_feature, num_layers)) + 3 * window_bytes(B, T, V);
}

int dstd_model_predict(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon, float* out,
                       void* workspace, size_t workspace_bytes, void* stream, unsigned flags) {
  // (1) arguments
  StreamDeviceGuard dev_guard_(stream, obs);
  if (!p || !obs || !out || !workspace) return DSTD_EINVAL;
  const int T = p->T, V = p->V, C = p->num_feature, L_ = p->num_layers, Tin = input_n;
  if (Tin < 1 || Tin >= T || horizon < 1) return DSTD_EINVAL;
  const int Tout = T - Tin, K = (int)(((long long)horizon + Tout - 1) / Tout);
  if (!fwd_flags_ok(flags)) return DSTD_EINVAL;
  // (2) envelope
  if (K > DSTD_PREDICT_MAX_WINDOWS) return DSTD_ELIMIT;
  if (p->in_channels != 6) return DSTD_EINVAL;
  if (const int e = fwd_shape_code(B, T, V, C, L_, flags)) return e;
  if (!model_ptrs_ok(p)) return DSTD_EINVAL;
  // (3) workspace
  if (workspace_bytes < dstd_model_predict_workspace_bytes(B, T, V, C, L_)) return DSTD_EWORKSPACE;
  const size_t model_bytes = rup256(dstd_model_workspace_bytes(B, T, V, C, L_)), wb = window_bytes(B, T, V);
  char* base = (char*)workspace + model_bytes;
  float* xw[2] = {(float*)base, (float*)(base + wb)};
  float* y = (float*)(base + 2 * wb);

  hipStream_t s = (hipStream_t)stream;
  const int R = V * 3, grid = row_grid(B, T);
  k_window_obs<<<grid, DSTD_THREADS, 0, s>>>(obs, xw[0], B, T, Tin, R);
  DSTD_TRY(hipGetLastError());
  for (int k = 0; k < K; ++k) {
    const float* x = xw[k & 1];
    // windows after the first: same parameters, batch and workspace as the one before
    const unsigned fl = flags | (k > 0 ? DSTD_FWD_REUSE_CONSTANTS : 0u);
    if (const int e = dstd_model_fwd_ex(p, x, B, y, workspace, model_bytes, stream, fl, nullptr)) return e;
    k_window_roll<<<grid, DSTD_THREADS, 0, s>>>(x, y, out, k + 1 < K ? xw[(k + 1) & 1] : nullptr, B, T, Tin, R,
                                                horizon, k * Tout);
    DSTD_TRY(hipGetLastError());
  }
  return DSTD_OK;
}

}  // extern "C"
