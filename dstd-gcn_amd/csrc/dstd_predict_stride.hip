// Predict with a stride (include/ext/dstd_gcn_stride.h): K windows of
// dstd_model_fwd_ex chained on the device, each contributing its first S
// predicted frames, with the frame shuffling between two forwards in one launch.
//
// Window 0 is csrc/dstd_window.h's k_window_obs; the glue kernel is this file's,
// written as that header's are: destination-driven, a wave owns row (b, s) and
// its lanes walk the row's V * 3 floats, plain dword accesses, 64-bit element
// offsets, no LDS, no atomics, the source choice wave-uniform.
#include "../../include/dstd_gcn.h"
#include "../../include/ext/dstd_gcn_stride.h"
#include "dstd_common.h"
#include "dstd_host.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // k_window_roll, the unstrided chain's glue, is not used here
#include "dstd_window.h"
#pragma clang diagnostic pop

using namespace dstd;

namespace {

// After window k (f0 = k * S), row (b, s) of the window:
//   emit   out[b][f0 + s - Tin] = y[b][s]        for Tin <= s < Tin + S while f0 + s - Tin < H
//   build  xn[b][s]             = h[b][i],  i = f0 + S + min(s, Tin - 1),  h = obs then out:
//            i < Tin             obs[b][i]
//            i - Tin >= f0       y[b][Tin + (i - Tin - f0)]   a frame this launch emits
//            otherwise           out[b][i - Tin]              written by an earlier launch
// xn == nullptr (after the last forward): the emit alone.
//
// The one hazard: a row must never read a row of out that this launch writes.
// The launch writes out[b][f] for f >= f0 only, and a build row reads out[b][g]
// only where g = i - Tin < f0 -- frames at or above f0 are taken from y
// instead, where i - Tin - f0 = S + min(s, Tin - 1) - Tin <= S - 1 < Tout.
// Frames below f0 were written by the launches after windows 0..k-1, earlier on
// the same stream.  A build row exists only where (k + 1) * S < H, so g < H.
__global__ __launch_bounds__(DSTD_THREADS) void k_stride_glue(const float* obs, const float* y, float* out, float* xn,
                                                              int B, int T, int Tin, int R, int H, int S, int f0) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long rows = (long long)B * T;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / T;
    const int s = (int)(r - b * T);
    const int f = f0 + s - Tin;
    if (s >= Tin && s < Tin + S && f < H) {
      const float* src = y + r * R;
      float* dst = out + (b * H + f) * R;
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
    }
    if (xn) {
      const int i = f0 + S + (s < Tin ? s : Tin - 1);
      const int g = i - Tin;
      const float* src = i < Tin   ? obs + (b * Tin + i) * R
                         : g >= f0 ? y + (b * T + Tin + (g - f0)) * R
                                   : out + (b * H + g) * R;
      float* dst = xn + r * R;
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
    }
  }
}

}  // namespace

extern "C" {

size_t dstd_model_predict_strided_workspace_bytes(int B, int T, int V, int num_feature, int num_layers) {
  return rup256(dstd_model_workspace_bytes(B, T, V, num_feature, num_layers)) + 2 * window_bytes(B, T, V);
}

int dstd_model_predict_strided(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon,
                               int stride, float* out, void* workspace, size_t workspace_bytes, void* stream,
                               unsigned flags) {
  // (1) arguments
  StreamDeviceGuard dev_guard_(stream, obs);
  if (!p || !obs || !out || !workspace) return DSTD_EINVAL;
  const int T = p->T, V = p->V, C = p->num_feature, L_ = p->num_layers, Tin = input_n, S = stride;
  if (Tin < 1 || Tin >= T || horizon < 1 || S < 1 || S > T - Tin) return DSTD_EINVAL;
  const long long K = ((long long)horizon + S - 1) / S;
  if (!fwd_flags_ok(flags)) return DSTD_EINVAL;
  // (2) envelope
  if (K > DSTD_PREDICT_MAX_WINDOWS) return DSTD_ELIMIT;
  if (p->in_channels != 6) return DSTD_EINVAL;
  if (const int e = fwd_shape_code(B, T, V, C, L_, flags)) return e;
  if (!model_ptrs_ok(p)) return DSTD_EINVAL;
  // (3) workspace
  if (workspace_bytes < dstd_model_predict_strided_workspace_bytes(B, T, V, C, L_)) return DSTD_EWORKSPACE;
  const size_t model_bytes = rup256(dstd_model_workspace_bytes(B, T, V, C, L_)), wb = window_bytes(B, T, V);
  char* base = (char*)workspace + model_bytes;
  float* x = (float*)base;
  float* y = (float*)(base + wb);

  hipStream_t s = (hipStream_t)stream;
  const int R = V * 3, grid = row_grid(B, T);
  k_window_obs<<<grid, DSTD_THREADS, 0, s>>>(obs, x, B, T, Tin, R);
  DSTD_TRY(hipGetLastError());
  for (int k = 0; k < (int)K; ++k) {
    // windows after the first: same parameters, batch and workspace as the one before
    const unsigned fl = flags | (k > 0 ? DSTD_FWD_REUSE_CONSTANTS : 0u);
    if (const int e = dstd_model_fwd_ex(p, x, B, y, workspace, model_bytes, stream, fl, nullptr)) return e;
    // x_{k+1} reads obs, out and y_k, nothing of x_k: built in place
    k_stride_glue<<<grid, DSTD_THREADS, 0, s>>>(obs, y, out, k + 1 < K ? x : nullptr, B, T, Tin, R, horizon, S, k * S);
    DSTD_TRY(hipGetLastError());
  }
  return DSTD_OK;
}

}  // extern "C"
