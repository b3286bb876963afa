// Autoregressive rollout of the eval forward (include/dstd_gcn_predict.h):
// K windows of dstd_model_fwd_ex chained on the device, with the frame
// shuffling between two forwards in one launch.
//
// Destination-driven, as dstd_data.hip: a wave owns row (b, s) of a window and
// its lanes walk the row's consecutive floats, so every load and store is a
// contiguous run.  Plain dword accesses: rows are V * 3 = 66 / 69 / 75 floats,
// only 4-byte aligned, and a B = 256 window is 2.4 MB -- the launch is
// latency-bound.  64-bit element offsets, no LDS, no atomics; the row
// arithmetic is wave-uniform.
#include "../../include/dstd_gcn.h"
#include "../../include/dstd_gcn_predict.h"
#include "dstd_common.h"
#include "dstd_host.h"

using namespace dstd;

namespace {

constexpr int kMaxBlocks = 1 << 16;  // grid cap; the rows beyond are reached by the grid-stride loop

// window 0: x0[b][s] = obs[b][min(s, Tin - 1)]
__global__ __launch_bounds__(DSTD_THREADS) void k_window_obs(const float* obs, float* x0, int B, int T, int Tin,
                                                             int R) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long rows = (long long)B * T;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / T;
    const int s = (int)(r - b * T);
    const float* src = obs + (b * Tin + (s < Tin ? s : Tin - 1)) * R;
    float* dst = x0 + r * R;
    for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
  }
}

// Between window k and k + 1, row (b, s) of the window:
//   out[b][f0 + s - Tin] = y[b][s]                       for s >= Tin while f0 + s - Tin < H   (f0 = k * Tout)
//   xn[b][s]             = seq[b][T - Tin + min(s, Tin - 1)], seq = x below Tin, y from Tin on
// xn == nullptr (after the last forward): the slice of out alone.
__global__ __launch_bounds__(DSTD_THREADS) void k_window_roll(const float* x, const float* y, float* out, float* xn,
                                                              int B, int T, int Tin, int R, int H, int f0) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long rows = (long long)B * T;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / T;
    const int s = (int)(r - b * T);
    const int f = f0 + s - Tin;
    if (s >= Tin && f < H) {
      const float* src = y + r * R;
      float* dst = out + (b * H + f) * R;
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
    }
    if (xn) {
      const int t = T - Tin + (s < Tin ? s : Tin - 1);  // Tout <= t <= T - 1
      const float* src = (t < Tin ? x : y) + (b * T + t) * R;
      float* dst = xn + r * R;
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
    }
  }
}

int row_grid(int B, int T) {
  const long long blocks = ((long long)B * T + DSTD_WAVES - 1) / DSTD_WAVES;
  return (int)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

size_t rup256(size_t n) { return (n + 255) & ~size_t(255); }
size_t window_bytes(int B, int T, int V) { return rup256((size_t)B * T * V * 3 * sizeof(float)); }

// The flags and the shape as dstd_model_fwd_ex judges them, through the
// schedule query that shares its checks (cus = 1: no device is asked).
int shape_code(int B, int T, int V, int C, int layers, unsigned flags) {
  const int n = dstd_model_fwd_schedule(B, T, V, C, layers, flags, 0, 0, 1, nullptr, 0);
  return n < 0 ? n : DSTD_OK;
}
bool flags_ok(unsigned flags) { return shape_code(1, 2, 1, 1, 0, flags) == DSTD_OK; }

// the parameter pointers dstd_model_fwd_ex checks (after the shape, before the workspace)
bool model_ptrs_ok(const dstd_model_params* p) {
  const int C = p->num_feature;
  if (!block_ptrs_ok(&p->st_in) || !block_ptrs_ok(&p->st_out) || !bn_ok(p->bn_in) || !p->prelu) return false;
  if (p->st_in.cin != 6 || p->st_in.cout != C || p->st_out.cin != C || p->st_out.cout != 3) return false;
  for (int i = 0; i < p->num_layers; ++i) {
    if (!block_ptrs_ok(&p->enc[i]) || !bn_ok(p->enc_bn[i]) || !p->enc_prelu[i]) return false;
    if (p->enc[i].cin != C || p->enc[i].cout != C) return false;
  }
  return true;
}

}  // namespace

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
  if (!flags_ok(flags)) return DSTD_EINVAL;
  // (2) envelope
  if (K > DSTD_PREDICT_MAX_WINDOWS) return DSTD_ELIMIT;
  if (p->in_channels != 6) return DSTD_EINVAL;
  if (const int e = shape_code(B, T, V, C, L_, flags)) return e;
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
