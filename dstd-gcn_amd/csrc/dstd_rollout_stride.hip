// Training through a strided rollout (include/ext/dstd_gcn_stride_train.h): K
// windows of dstd_model_train_fwd_ex chained on the device, each contributing
// its first S predicted frames, every window's input and saved region kept, and
// the chain's backward -- K dstd_model_train_bwd_ex around a gradient history
// Gh of the known sequence, with scheduled sampling at the window boundaries.
//
// The forward is dstd_rollout.hip's chain_fwd (dstd_chain.h) with adv = S; the
// backward glue kernels are this file's, written as csrc/dstd_window.h's are:
// destination-driven, a wave owns one row
// and its lanes walk the row's V * 3 floats, plain dword accesses, 64-bit
// element offsets, no LDS, no atomics, wave-uniform row arithmetic.  A sample's
// mask byte is read once per row into a scalar, so the row's branch is
// wave-uniform.  Every sum is a sequential fp32 chain in one lane, in the order
// the header fixes.
#include "../../include/ext/dstd_gcn_stride_train.h"
#include "dstd_common.h"
#include "dstd_host.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // the window kernels are chain_fwd's, not used here
#include "dstd_window.h"
#pragma clang diagnostic pop
#include "dstd_chain.h"

using namespace dstd;

namespace {

// Gh = +0.  Rows: B * (Tin + H).
__global__ __launch_bounds__(DSTD_THREADS) void k_stride_bwd_zero(float* Gh, long long rows, int R) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    float* dst = Gh + r * R;
    for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = 0.f;
  }
}

// dy_k (f0 = k * S).  Row (b, s): Gh[b][f0 + s] + dout[b][f0 + s - Tin] for
// Tin <= s < Tin + S while f0 + s - Tin < H, zero elsewhere.  L = Tin + H, the
// frames of Gh; f0 + s < L wherever Gh is read.
__global__ __launch_bounds__(DSTD_THREADS) void k_stride_bwd_dy(const float* dout, const float* Gh, float* dy, int B,
                                                                int T, int Tin, int R, int H, int S, int f0) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long rows = (long long)B * T, L = (long long)Tin + H;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / T;
    const int s = (int)(r - b * T);
    const int f = f0 + s - Tin;
    float* dst = dy + r * R;
    if (s < Tin || s >= Tin + S || f >= H) {
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = 0.f;
      continue;
    }
    const float* gsrc = Gh + (b * L + f0 + s) * R;
    const float* dsrc = dout + (b * H + f) * R;
    for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = gsrc[d] + dsrc[d];
  }
}

// dx_k into Gh (f0 = k * S).  Row (b, i), i < Tin: Gh[b][f0 + i] += dx[b][i]
// below Tin - 1; at Tin - 1 the chain Gh[b][f0 + Tin - 1] + dx[b][Tin - 1] + ...
// + dx[b][T - 1] (the padding copies of the window's last observed frame),
// ascending.  A sample that mrow (row k of the mask, k >= 1; nullptr: none)
// forces observed the truth in these Tin frames, and so does every later window
// that read them: its rows of Gh become +0.  dobs (window 0 alone, or nullptr):
// dobs[b][i] = the row's new value, by the lane that wrote it.  Rows: B * Tin;
// f0 + Tin - 1 < Tin + H because f0 < H.
__global__ __launch_bounds__(DSTD_THREADS) void k_stride_bwd_acc(const float* dx, float* Gh, float* dobs,
                                                                 const unsigned char* mrow, int B, int T, int Tin,
                                                                 int R, int H, int f0) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long rows = (long long)B * Tin, L = (long long)Tin + H;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / Tin;
    const int i = (int)(r - b * Tin);
    const float* src = dx + (b * T + i) * R;
    float* dst = Gh + (b * L + f0 + i) * R;
    if (mrow && __builtin_amdgcn_readfirstlane((int)mrow[b])) {
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = 0.f;
      continue;
    }
    float* odst = dobs ? dobs + r * R : nullptr;
    const int more = i == Tin - 1 ? T - Tin : 0;
    for (int d = lane; d < R; d += DSTD_WAVE) {
      float acc = dst[d] + src[d];
      for (int q = 1; q <= more; ++q) acc += src[(long long)q * R + d];
      dst[d] = acc;
      if (odst) odst[d] = acc;
    }
  }
}

inline size_t gh_bytes(int B, int V, int Tin, int H) {
  const long long frames = (long long)Tin + H;
  return rup256((size_t)B * (size_t)(frames > 0 ? frames : 0) * V * 3 * sizeof(float));
}

// The backward of the chain: every window from K - 1 down to 0 (only < 0), or
// window `only` alone, which finds Gh where the calls for the later windows
// left it.
int strided_bwd(const dstd_model_params* p, int B, int Tin, int horizon, int S, int only, float dropout_p,
                const unsigned long long* seeds, const void* saved, size_t saved_bytes, const float* dout,
                const dstd_model_grads* g, float* dobs, void* workspace, size_t workspace_bytes, const TeacherArgs& ta,
                void* stream, unsigned flags) {
  StreamDeviceGuard dev_guard_(stream, dout);
  if (!p || !saved || !dout || !g || !workspace) return DSTD_EINVAL;
  int K = 0;
  Teacher tf;
  auto probe = [&] {
    return dstd_model_train_bwd_ex(p, (const float*)saved, B, dropout_p, seed_of(seeds, 0, flags), saved, 0, dout, g,
                                   nullptr, workspace, 0, stream, flags);
  };
  if (const int e = chain_open(p, B, Tin, horizon, S, only, dropout_p, seeds, ta, flags, saved_bytes, probe, &K, &tf))
    return e;
  const int T = p->T, V = p->V, C = p->num_feature, L_ = p->num_layers;
  if (workspace_bytes < dstd_model_rollout_strided_workspace_bytes(B, T, V, C, L_, Tin, horizon))
    return DSTD_EWORKSPACE;

  const ChainSaved at(saved, p, B);
  const size_t W = at.W, M = model_ws(B, T, V, C, L_);
  char* wbase = (char*)workspace + M;
  float* dy = (float*)wbase;
  float* dx = (float*)(wbase + W);
  float* Gh = (float*)(wbase + 2 * W);

  hipStream_t s = (hipStream_t)stream;
  const int R = V * 3, grid = row_grid(B, T);
  const int first = only < 0 ? K - 1 : only, last = only < 0 ? 0 : only;
  if (first == K - 1) {
    const long long rows = (long long)B * (Tin + horizon);
    const long long blocks = (rows + DSTD_WAVES - 1) / DSTD_WAVES;
    k_stride_bwd_zero<<<(int)(blocks < kMaxBlocks ? blocks : kMaxBlocks), DSTD_THREADS, 0, s>>>(Gh, rows, R);
    DSTD_TRY(hipGetLastError());
  }
  for (int k = first; k >= last; --k) {
    k_stride_bwd_dy<<<grid, DSTD_THREADS, 0, s>>>(dout, Gh, dy, B, T, Tin, R, horizon, S, k * S);
    DSTD_TRY(hipGetLastError());
    const bool need_dx = k > 0 || dobs;  // window 0's input gradient only for dobs
    if (const int e = dstd_model_train_bwd_ex(p, at.x(k), B, dropout_p, seed_of(seeds, k, flags), at.saved(k), at.S, dy,
                                              g, need_dx ? dx : nullptr, workspace, M, stream, flags))
      return e;
    if (need_dx) {
      const unsigned char* mrow = k > 0 ? tf.row(k, B) : nullptr;
      k_stride_bwd_acc<<<row_grid(B, Tin), DSTD_THREADS, 0, s>>>(dx, Gh, k == 0 ? dobs : nullptr, mrow, B, T, Tin, R,
                                                                 horizon, k * S);
      DSTD_TRY(hipGetLastError());
    }
  }
  return DSTD_OK;
}

}  // namespace

extern "C" {

size_t dstd_model_rollout_strided_workspace_bytes(int B, int T, int V, int num_feature, int num_layers, int input_n,
                                                  int horizon) {
  return model_ws(B, T, V, num_feature, num_layers) + 2 * window_bytes(B, T, V) + gh_bytes(B, V, input_n, horizon);
}

int dstd_model_rollout_strided_fwd(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon,
                                   int stride, float momentum, float dropout_p, const unsigned long long* seeds,
                                   float* out, void* saved, size_t saved_bytes, const float* truth, int truth_T,
                                   const int* t0, const int* step, const unsigned char* mask, void* stream,
                                   unsigned flags) {
  return chain_fwd(p, obs, B, input_n, horizon, stride, momentum, dropout_p, seeds, out, saved, saved_bytes,
                   {truth, truth_T, t0, step, mask}, stream, flags);
}

int dstd_model_rollout_strided_bwd(const dstd_model_params* p, int B, int input_n, int horizon, int stride,
                                   float dropout_p, const unsigned long long* seeds, const void* saved,
                                   size_t saved_bytes, const float* dout, const dstd_model_grads* g, float* dobs,
                                   void* workspace, size_t workspace_bytes, const float* truth, int truth_T,
                                   const int* t0, const int* step, const unsigned char* mask, void* stream,
                                   unsigned flags) {
  return strided_bwd(p, B, input_n, horizon, stride, -1, dropout_p, seeds, saved, saved_bytes, dout, g, dobs,
                     workspace, workspace_bytes, {truth, truth_T, t0, step, mask}, stream, flags);
}

int dstd_model_rollout_strided_bwd_window(const dstd_model_params* p, int B, int input_n, int horizon, int stride,
                                          int k, float dropout_p, const unsigned long long* seeds, const void* saved,
                                          size_t saved_bytes, const float* dout, const dstd_model_grads* g,
                                          float* dobs, void* workspace, size_t workspace_bytes, const float* truth,
                                          int truth_T, const int* t0, const int* step, const unsigned char* mask,
                                          void* stream, unsigned flags) {
  if (k < 0) return DSTD_EINVAL;
  return strided_bwd(p, B, input_n, horizon, stride, k, dropout_p, seeds, saved, saved_bytes, dout, g, dobs, workspace,
                     workspace_bytes, {truth, truth_T, t0, step, mask}, stream, flags);
}

int dstd_model_rollout_strided_glue_bwd(int step, const float* dout, const float* dx, float* Gh, float* dst,
                                        const unsigned char* mask_row, int B, int T, int input_n, int V, int horizon,
                                        int stride, int k, void* stream) {
  StreamDeviceGuard dev_guard_(stream, Gh);
  const int Tin = input_n, S = stride;
  if (!Gh || B <= 0 || V <= 0 || Tin < 1 || Tin >= T || horizon < 1 || S < 1 || S > T - Tin || k < 0)
    return DSTD_EINVAL;
  if (k >= ((long long)horizon + S - 1) / S) return DSTD_EINVAL;
  if ((long long)B * T > INT32_MAX || (long long)V * 3 > INT32_MAX) return DSTD_ELIMIT;
  hipStream_t s = (hipStream_t)stream;
  const int R = V * 3;
  if (step == 0) {
    if (!dout || !dst) return DSTD_EINVAL;
    k_stride_bwd_dy<<<row_grid(B, T), DSTD_THREADS, 0, s>>>(dout, Gh, dst, B, T, Tin, R, horizon, S, k * S);
  } else if (step == 1) {
    if (!dx) return DSTD_EINVAL;
    k_stride_bwd_acc<<<row_grid(B, Tin), DSTD_THREADS, 0, s>>>(dx, Gh, k == 0 ? dst : nullptr,
                                                               k > 0 ? mask_row : nullptr, B, T, Tin, R, horizon, k * S);
  } else {
    return DSTD_EINVAL;
  }
  DSTD_TRY(hipGetLastError());
  return DSTD_OK;
}

}  // extern "C"
