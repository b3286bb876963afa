// Training through the rollout (include/ext/dstd_gcn_rollout.h): K windows of
// dstd_model_train_fwd_ex chained on the device, every window's input and
// saved region kept, and the chain's backward -- K dstd_model_train_bwd_ex
// with the backward of the frame shuffling between two of them.
//
// The forward glue is csrc/dstd_window.h's (shared with dstd_predict.hip).  The
// backward glue follows it: destination-driven, a wave owns one row (b, s) and
// its lanes walk the row's V * 3 floats; plain dword accesses, 64-bit element
// offsets, no LDS, no atomics, wave-uniform row arithmetic; every sum is a
// sequential fp32 chain in one lane, in the order the header fixes.
//
// Scheduled sampling (include/ext/dstd_gcn_teacher.h) is the same chain with a
// mask row per boundary: kernels of their own below (k_roll_tf and the _tf
// forms of the two backward kernels that see G_{k+1}), launched in place of the
// free-running ones only where a mask row applies, so a call without a teacher
// launches exactly what it did.  The mask byte is read once per row into a
// scalar: the row's branch is wave-uniform.
#include "../../include/ext/dstd_gcn_teacher.h"
#include "dstd_common.h"
#include "dstd_host.h"
#include "dstd_window.h"
#include "dstd_chain.h"

using namespace dstd;

namespace {

// dy_k from dout and G_{k+1} (Gn; nullptr for the last window: no term).
// Row (b, s): zero below Tin; from Tin on the G_{k+1} rows s' with
// Tout + min(s', Tin - 1) == s in ascending s' -- s - Tout alone below T - 1
// (if it is a row), Tin - 1 .. T - 1 at T - 1 -- then dout's frame f0 + s - Tin
// while it is below H.
__global__ __launch_bounds__(DSTD_THREADS) void k_roll_bwd_dy(const float* dout, const float* Gn, float* dy, int B,
                                                              int T, int Tin, int R, int H, int f0) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const int Tout = T - Tin;
  const long long rows = (long long)B * T;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / T;
    const int s = (int)(r - b * T);
    float* dst = dy + r * R;
    if (s < Tin) {
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = 0.f;
      continue;
    }
    int lo = 0, hi = -1;  // the rows lo .. hi of Gn
    if (Gn) {
      if (s == T - 1) {
        lo = Tin - 1;
        hi = T - 1;
      } else if (s >= Tout) {
        lo = hi = s - Tout;
      }
    }
    const int f = f0 + s - Tin;
    const float* dsrc = f < H ? dout + (b * H + f) * R : nullptr;
    const float* gsrc = lo <= hi ? Gn + (b * T + lo) * R : nullptr;
    for (int d = lane; d < R; d += DSTD_WAVE) {
      float acc = 0.f;
      if (lo <= hi) {
        acc = gsrc[d];
        for (int q = 1; q <= hi - lo; ++q) acc += gsrc[(long long)q * R + d];
        if (dsrc) acc += dsrc[d];
      } else if (dsrc) {
        acc = dsrc[d];
      }
      dst[d] = acc;
    }
  }
}

// G_k in place of dx_k: G[b][t] = Gn[b][t - Tout] + G[b][t] for Tout <= t < Tin
// (the observed frames window k + 1 took from x_k); the other rows are dx_k
// already.  Rows: B * (Tin - Tout).
__global__ __launch_bounds__(DSTD_THREADS) void k_roll_bwd_fold(float* G, const float* Gn, int B, int T, int Tin,
                                                                int R) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const int Tout = T - Tin, n = Tin - Tout;
  const long long rows = (long long)B * n;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / n;
    const int t = Tout + (int)(r - b * n);
    float* dst = G + (b * T + t) * R;
    const float* src = Gn + (b * T + t - Tout) * R;
    for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d] + dst[d];
  }
}

// dobs[b][i] = G0[b][i] below Tin - 1; dobs[b][Tin - 1] = G0[b][Tin - 1] + ... + G0[b][T - 1]
// (the padding copies of the last observed frame), ascending.  Rows: B * Tin.
__global__ __launch_bounds__(DSTD_THREADS) void k_roll_bwd_obs(const float* G0, float* dobs, int B, int T, int Tin,
                                                               int R) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long rows = (long long)B * Tin;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / Tin;
    const int i = (int)(r - b * Tin);
    const float* src = G0 + (b * T + i) * R;
    float* dst = dobs + r * R;
    const int more = i == Tin - 1 ? T - Tin : 0;
    for (int d = lane; d < R; d += DSTD_WAVE) {
      float acc = src[d];
      for (int q = 1; q <= more; ++q) acc += src[(long long)q * R + d];
      dst[d] = acc;
    }
  }
}

// k_window_roll between window k and k + 1 (xn is never null here) with the
// source of xn chosen per sample: mrow[b] == 0 as there; otherwise truth row
// tb[h] + ts[h] * min(s, Tin - 1) of sample b mod Bt, h = b / Bt, where tb[h] is
// the half's truth frame of the window's first row (checked on the host to lie
// in 0 .. truth_T - 1 for every row).  The slice of out is y's either way.
__global__ __launch_bounds__(DSTD_THREADS) void k_roll_tf(const float* x, const float* y, float* out, float* xn,
                                                          const float* truth, const unsigned char* mrow, int B, int Bt,
                                                          int T, int Tin, int R, int H, int f0, int truth_T, int tb0,
                                                          int ts0, int tb1, int ts1) {
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
    const int ms = s < Tin ? s : Tin - 1;
    const float* src;
    if (__builtin_amdgcn_readfirstlane((int)mrow[b])) {
      const bool second = b >= Bt;
      const long long bt = second ? b - Bt : b;
      const int frame = second ? tb1 + ts1 * ms : tb0 + ts0 * ms;
      src = truth + (bt * truth_T + frame) * R;
    } else {
      const int t = T - Tin + ms;  // Tout <= t <= T - 1
      src = (t < Tin ? x : y) + (b * T + t) * R;
    }
    float* dst = xn + r * R;
    for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
  }
}

// k_roll_bwd_dy with Gn = G_{k+1} present and row k + 1 of the mask: a forced
// sample's rows have no G term (dout's frame alone, or zero).
__global__ __launch_bounds__(DSTD_THREADS) void k_roll_bwd_dy_tf(const float* dout, const float* Gn,
                                                                 const unsigned char* mrow, float* dy, int B, int T,
                                                                 int Tin, int R, int H, int f0) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const int Tout = T - Tin;
  const long long rows = (long long)B * T;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / T;
    const int s = (int)(r - b * T);
    float* dst = dy + r * R;
    if (s < Tin) {
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = 0.f;
      continue;
    }
    int lo = 0, hi = -1;  // the rows lo .. hi of Gn
    if (!__builtin_amdgcn_readfirstlane((int)mrow[b])) {
      if (s == T - 1) {
        lo = Tin - 1;
        hi = T - 1;
      } else if (s >= Tout) {
        lo = hi = s - Tout;
      }
    }
    const int f = f0 + s - Tin;
    const float* dsrc = f < H ? dout + (b * H + f) * R : nullptr;
    const float* gsrc = lo <= hi ? Gn + (b * T + lo) * R : nullptr;
    for (int d = lane; d < R; d += DSTD_WAVE) {
      float acc = 0.f;
      if (lo <= hi) {
        acc = gsrc[d];
        for (int q = 1; q <= hi - lo; ++q) acc += gsrc[(long long)q * R + d];
        if (dsrc) acc += dsrc[d];
      } else if (dsrc) {
        acc = dsrc[d];
      }
      dst[d] = acc;
    }
  }
}

// k_roll_bwd_fold with row k + 1 of the mask: a forced sample's rows stay dx_k.
__global__ __launch_bounds__(DSTD_THREADS) void k_roll_bwd_fold_tf(float* G, const float* Gn, const unsigned char* mrow,
                                                                   int B, int T, int Tin, int R) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const int Tout = T - Tin, n = Tin - Tout;
  const long long rows = (long long)B * n;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / n;
    if (__builtin_amdgcn_readfirstlane((int)mrow[b])) continue;
    const int t = Tout + (int)(r - b * n);
    float* dst = G + (b * T + t) * R;
    const float* src = Gn + (b * T + t - Tout) * R;
    for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d] + dst[d];
  }
}

// The backward of the chain: every window from K - 1 down to 0 (only < 0), or
// window `only` alone, which finds G_{only+1} where the call for that window
// left it: G_k lives in the workspace's G buffer k & 1.
int rollout_bwd(const dstd_model_params* p, int B, int input_n, int horizon, int only, float dropout_p,
                const unsigned long long* seeds, const void* saved, size_t saved_bytes, const float* dout,
                const dstd_model_grads* g, float* dobs, void* workspace, size_t workspace_bytes, void* stream,
                unsigned flags, const float* truth = nullptr, int truth_T = 0, const int* t0 = nullptr,
                const int* step = nullptr, const unsigned char* mask = nullptr) {
  StreamDeviceGuard dev_guard_(stream, dout);
  if (!p || !saved || !dout || !g || !workspace) return DSTD_EINVAL;
  const int T = p->T, V = p->V, C = p->num_feature, L_ = p->num_layers, Tin = input_n;
  if (Tin < 1 || Tin >= T || horizon < 1) return DSTD_EINVAL;
  if (dropout_p > 0.f && !seeds) return DSTD_EINVAL;
  const int Tout = T - Tin;
  const long long Kll = ((long long)horizon + Tout - 1) / Tout;
  if (only >= Kll) return DSTD_EINVAL;
  Teacher tf;
  if (const int e = teacher_check(truth, truth_T, t0, step, mask, flags, Tin, Tout, Kll, &tf)) return e;
  const int probe = dstd_model_train_bwd_ex(p, (const float*)saved, B, dropout_p, seed_of(seeds, 0, flags), saved, 0,
                                            dout, g, nullptr, workspace, 0, stream, flags);
  if (const int e = chain_code(probe, Kll)) return e;
  const int K = (int)Kll;
  if (saved_bytes < dstd_model_rollout_saved_bytes(B, T, V, C, L_, K)) return DSTD_EWORKSPACE;
  if (workspace_bytes < dstd_model_rollout_workspace_bytes(B, T, V, C, L_)) return DSTD_EWORKSPACE;

  const size_t W = window_bytes(B, T, V), S = model_saved(B, T, V, C, L_), M = model_ws(B, T, V, C, L_);
  const char* base = (const char*)saved;
  auto xk = [&](int k) { return (const float*)(base + W + (size_t)k * (W + S)); };
  auto sk = [&](int k) { return (const void*)(base + W + (size_t)k * (W + S) + W); };
  char* wbase = (char*)workspace + M;
  float* dy = (float*)wbase;
  float* Gb[2] = {(float*)(wbase + W), (float*)(wbase + 2 * W)};

  hipStream_t s = (hipStream_t)stream;
  const int R = V * 3, grid = row_grid(B, T);
  const int first = only < 0 ? K - 1 : only, last = only < 0 ? 0 : only;
  for (int k = first; k >= last; --k) {
    const float* Gn = k + 1 < K ? Gb[(k + 1) & 1] : nullptr;  // G_{k+1}
    const unsigned char* mrow = Gn && tf.mask ? tf.mask + (size_t)(k + 1) * B : nullptr;  // the boundary G_{k+1} crossed
    if (mrow)
      k_roll_bwd_dy_tf<<<grid, DSTD_THREADS, 0, s>>>(dout, Gn, mrow, dy, B, T, Tin, R, horizon, k * Tout);
    else
      k_roll_bwd_dy<<<grid, DSTD_THREADS, 0, s>>>(dout, Gn, dy, B, T, Tin, R, horizon, k * Tout);
    DSTD_TRY(hipGetLastError());
    float* G = (k > 0 || dobs) ? Gb[k & 1] : nullptr;  // window 0's input gradient only for dobs
    if (const int e = dstd_model_train_bwd_ex(p, xk(k), B, dropout_p, seed_of(seeds, k, flags), sk(k), S, dy, g, G,
                                              workspace, M, stream, flags))
      return e;
    if (G && Gn && Tin > Tout) {
      if (mrow)
        k_roll_bwd_fold_tf<<<row_grid(B, Tin - Tout), DSTD_THREADS, 0, s>>>(G, Gn, mrow, B, T, Tin, R);
      else
        k_roll_bwd_fold<<<row_grid(B, Tin - Tout), DSTD_THREADS, 0, s>>>(G, Gn, B, T, Tin, R);
      DSTD_TRY(hipGetLastError());
    }
  }
  if (last == 0 && dobs) {
    k_roll_bwd_obs<<<row_grid(B, Tin), DSTD_THREADS, 0, s>>>(Gb[0], dobs, B, T, Tin, R);
    DSTD_TRY(hipGetLastError());
  }
  return DSTD_OK;
}

// The forward of the chain, with a teacher (mask != nullptr) or without.
int rollout_fwd(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon, float momentum,
                float dropout_p, const unsigned long long* seeds, float* out, void* saved, size_t saved_bytes,
                void* stream, unsigned flags, const float* truth = nullptr, int truth_T = 0,
                const int* t0 = nullptr, const int* step = nullptr, const unsigned char* mask = nullptr) {
  StreamDeviceGuard dev_guard_(stream, obs);
  if (!p || !obs || !out || !saved) return DSTD_EINVAL;
  const int T = p->T, V = p->V, C = p->num_feature, L_ = p->num_layers, Tin = input_n;
  if (Tin < 1 || Tin >= T || horizon < 1) return DSTD_EINVAL;
  if (dropout_p > 0.f && !seeds) return DSTD_EINVAL;
  const int Tout = T - Tin;
  const long long Kll = ((long long)horizon + Tout - 1) / Tout;
  Teacher tf;
  if (const int e = teacher_check(truth, truth_T, t0, step, mask, flags, Tin, Tout, Kll, &tf)) return e;
  const int probe = dstd_model_train_fwd_ex(p, obs, B, momentum, dropout_p, seed_of(seeds, 0, flags), out, saved, 0,
                                            stream, flags);
  if (const int e = chain_code(probe, Kll)) return e;
  const int K = (int)Kll;
  if (saved_bytes < dstd_model_rollout_saved_bytes(B, T, V, C, L_, K)) return DSTD_EWORKSPACE;

  const size_t W = window_bytes(B, T, V), S = model_saved(B, T, V, C, L_);
  char* base = (char*)saved;
  float* y = (float*)base;
  auto xk = [&](int k) { return (float*)(base + W + (size_t)k * (W + S)); };
  auto sk = [&](int k) { return (void*)(base + W + (size_t)k * (W + S) + W); };

  hipStream_t s = (hipStream_t)stream;
  const int R = V * 3, grid = row_grid(B, T);
  const int Bt = (flags & DSTD_TRAIN_PAIRED) ? B / 2 : B;
  k_window_obs<<<grid, DSTD_THREADS, 0, s>>>(obs, xk(0), B, T, Tin, R);
  DSTD_TRY(hipGetLastError());
  for (int k = 0; k < K; ++k) {
    if (const int e = dstd_model_train_fwd_ex(p, xk(k), B, momentum, dropout_p, seed_of(seeds, k, flags), y, sk(k), S,
                                              stream, flags))
      return e;
    if (tf.mask && k + 1 < K)
      k_roll_tf<<<grid, DSTD_THREADS, 0, s>>>(xk(k), y, out, xk(k + 1), tf.truth, tf.mask + (size_t)(k + 1) * B, B, Bt, T,
                                              Tin, R, horizon, k * Tout, tf.truth_T, tf.base(0, k + 1, Tout), tf.step[0],
                                              tf.base(1, k + 1, Tout), tf.step[1]);
    else
      k_window_roll<<<grid, DSTD_THREADS, 0, s>>>(xk(k), y, out, k + 1 < K ? xk(k + 1) : nullptr, B, T, Tin, R, horizon,
                                                  k * Tout);
    DSTD_TRY(hipGetLastError());
  }
  return DSTD_OK;
}

// One launch of the backward's glue (the test hooks); mrow: row k + 1 of a
// teacher's mask for steps 0 and 1, or nullptr.
int glue_bwd(int step, const float* dout, const float* Gn, float* dst, const unsigned char* mrow, int B, int T,
             int input_n, int V, int horizon, int k, void* stream) {
  StreamDeviceGuard dev_guard_(stream, dst);
  const int Tin = input_n;
  if (!dst || B <= 0 || V <= 0 || Tin < 1 || Tin >= T || horizon < 1 || k < 0) return DSTD_EINVAL;
  const int Tout = T - Tin;
  if (k >= ((long long)horizon + Tout - 1) / Tout) return DSTD_EINVAL;
  if ((long long)B * T > INT32_MAX || (long long)V * 3 > INT32_MAX) return DSTD_ELIMIT;
  hipStream_t s = (hipStream_t)stream;
  const int R = V * 3;
  if (step == 0) {
    if (!dout) return DSTD_EINVAL;
    if (Gn && mrow)
      k_roll_bwd_dy_tf<<<row_grid(B, T), DSTD_THREADS, 0, s>>>(dout, Gn, mrow, dst, B, T, Tin, R, horizon, k * Tout);
    else
      k_roll_bwd_dy<<<row_grid(B, T), DSTD_THREADS, 0, s>>>(dout, Gn, dst, B, T, Tin, R, horizon, k * Tout);
  } else if (step == 1) {
    if (!Gn) return DSTD_EINVAL;
    if (Tin <= Tout) return DSTD_OK;
    if (mrow)
      k_roll_bwd_fold_tf<<<row_grid(B, Tin - Tout), DSTD_THREADS, 0, s>>>(dst, Gn, mrow, B, T, Tin, R);
    else
      k_roll_bwd_fold<<<row_grid(B, Tin - Tout), DSTD_THREADS, 0, s>>>(dst, Gn, B, T, Tin, R);
  } else if (step == 2) {
    if (!Gn) return DSTD_EINVAL;
    k_roll_bwd_obs<<<row_grid(B, Tin), DSTD_THREADS, 0, s>>>(Gn, dst, B, T, Tin, R);
  } else {
    return DSTD_EINVAL;
  }
  DSTD_TRY(hipGetLastError());
  return DSTD_OK;
}

}  // namespace

extern "C" {

size_t dstd_model_rollout_saved_bytes(int B, int T, int V, int num_feature, int num_layers, int windows) {
  const size_t W = window_bytes(B, T, V);
  return W + (size_t)(windows > 0 ? windows : 0) * (W + model_saved(B, T, V, num_feature, num_layers));
}

size_t dstd_model_rollout_workspace_bytes(int B, int T, int V, int num_feature, int num_layers) {
  return model_ws(B, T, V, num_feature, num_layers) + 3 * window_bytes(B, T, V);
}

int dstd_model_rollout_fwd(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon,
                           float momentum, float dropout_p, const unsigned long long* seeds, float* out,
                           void* saved, size_t saved_bytes, void* stream, unsigned flags) {
  return rollout_fwd(p, obs, B, input_n, horizon, momentum, dropout_p, seeds, out, saved, saved_bytes, stream, flags);
}

int dstd_model_rollout_bwd(const dstd_model_params* p, int B, int input_n, int horizon, float dropout_p,
                           const unsigned long long* seeds, const void* saved, size_t saved_bytes, const float* dout,
                           const dstd_model_grads* g, float* dobs, void* workspace, size_t workspace_bytes,
                           void* stream, unsigned flags) {
  return rollout_bwd(p, B, input_n, horizon, -1, dropout_p, seeds, saved, saved_bytes, dout, g, dobs, workspace,
                     workspace_bytes, stream, flags);
}

int dstd_model_rollout_bwd_window(const dstd_model_params* p, int B, int input_n, int horizon, int k, float dropout_p,
                                  const unsigned long long* seeds, const void* saved, size_t saved_bytes,
                                  const float* dout, const dstd_model_grads* g, float* dobs, void* workspace,
                                  size_t workspace_bytes, void* stream, unsigned flags) {
  if (k < 0) return DSTD_EINVAL;
  return rollout_bwd(p, B, input_n, horizon, k, dropout_p, seeds, saved, saved_bytes, dout, g, dobs, workspace,
                     workspace_bytes, stream, flags);
}

int dstd_model_rollout_glue_bwd(int step, const float* dout, const float* Gn, float* dst, int B, int T, int input_n,
                                int V, int horizon, int k, void* stream) {
  return glue_bwd(step, dout, Gn, dst, nullptr, B, T, input_n, V, horizon, k, stream);
}

// ---- include/ext/dstd_gcn_teacher.h ----------------------------------------------

int dstd_model_rollout_tf_fwd(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon,
                              float momentum, float dropout_p, const unsigned long long* seeds, float* out,
                              void* saved, size_t saved_bytes, const float* truth, int truth_T, const int* t0,
                              const int* step, const unsigned char* mask, void* stream, unsigned flags) {
  return rollout_fwd(p, obs, B, input_n, horizon, momentum, dropout_p, seeds, out, saved, saved_bytes, stream, flags,
                     truth, truth_T, t0, step, mask);
}

int dstd_model_rollout_tf_bwd(const dstd_model_params* p, int B, int input_n, int horizon, float dropout_p,
                              const unsigned long long* seeds, const void* saved, size_t saved_bytes,
                              const float* dout, const dstd_model_grads* g, float* dobs, void* workspace,
                              size_t workspace_bytes, const float* truth, int truth_T, const int* t0, const int* step,
                              const unsigned char* mask, void* stream, unsigned flags) {
  return rollout_bwd(p, B, input_n, horizon, -1, dropout_p, seeds, saved, saved_bytes, dout, g, dobs, workspace,
                     workspace_bytes, stream, flags, truth, truth_T, t0, step, mask);
}

int dstd_model_rollout_tf_bwd_window(const dstd_model_params* p, int B, int input_n, int horizon, int k,
                                     float dropout_p, const unsigned long long* seeds, const void* saved,
                                     size_t saved_bytes, const float* dout, const dstd_model_grads* g, float* dobs,
                                     void* workspace, size_t workspace_bytes, const float* truth, int truth_T,
                                     const int* t0, const int* step, const unsigned char* mask, void* stream,
                                     unsigned flags) {
  if (k < 0) return DSTD_EINVAL;
  return rollout_bwd(p, B, input_n, horizon, k, dropout_p, seeds, saved, saved_bytes, dout, g, dobs, workspace,
                     workspace_bytes, stream, flags, truth, truth_T, t0, step, mask);
}

int dstd_model_rollout_tf_glue_bwd(int step, const float* dout, const float* Gn, float* dst,
                                   const unsigned char* mask_row, int B, int T, int input_n, int V, int horizon,
                                   int k, void* stream) {
  return glue_bwd(step, dout, Gn, dst, mask_row, B, T, input_n, V, horizon, k, stream);
}

}  // extern "C"
