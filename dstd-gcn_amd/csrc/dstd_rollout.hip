// Training through the rollout (include/ext/dstd_gcn_rollout.h): K windows of
// dstd_model_train_fwd_ex chained on the device, every window's input and
// saved region kept, and the chain's backward -- K dstd_model_train_bwd_ex
// with the backward of the frame shuffling between two of them.
//
// The forward is chain_fwd (dstd_chain.h), the one driver of every chain: whole
// windows (adv = Tout) here, a stride (adv < Tout) for dstd_rollout_stride.hip.
// A boundary of whole windows without a mask row is csrc/dstd_window.h's
// k_window_roll (shared with dstd_predict.hip), so a call without a teacher
// launches exactly what it did; every other boundary is k_chain_glue below.
//
// The backward glue follows the forward's: destination-driven, a wave owns one
// row (b, s) and its lanes walk the row's V * 3 floats; plain dword accesses,
// 64-bit element offsets, no LDS, no atomics, wave-uniform row arithmetic; every
// sum is a sequential fp32 chain in one lane, in the order the header fixes.
//
// Scheduled sampling (include/ext/dstd_gcn_teacher.h) is the same chain with a
// mask row per boundary: the <true> instantiations of the two backward kernels
// that see G_{k+1}, launched in place of the <false> ones only where a mask row
// applies.  The mask byte is read once per row into a scalar: the row's branch
// is wave-uniform.
#include "../../include/ext/dstd_gcn_teacher.h"
#include "dstd_common.h"
#include "dstd_host.h"
#include "dstd_window.h"
#include "dstd_chain.h"

using namespace dstd;

namespace {

// After window k (f0 = k * adv), row (b, s) of the window:
//   emit   out[b][f0 + s - Tin] = y[b][s]        for Tin <= s < Tin + adv while f0 + s - Tin < H
//   build  xn[b][s]             = seq[b][adv + min(s, Tin - 1)],  seq = x below Tin, y from Tin on
// xn == nullptr (after the last forward): the emit alone.  xn is window k + 1's
// own saved slot.  At adv = Tout this is k_window_roll's row; below it, for a
// free-running sample seq[adv + i] is h[f0 + adv + i], the frame
// dstd_predict_stride.hip's k_stride_glue takes from obs, out or y: every row
// of x below Tin is a copy of that frame, so the two build the same window.
// A sample that mrow (row k + 1 of the mask; nullptr: none) forces takes its
// rows from truth instead -- frame tb[h] + ts[h] * min(s, Tin - 1) of sample
// b mod Bt, h = b / Bt, where tb[h] is the half's truth frame of the window's
// first row (checked on the host to lie in 0 .. truth_T - 1 for every row) --
// and hands them on through x like any observed frame.
//
// No hazard: the launch reads x, y and truth and writes out and xn, which are
// five different buffers; adv + min(s, Tin - 1) <= adv + Tin - 1 <= T - 1.
__global__ __launch_bounds__(DSTD_THREADS) void k_chain_glue(const float* x, const float* y, float* out, float* xn,
                                                             const float* truth, const unsigned char* mrow, int B,
                                                             int Bt, int T, int Tin, int R, int H, int adv, int f0,
                                                             int truth_T, int tb0, int ts0, int tb1, int ts1) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const long long rows = (long long)B * T;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / T;
    const int s = (int)(r - b * T);
    const int f = f0 + s - Tin;
    if (s >= Tin && s < Tin + adv && f < H) {
      const float* src = y + r * R;
      float* dst = out + (b * H + f) * R;
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
    }
    if (xn) {
      const int ms = s < Tin ? s : Tin - 1;
      const float* src;
      if (mrow && __builtin_amdgcn_readfirstlane((int)mrow[b])) {
        const bool second = b >= Bt;
        const long long bt = second ? b - Bt : b;
        const int frame = second ? tb1 + ts1 * ms : tb0 + ts0 * ms;
        src = truth + (bt * truth_T + frame) * R;
      } else {
        const int t = adv + ms;  // adv <= t <= T - 1
        src = (t < Tin ? x : y) + (b * T + t) * R;
      }
      float* dst = xn + r * R;
      for (int d = lane; d < R; d += DSTD_WAVE) dst[d] = src[d];
    }
  }
}

// dy_k from dout and G_{k+1} (Gn; nullptr for the last window: no term).
// Row (b, s): zero below Tin; from Tin on the G_{k+1} rows s' with
// Tout + min(s', Tin - 1) == s in ascending s' -- s - Tout alone below T - 1
// (if it is a row), Tin - 1 .. T - 1 at T - 1 -- then dout's frame f0 + s - Tin
// while it is below H.  kMasked: Gn is present and mrow is row k + 1 of the
// mask: a forced sample's rows have no G term (dout's frame alone, or zero).
template <bool kMasked>
__global__ __launch_bounds__(DSTD_THREADS) void k_roll_bwd_dy(const float* dout, const float* Gn,
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
    bool term;
    if constexpr (kMasked)
      term = !__builtin_amdgcn_readfirstlane((int)mrow[b]);
    else
      term = Gn != nullptr;
    if (term) {
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
// already.  Rows: B * (Tin - Tout).  kMasked: mrow is row k + 1 of the mask: a
// forced sample's rows stay dx_k.
template <bool kMasked>
__global__ __launch_bounds__(DSTD_THREADS) void k_roll_bwd_fold(float* G, const float* Gn, const unsigned char* mrow,
                                                                int B, int T, int Tin, int R) {
  const int lane = threadIdx.x & (DSTD_WAVE - 1);
  const int Tout = T - Tin, n = Tin - Tout;
  const long long rows = (long long)B * n;
  const long long stride = (long long)gridDim.x * DSTD_WAVES;
  for (long long r = (long long)blockIdx.x * DSTD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const long long b = r / n;
    if constexpr (kMasked)
      if (__builtin_amdgcn_readfirstlane((int)mrow[b])) continue;
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

// The two launches that choose an instantiation (rollout_bwd and the test
// hooks): masked where G_{k+1} exists and its boundary has a mask row.
void launch_dy(const float* dout, const float* Gn, const unsigned char* mrow, float* dy, int B, int T, int Tin, int R,
               int H, int f0, hipStream_t s) {
  (Gn && mrow ? k_roll_bwd_dy<true> : k_roll_bwd_dy<false>)<<<row_grid(B, T), DSTD_THREADS, 0, s>>>(
      dout, Gn, mrow, dy, B, T, Tin, R, H, f0);
}

void launch_fold(float* G, const float* Gn, const unsigned char* mrow, int B, int T, int Tin, int R, hipStream_t s) {
  (mrow ? k_roll_bwd_fold<true> : k_roll_bwd_fold<false>)<<<row_grid(B, Tin - (T - Tin)), DSTD_THREADS, 0, s>>>(
      G, Gn, mrow, B, T, Tin, R);
}

// Whole windows: the chain advances Tout frames per window (0, which is
// refused, where the arguments give no such count).
inline int whole(const dstd_model_params* p, int Tin) { return p && Tin >= 1 ? p->T - Tin : 0; }

// The backward of the chain: every window from K - 1 down to 0 (only < 0), or
// window `only` alone, which finds G_{only+1} where the call for that window
// left it: G_k lives in the workspace's G buffer k & 1.
int rollout_bwd(const dstd_model_params* p, int B, int Tin, int horizon, int only, float dropout_p,
                const unsigned long long* seeds, const void* saved, size_t saved_bytes, const float* dout,
                const dstd_model_grads* g, float* dobs, void* workspace, size_t workspace_bytes, void* stream,
                unsigned flags, const TeacherArgs& ta = {}) {
  StreamDeviceGuard dev_guard_(stream, dout);
  if (!p || !saved || !dout || !g || !workspace) return DSTD_EINVAL;
  int K = 0;
  Teacher tf;
  auto probe = [&] {
    return dstd_model_train_bwd_ex(p, (const float*)saved, B, dropout_p, seed_of(seeds, 0, flags), saved, 0, dout, g,
                                   nullptr, workspace, 0, stream, flags);
  };
  if (const int e = chain_open(p, B, Tin, horizon, whole(p, Tin), only, dropout_p, seeds, ta, flags, saved_bytes,
                               probe, &K, &tf))
    return e;
  const int T = p->T, V = p->V, C = p->num_feature, L_ = p->num_layers, Tout = T - Tin;
  if (workspace_bytes < dstd_model_rollout_workspace_bytes(B, T, V, C, L_)) return DSTD_EWORKSPACE;

  const ChainSaved at(saved, p, B);
  const size_t W = at.W, M = model_ws(B, T, V, C, L_);
  char* wbase = (char*)workspace + M;
  float* dy = (float*)wbase;
  float* Gb[2] = {(float*)(wbase + W), (float*)(wbase + 2 * W)};

  hipStream_t s = (hipStream_t)stream;
  const int R = V * 3;
  const int first = only < 0 ? K - 1 : only, last = only < 0 ? 0 : only;
  for (int k = first; k >= last; --k) {
    const float* Gn = k + 1 < K ? Gb[(k + 1) & 1] : nullptr;  // G_{k+1}
    const unsigned char* mrow = Gn ? tf.row(k + 1, B) : nullptr;  // the boundary G_{k+1} crossed
    launch_dy(dout, Gn, mrow, dy, B, T, Tin, R, horizon, k * Tout, s);
    DSTD_TRY(hipGetLastError());
    float* G = (k > 0 || dobs) ? Gb[k & 1] : nullptr;  // window 0's input gradient only for dobs
    if (const int e = dstd_model_train_bwd_ex(p, at.x(k), B, dropout_p, seed_of(seeds, k, flags), at.saved(k), at.S, dy,
                                              g, G, workspace, M, stream, flags))
      return e;
    if (G && Gn && Tin > Tout) {
      launch_fold(G, Gn, mrow, B, T, Tin, R, s);
      DSTD_TRY(hipGetLastError());
    }
  }
  if (last == 0 && dobs) {
    k_roll_bwd_obs<<<row_grid(B, Tin), DSTD_THREADS, 0, s>>>(Gb[0], dobs, B, T, Tin, R);
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
    launch_dy(dout, Gn, mrow, dst, B, T, Tin, R, horizon, k * Tout, s);
  } else if (step == 1) {
    if (!Gn) return DSTD_EINVAL;
    if (Tin <= Tout) return DSTD_OK;
    launch_fold(dst, Gn, mrow, B, T, Tin, R, s);
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

// The forward of every chain, with a teacher (ta.mask != nullptr) or without.
int dstd::chain_fwd(const dstd_model_params* p, const float* obs, int B, int Tin, int horizon, int adv, float momentum,
                    float dropout_p, const unsigned long long* seeds, float* out, void* saved, size_t saved_bytes,
                    const TeacherArgs& ta, void* stream, unsigned flags) {
  StreamDeviceGuard dev_guard_(stream, obs);
  if (!p || !obs || !out || !saved) return DSTD_EINVAL;
  int K = 0;
  Teacher tf;
  auto probe = [&] {
    return dstd_model_train_fwd_ex(p, obs, B, momentum, dropout_p, seed_of(seeds, 0, flags), out, saved, 0, stream,
                                   flags);
  };
  if (const int e = chain_open(p, B, Tin, horizon, adv, -1, dropout_p, seeds, ta, flags, saved_bytes, probe, &K, &tf))
    return e;

  const ChainSaved at(saved, p, B);
  hipStream_t s = (hipStream_t)stream;
  const int T = p->T, R = p->V * 3, grid = row_grid(B, T);
  const int Bt = (flags & DSTD_TRAIN_PAIRED) ? B / 2 : B;
  k_window_obs<<<grid, DSTD_THREADS, 0, s>>>(obs, at.x(0), B, T, Tin, R);
  DSTD_TRY(hipGetLastError());
  for (int k = 0; k < K; ++k) {
    if (const int e = dstd_model_train_fwd_ex(p, at.x(k), B, momentum, dropout_p, seed_of(seeds, k, flags), at.y(),
                                              at.saved(k), at.S, stream, flags))
      return e;
    float* xn = k + 1 < K ? at.x(k + 1) : nullptr;
    const unsigned char* mrow = xn ? tf.row(k + 1, B) : nullptr;
    if (mrow || adv < T - Tin)
      k_chain_glue<<<grid, DSTD_THREADS, 0, s>>>(at.x(k), at.y(), out, xn, tf.truth, mrow, B, Bt, T, Tin, R, horizon, adv,
                                                 k * adv, tf.truth_T, tf.base(0, k + 1, adv), tf.step[0],
                                                 tf.base(1, k + 1, adv), tf.step[1]);
    else
      k_window_roll<<<grid, DSTD_THREADS, 0, s>>>(at.x(k), at.y(), out, xn, B, T, Tin, R, horizon, k * adv);
    DSTD_TRY(hipGetLastError());
  }
  return DSTD_OK;
}

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
  return chain_fwd(p, obs, B, input_n, horizon, whole(p, input_n), momentum, dropout_p, seeds, out, saved, saved_bytes,
                   {}, stream, flags);
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
  return chain_fwd(p, obs, B, input_n, horizon, whole(p, input_n), momentum, dropout_p, seeds, out, saved, saved_bytes,
                   {truth, truth_T, t0, step, mask}, stream, flags);
}

int dstd_model_rollout_tf_bwd(const dstd_model_params* p, int B, int input_n, int horizon, float dropout_p,
                              const unsigned long long* seeds, const void* saved, size_t saved_bytes,
                              const float* dout, const dstd_model_grads* g, float* dobs, void* workspace,
                              size_t workspace_bytes, const float* truth, int truth_T, const int* t0, const int* step,
                              const unsigned char* mask, void* stream, unsigned flags) {
  return rollout_bwd(p, B, input_n, horizon, -1, dropout_p, seeds, saved, saved_bytes, dout, g, dobs, workspace,
                     workspace_bytes, stream, flags, {truth, truth_T, t0, step, mask});
}

int dstd_model_rollout_tf_bwd_window(const dstd_model_params* p, int B, int input_n, int horizon, int k,
                                     float dropout_p, const unsigned long long* seeds, const void* saved,
                                     size_t saved_bytes, const float* dout, const dstd_model_grads* g, float* dobs,
                                     void* workspace, size_t workspace_bytes, const float* truth, int truth_T,
                                     const int* t0, const int* step, const unsigned char* mask, void* stream,
                                     unsigned flags) {
  if (k < 0) return DSTD_EINVAL;
  return rollout_bwd(p, B, input_n, horizon, k, dropout_p, seeds, saved, saved_bytes, dout, g, dobs, workspace,
                     workspace_bytes, stream, flags, {truth, truth_T, t0, step, mask});
}

int dstd_model_rollout_tf_glue_bwd(int step, const float* dout, const float* Gn, float* dst,
                                   const unsigned char* mask_row, int B, int T, int input_n, int V, int horizon,
                                   int k, void* stream) {
  return glue_bwd(step, dout, Gn, dst, mask_row, B, T, input_n, V, horizon, k, stream);
}

}  // extern "C"
