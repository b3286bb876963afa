// Host-side helpers shared by the C entry points (dstd_capi.hip,
// dstd_train_capi.hip, dstd_ctg.hip): the workspace carver, the error-return
// macros, the shape envelope and the pointer validators of the parameter
// structures.  Host code only -- nothing here reaches a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/dstd_gcn.h"
#include "../../include/dstd_gcn_train.h"

namespace dstd {

// Bump allocator over a caller's buffer.  With base == nullptr it only
// measures, so a size export and the call that carves share one layout.
struct Carver {
  char* base;
  size_t off = 0;
  float* take(size_t nfloats) {
    off = (off + 255) & ~size_t(255);
    float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += nfloats * sizeof(float);
    return p;
  }
};

// Return a failed HIP call's error from a C entry point (int) / a launcher (hipError_t).
#define DSTD_TRY(expr)                    \
  do {                                    \
    hipError_t _e = (expr);               \
    if (_e != hipSuccess) return (int)_e; \
  } while (0)

#define DSTD_TRYH(expr)              \
  do {                               \
    hipError_t _e = (expr);          \
    if (_e != hipSuccess) return _e; \
  } while (0)

// The envelope every entry point refuses beyond (DSTD_ELIMIT).
constexpr int kMaxT = 128;  // the generic kernels cover T <= 128 (adjacency row groups past 112)
constexpr int kMaxV = 32;
constexpr int kMaxC = 64;
constexpr int kMaxRed = 8;  // red_channels of one DSTDGC (P / Q channels each)

inline bool gc_ok(const dstd_gc_weights* w) {
  return w && w->wf && w->bf && w->wm1 && w->bm1 && w->wm2 && w->bm2 && w->wrm && w->brm;
}
inline bool gg_ok(const dstd_gc_grads* g) {
  return g && g->wf && g->bf && g->wm1 && g->bm1 && g->wm2 && g->bm2 && g->wrm && g->brm;
}
inline bool bn_ok(const dstd_bn& b) { return b.weight && b.bias && b.running_mean && b.running_var; }
inline bool bng_ok(const dstd_bn_grads& b) { return b.weight && b.bias; }
// The pointers of one block; the residual members only where cin != cout.
// The channel counts themselves are judged by the callers: the eval forward
// through its envelope (DSTD_ELIMIT), the training path as an argument error
// (DSTD_EINVAL, dstd_train_capi.hip block_channels_ok).
inline bool block_ptrs_ok(const dstd_block_params* p) {
  if (!p || !p->A_s || !p->W_s || !p->R_s || !p->A_t || !p->R_t || !p->alpha_sm || !p->alpha_tm || !p->prelu)
    return false;
  if (!gc_ok(&p->conv_s[0]) || !gc_ok(&p->conv_s[1]) || !gc_ok(&p->conv_t) || !bn_ok(p->bn)) return false;
  if (p->cin != p->cout && (!p->res_w || !p->res_b || !bn_ok(p->res_bn))) return false;
  return true;
}

// What the chains over dstd_model_fwd_ex (dstd_predict.hip,
// dstd_predict_stride.hip) check before their first launch, as the forward
// itself judges it.  The flags and the shape go through the schedule query
// that shares the forward's checks (cus = 1: no device is asked).
inline int fwd_shape_code(int B, int T, int V, int C, int layers, unsigned flags) {
  const int n = dstd_model_fwd_schedule(B, T, V, C, layers, flags, 0, 0, 1, nullptr, 0);
  return n < 0 ? n : DSTD_OK;
}
inline bool fwd_flags_ok(unsigned flags) { return fwd_shape_code(1, 2, 1, 1, 0, flags) == DSTD_OK; }

// the parameter pointers dstd_model_fwd_ex checks (after the shape, before the workspace)
inline bool model_ptrs_ok(const dstd_model_params* p) {
  const int C = p->num_feature;
  if (!block_ptrs_ok(&p->st_in) || !block_ptrs_ok(&p->st_out) || !bn_ok(p->bn_in) || !p->prelu) return false;
  if (p->st_in.cin != 6 || p->st_in.cout != C || p->st_out.cin != C || p->st_out.cout != 3) return false;
  for (int i = 0; i < p->num_layers; ++i) {
    if (!block_ptrs_ok(&p->enc[i]) || !bn_ok(p->enc_bn[i]) || !p->enc_prelu[i]) return false;
    if (p->enc[i].cin != C || p->enc[i].cout != C) return false;
  }
  return true;
}

}  // namespace dstd
