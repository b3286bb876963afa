// Host-side pieces of a differentiable chain of train forwards, shared by
// dstd_rollout.hip (the forward of every chain, and the backward of whole
// windows) and dstd_rollout_stride.hip (the backward of a stride): rounded
// model sizes, the per-window dropout seed, the layout of the saved region, the
// teacher of include/ext/dstd_gcn_teacher.h, and the checks and the order of
// the refusals of all three drivers.  `adv` below is the number of frames the
// chain advances per window: Tout, or the stride.
//
// Everything but chain_fwd has internal linkage, as dstd_window.h, which it follows.
#pragma once
#include "../../include/ext/dstd_gcn_teacher.h"
#include "dstd_window.h"

namespace dstd {

// A call's teacher arguments as the entry points take them (all zero: none).
struct TeacherArgs {
  const float* truth = nullptr;
  int truth_T = 0;
  const int *t0 = nullptr, *step = nullptr;
  const unsigned char* mask = nullptr;
};

// The forward of every chain (dstd_rollout.hip): dstd_model_rollout_fwd and
// _tf_fwd with adv = Tout, dstd_model_rollout_strided_fwd with adv = stride.
int chain_fwd(const dstd_model_params* p, const float* obs, int B, int Tin, int horizon, int adv, float momentum,
              float dropout_p, const unsigned long long* seeds, float* out, void* saved, size_t saved_bytes,
              const TeacherArgs& ta, void* stream, unsigned flags);

}  // namespace dstd

namespace {

size_t model_saved(int B, int T, int V, int C, int L) { return rup256(dstd_model_train_saved_bytes(B, T, V, C, L)); }
size_t model_ws(int B, int T, int V, int C, int L) { return rup256(dstd_model_train_workspace_bytes(B, T, V, C, L)); }

// window k's dropout seed as dstd_model_train_*_ex takes it: the value, or
// under DSTD_TRAIN_SEED_DEVICE the address of element k
unsigned long long seed_of(const unsigned long long* seeds, int k, unsigned flags) {
  if (!seeds) return 0ull;
  return (flags & DSTD_TRAIN_SEED_DEVICE) ? (unsigned long long)(uintptr_t)(seeds + k) : seeds[k];
}

// The saved region of a chain: y at 0, then per window x_k and the model's
// saved bytes (S of them).  The backwards only read through it.
struct ChainSaved {
  char* base;
  size_t W, S;
  ChainSaved(const void* saved, const dstd_model_params* p, int B)
      : base((char*)saved), W(window_bytes(B, p->T, p->V)),
        S(model_saved(B, p->T, p->V, p->num_feature, p->num_layers)) {}
  float* y() const { return (float*)base; }
  float* x(int k) const { return (float*)(base + W + (size_t)k * (W + S)); }
  void* saved(int k) const { return base + W + (size_t)k * (W + S) + W; }
};

// A model call's own verdict with the sizes taken out: the entry points look
// at saved_bytes last, so with 0 bytes they answer DSTD_EWORKSPACE exactly when
// nothing else is wrong, and launch nothing either way.
int chain_code(int probe, long long K) {
  if (probe == DSTD_EINVAL) return DSTD_EINVAL;
  if (K > DSTD_PREDICT_MAX_WINDOWS) return DSTD_ELIMIT;
  if (probe != DSTD_EWORKSPACE) return probe == DSTD_OK ? DSTD_EINVAL : probe;
  return DSTD_OK;
}

// The teacher of a call as the chain uses it (mask == nullptr: none).
struct Teacher {
  const float* truth = nullptr;
  const unsigned char* mask = nullptr;
  int truth_T = 0, t0[2] = {0, 0}, step[2] = {0, 0};
  // the half's truth frame of row 0 of window k
  int base(int h, int k, int adv) const { return t0[h] + step[h] * k * adv; }
  // row k of the mask for B samples, or nullptr without a teacher
  const unsigned char* row(int k, int B) const { return mask ? mask + (size_t)k * B : nullptr; }
};

// The teacher's own refusals (include/ext/dstd_gcn_teacher.h); Tin, adv and
// horizon have been checked.  Every frame a boundary can read lies between the
// two ends of tau = adv .. (K-1) * adv + Tin - 1, the map being monotonic.
int teacher_check(const dstd::TeacherArgs& a, unsigned flags, int Tin, int adv, long long K, Teacher* t) {
  if (!a.truth != !a.mask) return DSTD_EINVAL;
  if (!a.mask) return DSTD_OK;
  if (!a.t0 || !a.step || a.truth_T < 1) return DSTD_EINVAL;
  const int halves = (flags & DSTD_TRAIN_PAIRED) ? 2 : 1;
  for (int h = 0; h < halves; ++h) {
    if (a.step[h] != 1 && a.step[h] != -1) return DSTD_EINVAL;
    if (K > 1) {
      const long long lo = (long long)a.t0[h] + (long long)a.step[h] * adv;
      const long long hi = (long long)a.t0[h] + (long long)a.step[h] * ((K - 1) * adv + Tin - 1);
      if (lo < 0 || lo >= a.truth_T || hi < 0 || hi >= a.truth_T) return DSTD_EINVAL;
    }
    t->t0[h] = a.t0[h];
    t->step[h] = a.step[h];
  }
  t->truth = a.truth;
  t->mask = a.mask;
  t->truth_T = a.truth_T;
  return DSTD_OK;
}

// What chain_fwd and both backwards check alike once their own pointers are
// there, in the one order of the refusals: DSTD_EINVAL for the arguments, the
// seeds, window `only` (< 0: every window), the teacher and the model -- asked
// through probe(), a dstd_model_train_*_ex call with 0 saved bytes --, then
// DSTD_ELIMIT above DSTD_PREDICT_MAX_WINDOWS, then the model's own code, then
// DSTD_EWORKSPACE for saved_bytes.  On DSTD_OK: the K windows and the teacher.
template <class Probe>
int chain_open(const dstd_model_params* p, int B, int Tin, int horizon, int adv, int only, float dropout_p,
               const unsigned long long* seeds, const dstd::TeacherArgs& ta, unsigned flags, size_t saved_bytes,
               Probe probe, int* K, Teacher* tf) {
  if (Tin < 1 || Tin >= p->T || horizon < 1) return DSTD_EINVAL;
  if (adv < 1 || adv > p->T - Tin) return DSTD_EINVAL;
  if (dropout_p > 0.f && !seeds) return DSTD_EINVAL;
  const long long Kll = ((long long)horizon + adv - 1) / adv;
  if (only >= Kll) return DSTD_EINVAL;
  if (const int e = teacher_check(ta, flags, Tin, adv, Kll, tf)) return e;
  if (const int e = chain_code(probe(), Kll)) return e;
  *K = (int)Kll;
  if (saved_bytes < dstd_model_rollout_saved_bytes(B, p->T, p->V, p->num_feature, p->num_layers, *K))
    return DSTD_EWORKSPACE;
  return DSTD_OK;
}

}  // namespace
