// Host-side pieces of a differentiable chain of train forwards, shared by
// dstd_rollout.hip (whole windows) and dstd_rollout_stride.hip (a stride):
// rounded model sizes, the per-window dropout seed, the order of the refusals,
// and the teacher of include/ext/dstd_gcn_teacher.h.  `adv` below is the
// number of frames the chain advances per window: Tout, or the stride.
//
// Everything here has internal linkage, as dstd_window.h, which it follows.
#pragma once
#include "../../include/ext/dstd_gcn_teacher.h"
#include "dstd_window.h"

namespace {

size_t model_saved(int B, int T, int V, int C, int L) { return rup256(dstd_model_train_saved_bytes(B, T, V, C, L)); }
size_t model_ws(int B, int T, int V, int C, int L) { return rup256(dstd_model_train_workspace_bytes(B, T, V, C, L)); }

// window k's dropout seed as dstd_model_train_*_ex takes it: the value, or
// under DSTD_TRAIN_SEED_DEVICE the address of element k
unsigned long long seed_of(const unsigned long long* seeds, int k, unsigned flags) {
  if (!seeds) return 0ull;
  return (flags & DSTD_TRAIN_SEED_DEVICE) ? (unsigned long long)(uintptr_t)(seeds + k) : seeds[k];
}

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
};

// The teacher's own refusals (include/ext/dstd_gcn_teacher.h); Tin, adv and
// horizon have been checked.  Every frame a boundary can read lies between the
// two ends of tau = adv .. (K-1) * adv + Tin - 1, the map being monotonic.
int teacher_check(const float* truth, int truth_T, const int* t0, const int* step, const unsigned char* mask,
                  unsigned flags, int Tin, int adv, long long K, Teacher* t) {
  if (!truth != !mask) return DSTD_EINVAL;
  if (!mask) return DSTD_OK;
  if (!t0 || !step || truth_T < 1) return DSTD_EINVAL;
  const int halves = (flags & DSTD_TRAIN_PAIRED) ? 2 : 1;
  for (int h = 0; h < halves; ++h) {
    if (step[h] != 1 && step[h] != -1) return DSTD_EINVAL;
    if (K > 1) {
      const long long a = (long long)t0[h] + (long long)step[h] * adv;
      const long long b = (long long)t0[h] + (long long)step[h] * ((K - 1) * adv + Tin - 1);
      if (a < 0 || a >= truth_T || b < 0 || b >= truth_T) return DSTD_EINVAL;
    }
    t->t0[h] = t0[h];
    t->step[h] = step[h];
  }
  t->truth = truth;
  t->mask = mask;
  t->truth_T = truth_T;
  return DSTD_OK;
}

}  // namespace
