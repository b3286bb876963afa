/*
 * dstd_gcn_teacher.h -- scheduled sampling for the rollout of
 * dstd_gcn_rollout.h: at a window boundary some samples take the ground truth
 * as their next window instead of the model's predictions, with no gradient
 * through that boundary.
 *
 * In include/ext/ for the reason dstd_gcn_rollout.h gives; no struct and no
 * #define of its own either.  Its binding is dstd_native/ext.py (TEACHER_ABI),
 * checked by tests/test_teacher_host.py.
 *
 * This extends the contract of dstd_gcn_rollout.h and uses its symbols: T, Tin,
 * Tout, K, m(s) = min(s, Tin - 1), x_k, y_k, seq_k, G_k.
 *
 * Inputs, both the caller's, both on the device:
 *
 *   truth [Bt][truth_T][V][3]   fp32, in the model's input layout.  Bt = B, or
 *                               B / 2 under DSTD_TRAIN_PAIRED: both halves read
 *                               one truth tensor.
 *   t0[h], step[h]              host arrays, one frame map per half (element 0
 *                               alone without DSTD_TRAIN_PAIRED), step = +1 or
 *                               -1.  Sample b belongs to half h = b / Bt; its
 *                               truth frame at rollout time tau is
 *                               truth[b mod Bt][t0[h] + step[h] * tau].  tau = 0
 *                               is the first observed frame, tau = Tin + j is
 *                               predicted frame j.
 *   mask [K][B]                 uint8.  Row k belongs to the boundary INTO
 *                               window k; row 0 is never read.
 *
 * Forward.  Window 0, y_k and out are those of dstd_gcn_rollout.h; out is
 * always the model's prediction, never truth.  For k >= 0:
 *
 *   x_{k+1}[b][s] = seq_k[b][T - Tin + m(s)]                                  mask[k+1][b] == 0
 *   x_{k+1}[b][s] = truth[b mod Bt][t0[h] + step[h] * ((k+1)*Tout + m(s))]    otherwise
 *
 * (all Tin observed frames of a forced sample and its padding).  One launch
 * per boundary, as in the free-running chain: the launch that emits window k's
 * slice of out builds x_{k+1} from either source.
 *
 * Backward.  A forced sample's window k + 1 does not depend on x_k or y_k: for
 * those b the G_{k+1} terms are absent from dy_k[b] and from the pass-through
 * into G_k[b] (absent, not an added zero).  Everything else is as in
 * dstd_gcn_rollout.h: the order of every sum, the dout / dx term last, dobs
 * from G_0, one lane per output element, no atomics, bit-reproducible.  There
 * is no gradient to truth.
 *
 * Memory.  saved and the workspace are exactly those of
 * dstd_model_rollout_saved_bytes / dstd_model_rollout_workspace_bytes, with the
 * same layout: this header needs no size export.  The mask and the truth stay
 * the caller's; neither is copied.  The backward reads mask again (never
 * truth), so the caller keeps the mask alive and unchanged until the backward
 * has run.  Launches per call are those of dstd_gcn_rollout.h.
 *
 * Refusals.  Those of the entry point each one mirrors, in their order, and
 * DSTD_EINVAL -- before any launch, among the argument errors, so before the
 * window cap and the sizes -- for
 *   - truth NULL with mask non-NULL, or the reverse;
 *   - with a truth: NULL t0 or step, truth_T < 1, a step that is not +1 or -1
 *     (of a half the call has);
 *   - any frame the call could read outside [0, truth_T): the reads span
 *     tau = Tout .. (K-1)*Tout + Tin - 1 (none when K == 1), so
 *     truth_T >= Tin + horizon always suffices for the maps (0, +1) and
 *     (truth_T - 1, -1).
 * A refused call launches nothing and writes nothing.  With truth and mask
 * both NULL every entry point is the one it mirrors: the same launches.
 */
#ifndef DSTD_GCN_TEACHER_H
#define DSTD_GCN_TEACHER_H

#include "dstd_gcn_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dstd_model_rollout_fwd with a teacher. */
int dstd_model_rollout_tf_fwd(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon,
                              float momentum, float dropout_p, const unsigned long long* seeds, float* out,
                              void* saved, size_t saved_bytes, const float* truth, int truth_T, const int* t0,
                              const int* step, const unsigned char* mask, void* stream, unsigned flags);

/* dstd_model_rollout_bwd of the call above: the same truth_T, t0, step and
 * mask (checked as there; mask is read, truth is not). */
int dstd_model_rollout_tf_bwd(const dstd_model_params* p, int B, int input_n, int horizon, float dropout_p,
                              const unsigned long long* seeds, const void* saved, size_t saved_bytes,
                              const float* dout, const dstd_model_grads* g, float* dobs, void* workspace,
                              size_t workspace_bytes, const float* truth, int truth_T, const int* t0, const int* step,
                              const unsigned char* mask, void* stream, unsigned flags);

/* dstd_model_rollout_bwd_window likewise: window k reads row k + 1 of mask. */
int dstd_model_rollout_tf_bwd_window(const dstd_model_params* p, int B, int input_n, int horizon, int k,
                                     float dropout_p, const unsigned long long* seeds, const void* saved,
                                     size_t saved_bytes, const float* dout, const dstd_model_grads* g, float* dobs,
                                     void* workspace, size_t workspace_bytes, const float* truth, int truth_T,
                                     const int* t0, const int* step, const unsigned char* mask, void* stream,
                                     unsigned flags);

/* Test hook: dstd_model_rollout_glue_bwd with one row of the mask.  The glue of
 * the backward reads no truth and no frame map, so of the teacher's arguments
 * the hook takes the row alone: mask_row [B] is row k + 1 of a mask, the
 * boundary whose gradient Gn = G_{k+1} is.  Steps 0 and 1 skip the Gn terms of
 * the samples it forces (step 1 then leaves their rows of dst as they are);
 * step 2 does not read it.  mask_row == NULL: the free-running hook. */
int dstd_model_rollout_tf_glue_bwd(int step, const float* dout, const float* Gn, float* dst,
                                   const unsigned char* mask_row, int B, int T, int input_n, int V, int horizon,
                                   int k, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_TEACHER_H */
