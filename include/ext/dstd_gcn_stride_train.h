/*
 * dstd_gcn_stride_train.h -- train through a strided rollout: the chain of
 * dstd_gcn_stride.h over the train-mode forward, its backward, and scheduled
 * sampling (the teacher of dstd_gcn_teacher.h) at its window boundaries.
 *
 * In include/ext/ for the reason dstd_gcn_rollout.h gives; no struct and no
 * #define of its own.  Its binding is dstd_native/ext_stride_train.py, checked
 * by tests/test_rollout_stride_host.py.
 *
 * Notation is that of dstd_gcn_stride.h: T = p->T, Tin = input_n, Tout = T - Tin,
 * S = stride (1 <= S <= Tout), H = horizon, K = ceil(H / S) windows
 * (K <= DSTD_PREDICT_MAX_WINDOWS), m(s) = min(s, Tin - 1), and the known
 * sequence h of Tin + H frames, h[b][i] = obs[b][i] for i < Tin and
 * h[b][Tin + f] = out[b][f] (but for the frames a teacher replaces, below).
 *
 * Forward.  The chain of dstd_gcn_stride.h with
 *
 *   y_k = dstd_model_train_fwd_ex(x_k, flags, momentum, dropout_p, seed_k)
 *
 * Batch statistics per window (per half under DSTD_TRAIN_PAIRED), the running
 * statistics updated K times in window order, one dropout seed per window;
 * with DSTD_TRAIN_RUNNING_STATS the eval forward under autograd.  Every x_k is
 * kept: saved is laid out as dstd_gcn_rollout.h lays it out, with this K
 * (dstd_model_rollout_saved_bytes(..., K)).
 *
 * Teacher (optional; truth, truth_T, t0[], step[], mask [K][B] uint8 as in
 * dstd_gcn_teacher.h, all NULL: free running).  Where mask[k][b] is set, k >= 1:
 *
 *   x_k[b][s] = truth[b mod Bt][t0[h] + step[h] * (k*S + m(s))]
 *
 * and, as in dstd_gcn_teacher.h, those frames are what sample b knows from then
 * on: h[b][k*S + i] = x_k[b][i], i < Tin, for every later window (the next
 * window is built from x_k below Tin and y_k from Tin on, so with S < Tin a
 * free window after a forced one observes the truth's frames next to the
 * frames predicted from them, not predictions made before the forcing).  Row
 * 0 of the mask is not read.  The reads span rollout times
 * tau = S .. (K-1)*S + Tin - 1 (none when K == 1), so truth_T >= Tin + H
 * suffices for the maps (0, +1) and (truth_T - 1, -1).  out is always the
 * model's prediction.  The backward reads the mask again and never truth.
 *
 * Backward, given dout [B][H][V][3].  A gradient history Gh [B][Tin + H][V][3]
 * lives in the workspace and starts at +0.  For k = K-1 .. 0:
 *
 *   dy_k[b][s] = Gh[b][k*S + s] + dout[b][k*S + s - Tin]   Tin <= s < Tin + S and k*S + s - Tin < H
 *   dy_k[b][s] = 0                                         every other s
 *   dx_k       = dstd_model_train_bwd_ex(x_k, saved_k, dy_k)     parameter gradients (+=) into g
 *   where (k >= 1 and mask[k][b]):             a forced window hands nothing back,
 *     Gh[b][k*S + i] = +0                      i < Tin           nor does a later one through its frames
 *   elsewhere:
 *     Gh[b][k*S + i] += dx_k[b][i]                               i < Tin - 1
 *     acc = Gh[b][k*S + Tin - 1]; for s = Tin-1 .. T-1 ascending: acc = acc + dx_k[b][s];
 *     Gh[b][k*S + Tin - 1] = acc
 *   dobs[b][i] = Gh[b][i]                                        i < Tin, after window 0
 *
 * Gh[k*S + s] is complete when window k reads it: only windows after k read h
 * at frames >= Tin + k*S.  The frames a forced window k replaced were read as
 * truth by window k and by every later window, so what those have summed into
 * their rows is dropped there, before any earlier window -- which read the
 * predictions -- adds to them.  Every sum is one lane's sequential fp32 chain in
 * the order written; no atomics; every element of Gh, dy and dobs is written by
 * one lane per launch; the results are bit-reproducible.  dobs == NULL skips
 * dx_0.  At S = Tout the call computes, term for term, what
 * dstd_model_rollout_fwd / _bwd (with a mask: _tf_fwd / _tf_bwd) compute, for
 * Tin <= Tout and for Tin > Tout (where a term is absent there, a +0 stands
 * first in the sum here: equal under ==, a -0 may come out +0).
 *
 * Conventions and return codes are those of dstd_gcn_rollout.h.  out must not
 * alias obs, saved or the workspace.
 *
 * workspace (backward), with M = rup(dstd_model_train_workspace_bytes(...), 256)
 * and W = rup(12*B*T*V, 256):
 *
 *   [0, M)                the model backward's workspace
 *   M, M + W              dy_k, dx_k
 *   M + 2W ..             Gh, rup(12*B*(Tin + H)*V, 256) bytes
 *
 * Launches per call.  Forward: 1 (window 0 from obs) + K x (one train forward
 * + 1).  Backward: 1 (Gh = 0) + K x (1 + one model backward + 1); the launch
 * after window 0's backward also writes dobs, and with dobs == NULL it is not
 * made.  "Accumulate window k" and "build dy_{k-1}" are two launches.
 */
#ifndef DSTD_GCN_STRIDE_TRAIN_H
#define DSTD_GCN_STRIDE_TRAIN_H

#include "dstd_gcn_stride.h"
#include "dstd_gcn_teacher.h"

#ifdef __cplusplus
extern "C" {
#endif

/* M + 2 * W + rup(12*B*(input_n + horizon)*V, 256), as laid out above
 * (input_n + horizon < 0 counts as 0). */
size_t dstd_model_rollout_strided_workspace_bytes(int B, int T, int V, int num_feature, int num_layers, int input_n,
                                                  int horizon);

/* obs [B][input_n][V][3] -> out [B][horizon][V][3].  flags and seeds as
 * dstd_model_rollout_fwd (K seeds).  Checked before any launch, in this order:
 * DSTD_EINVAL for a NULL p / obs / out / saved, input_n < 1, input_n >= p->T,
 * horizon < 1, stride outside 1 .. p->T - input_n, NULL seeds with
 * dropout_p > 0, whatever dstd_model_train_fwd_ex answers DSTD_EINVAL for and
 * the teacher's refusals (dstd_gcn_teacher.h, with the span above); DSTD_ELIMIT
 * for more than DSTD_PREDICT_MAX_WINDOWS windows, then for the model's
 * envelope; DSTD_EWORKSPACE for saved_bytes below
 * dstd_model_rollout_saved_bytes(..., K).  A refused call launches nothing and
 * writes nothing. */
int dstd_model_rollout_strided_fwd(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon,
                                   int stride, float momentum, float dropout_p, const unsigned long long* seeds,
                                   float* out, void* saved, size_t saved_bytes, const float* truth, int truth_T,
                                   const int* t0, const int* step, const unsigned char* mask, void* stream,
                                   unsigned flags);

/* The backward of the call above, with the same arguments: g accumulates (+=)
 * over the windows, K-1 first; dobs [B][input_n][V][3] is assigned (=) and may
 * be NULL.  Refusals as above with dout / g / workspace among the pointers,
 * then DSTD_EWORKSPACE for saved_bytes, then for workspace_bytes below
 * dstd_model_rollout_strided_workspace_bytes(...). */
int dstd_model_rollout_strided_bwd(const dstd_model_params* p, int B, int input_n, int horizon, int stride,
                                   float dropout_p, const unsigned long long* seeds, const void* saved,
                                   size_t saved_bytes, const float* dout, const dstd_model_grads* g, float* dobs,
                                   void* workspace, size_t workspace_bytes, const float* truth, int truth_T,
                                   const int* t0, const int* step, const unsigned char* mask, void* stream,
                                   unsigned flags);

/* The same backward one window per call, for a g per window (see
 * dstd_model_rollout_bwd_window).  The call for window K-1 zeroes Gh; Gh stays
 * in the workspace between calls: call k = K-1 .. 0 with the same arguments and
 * workspace and nothing else using the workspace in between.  dobs is written
 * by window 0 alone (NULL there: dx_0 is skipped).
 * dstd_model_rollout_strided_bwd is this loop with one g.  Refusals as above,
 * and DSTD_EINVAL for k outside 0 .. K-1. */
int dstd_model_rollout_strided_bwd_window(const dstd_model_params* p, int B, int input_n, int horizon, int stride,
                                          int k, float dropout_p, const unsigned long long* seeds, const void* saved,
                                          size_t saved_bytes, const float* dout, const dstd_model_grads* g,
                                          float* dobs, void* workspace, size_t workspace_bytes, const float* truth,
                                          int truth_T, const int* t0, const int* step, const unsigned char* mask,
                                          void* stream, unsigned flags);

/* Test hook: one launch of the backward's glue on caller-made buffers, at any
 * V.  Gh is [B][input_n + horizon][V][3], windows are [B][T][V][3], window k of
 * K = ceil(horizon / stride).
 *   step 0: dst = dy_k from Gh and dout [B][horizon][V][3]
 *   step 1: dx = dx_k accumulated into Gh; the Tin rows of a sample that mask_row
 *           forces become +0 instead (mask_row [B]: row k of a mask, read only
 *           where k >= 1; NULL: none);
 *           with k == 0 and dst != NULL also dst = dobs [B][input_n][V][3]
 * DSTD_EINVAL for a NULL pointer the step reads or writes, a non-positive B or
 * V, input_n outside 1 .. T-1, horizon < 1, stride outside 1 .. T - input_n,
 * k outside 0 .. K-1 or an unknown step. */
int dstd_model_rollout_strided_glue_bwd(int step, const float* dout, const float* dx, float* Gh, float* dst,
                                        const unsigned char* mask_row, int B, int T, int input_n, int V, int horizon,
                                        int stride, int k, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_STRIDE_TRAIN_H */
