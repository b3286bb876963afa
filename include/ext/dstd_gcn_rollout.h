/*
 * dstd_gcn_rollout.h -- train through the rollout: the autoregressive chain of
 * dstd_gcn_predict.h over the train-mode forward, and its backward.
 *
 * Why this header lives in include/ext/: tests/test_abi_host.py pins the
 * prototype, struct and define counts of every include/ (top level) header and
 * the key set of dstd_native.ABI, and this change may not edit it.  The
 * extension directory is outside that test's glob; the binding of this header
 * is dstd_native/ext.py, checked by tests/test_rollout_host.py.  Moving the
 * file up one level (and its table into dstd_native/abi.py) is a one-line
 * follow-up for whoever may edit that test.  For the same reason it brings no
 * struct and no #define: it reuses dstd_model_params, dstd_model_grads, the
 * DSTD_TRAIN_* flags, DSTD_PREDICT_MAX_WINDOWS and the error codes.
 *
 * Forward.  With T = p->T, Tin = input_n (1 <= Tin <= T - 1), Tout = T - Tin,
 * K = ceil(horizon / Tout) windows and m(s) = min(s, Tin - 1), the contract of
 * dstd_gcn_predict.h with one change:
 *
 *   y_k = dstd_model_train_fwd_ex(x_k, flags, momentum, dropout_p, seed_k)
 *
 * BatchNorm uses the batch statistics of each window (of each half under
 * DSTD_TRAIN_PAIRED) and the running statistics are updated K times in window
 * order; with DSTD_TRAIN_RUNNING_STATS it is the eval-mode forward under
 * autograd: no update, no dropout.
 *
 * Backward, given dout [B][horizon][V][3].  G_{k+1} is the gradient with
 * respect to x_{k+1}, G_K = 0 (no term).  For k = K-1 .. 0:
 *
 *   dy_k[b][s] = 0                                                          s <  Tin
 *   dy_k[b][s] = sum over s' with Tout + m(s') == s of G_{k+1}[b][s']
 *                + (dout[b][k*Tout + s - Tin] if k*Tout + s - Tin < horizon)  s >= Tin
 *   dx_k       = dstd_model_train_bwd_ex(x_k, saved_k, dy_k)     parameter gradients (+=) into g
 *   G_k[b][t]  = (G_{k+1}[b][t - Tout] if Tout <= t < Tin) + dx_k[b][t]
 *   dobs[b][i]     = G_0[b][i]                                    i < Tin - 1
 *   dobs[b][Tin-1] = sum_{s = Tin-1 .. T-1} G_0[b][s]
 *
 * Order of every sum: the G terms in ascending s' by sequential fp32 adds,
 * starting from the first term (an absent term is not a zero that is added),
 * then the dout term or the model's dx term last.  Only frame T - 1 of a
 * window (s' = Tin-1 .. T-1) and dobs[Tin-1] have more than two terms.  No
 * atomics: every output element is written by exactly one lane, and the
 * results are bit-reproducible.  dobs == NULL skips dx_0 and the G_0 / dobs
 * step.
 *
 * Conventions are those of dstd_gcn.h / dstd_gcn_train.h: device pointers to
 * contiguous fp32, caller-owned memory (bases aligned to 256 bytes), nothing
 * allocated, nothing synchronised, no state; every launch is enqueued on
 * `stream` (the model's own second stream unless DSTD_TRAIN_ONE_STREAM).  The
 * same return codes.  No dstd_bn_sync variant.
 *
 * saved (forward writes, backward reads; the backward reads nothing else of
 * the forward and leaves it unchanged), with W = rup(12*B*T*V, 256) and
 * S = rup(dstd_model_train_saved_bytes(B, T, V, num_feature, num_layers), 256):
 *
 *   [0, W)                             y scratch of the forward
 *   W + k*(W + S)      .. + W          x_k                      k = 0 .. K-1
 *   W + k*(W + S) + W  .. + S          window k's model saved region
 *
 * workspace (backward), with M = rup(dstd_model_train_workspace_bytes(...), 256):
 *
 *   [0, M)                             the model backward's workspace
 *   M, M + W, M + 2W                   dy_k, and the two buffers G_k / G_{k+1} alternate in
 *
 * Launches per call.  Forward: 1 (window 0 from obs) + K x (one train forward
 * + 1).  Backward: K x (1 + one model backward) + at most K-1 (the
 * pass-through fold, only where Tin > Tout and k < K-1) + 1 for dobs.
 */
#ifndef DSTD_GCN_ROLLOUT_H
#define DSTD_GCN_ROLLOUT_H

#include "../dstd_gcn_predict.h"
#include "../dstd_gcn_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* W + windows * (W + S), as laid out above (windows < 0 counts as 0). */
size_t dstd_model_rollout_saved_bytes(int B, int T, int V, int num_feature, int num_layers, int windows);
/* M + 3 * W */
size_t dstd_model_rollout_workspace_bytes(int B, int T, int V, int num_feature, int num_layers);

/* obs [B][input_n][V][3] -> out [B][horizon][V][3].  flags: exactly those of
 * dstd_model_train_fwd_ex, handed to every window.  seeds: K values on the host;
 * under DSTD_TRAIN_SEED_DEVICE a device array of K uint64 of which window k
 * reads element k; may be NULL when dropout_p == 0.
 * Checked before any launch, in this order: DSTD_EINVAL for a NULL p / obs /
 * out / saved, input_n < 1, input_n >= p->T, horizon < 1, NULL seeds with
 * dropout_p > 0, and whatever dstd_model_train_fwd_ex answers DSTD_EINVAL for
 * (pointers, dropout_p, flags, an odd B under DSTD_TRAIN_PAIRED, the shape);
 * DSTD_ELIMIT for more than DSTD_PREDICT_MAX_WINDOWS windows, then for the
 * model's envelope; DSTD_EWORKSPACE for saved_bytes below
 * dstd_model_rollout_saved_bytes(..., K).  A refused call launches nothing and
 * writes nothing. */
int dstd_model_rollout_fwd(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon,
                           float momentum, float dropout_p, const unsigned long long* seeds, float* out,
                           void* saved, size_t saved_bytes, void* stream, unsigned flags);

/* The backward of the call above: the same p, B, input_n, horizon, dropout_p,
 * seeds (before the values change) and flags.  g accumulates (+=) over the
 * windows, K-1 first; dobs [B][input_n][V][3] is assigned (=) and may be NULL.
 * Refusals as above with dout / g / workspace among the pointers, then
 * DSTD_EWORKSPACE for saved_bytes, then for workspace_bytes below
 * dstd_model_rollout_workspace_bytes(...). */
int dstd_model_rollout_bwd(const dstd_model_params* p, int B, int input_n, int horizon, float dropout_p,
                           const unsigned long long* seeds, const void* saved, size_t saved_bytes, const float* dout,
                           const dstd_model_grads* g, float* dobs, void* workspace, size_t workspace_bytes,
                           void* stream, unsigned flags);

/* The same backward one window per call, for a caller that wants each window's
 * parameter gradients in a g of its own (autograd's accumulation of K separate
 * backwards sums them per window first: a gradient that two operators of a
 * window add into, alpha_sm, then rounds differently from the one (+=) chain
 * above).  Window k finds G_{k+1} in the workspace, where the call for window
 * k + 1 left it, and leaves G_k there: call k = K-1 .. 0 with the same
 * arguments and workspace and nothing else using the workspace in between.
 * dobs is written by window 0 alone (NULL there: dx_0 is skipped).
 * dstd_model_rollout_bwd is this loop with one g.  Refusals as above, and
 * DSTD_EINVAL for k outside 0 .. K-1. */
int dstd_model_rollout_bwd_window(const dstd_model_params* p, int B, int input_n, int horizon, int k, float dropout_p,
                                  const unsigned long long* seeds, const void* saved, size_t saved_bytes,
                                  const float* dout, const dstd_model_grads* g, float* dobs, void* workspace,
                                  size_t workspace_bytes, void* stream, unsigned flags);

/* Test hook: one launch of the backward's glue on caller-made buffers, so that
 * its sums can be checked on arbitrary G (a model's dx is not arbitrary) and at
 * any V.  Windows are [B][T][V][3], window k of K = ceil(horizon / (T - input_n)).
 *   step 0: dst = dy_k from dout [B][horizon][V][3] and Gn = G_{k+1} (NULL: no term)
 *   step 1: dst = G_k, holding dx_k on entry, with Gn = G_{k+1} folded in (nothing
 *           to do, and no launch, where input_n <= T - input_n)
 *   step 2: dst = dobs [B][input_n][V][3] from Gn = G_0
 * dout is read by step 0 alone.  DSTD_EINVAL for a NULL pointer the step reads or
 * writes, a non-positive B or V, input_n outside 1 .. T-1, horizon < 1, k outside
 * 0 .. K-1 or an unknown step. */
int dstd_model_rollout_glue_bwd(int step, const float* dout, const float* Gn, float* dst, int B, int T, int input_n,
                                int V, int horizon, int k, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_ROLLOUT_H */
