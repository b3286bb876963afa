/*
 * dstd_gcn_predict.h -- any horizon from observed frames in one call: the
 * autoregressive rollout of the eval forward, chained on the device.
 *
 * The reference's model maps a window to a window (model/dstdgcn.py:293-317):
 * x [B][T][V][3] holds the input_n observed frames and then copies of the last
 * one (the datasets' i_idx padding), y is the whole window again.  To see
 * further than T - input_n frames a caller of the reference slices, concatenates
 * and re-pads in Python and calls the model once per window.  Here that loop is
 * one entry point.
 *
 * With T = p->T, Tin = input_n (1 <= Tin <= T - 1), Tout = T - Tin,
 * K = ceil(horizon / Tout) windows and m(s) = min(s, Tin - 1):
 *
 *   x_0[b][s]          = obs[b][m(s)]                            s = 0..T-1
 *   y_k                = DSTDGCN(x_k)                            as dstd_model_fwd_ex computes it
 *   seq_k[b][s]        = x_k[b][s] if s < Tin else y_k[b][s]     observations stay as given
 *   out[b][k*Tout + j] = y_k[b][Tin + j]                         j = 0..Tout-1 where k*Tout + j < horizon
 *   x_{k+1}[b][s]      = seq_k[b][T - Tin + m(s)]
 *
 * For Tin > Tout the observed part of the next window holds frames of x_k and
 * of y_k.  The last window is truncated to `horizon`.  The model's own
 * reconstruction of the observed frames (y_k[:, :Tin]) is never used.
 * horizon <= Tout is "the future of these frames" without a padded window
 * materialised by the caller.
 *
 * Conventions are those of dstd_gcn.h: device pointers to contiguous fp32, a
 * caller-owned workspace (base aligned to 256 bytes), no allocation, no state,
 * nothing synchronises, every launch is enqueued on `stream`, and the call can
 * be captured into a HIP graph on that one stream.  The same return codes.
 *
 * Workspace: the first dstd_model_workspace_bytes(...) bytes are the model
 * forward's region, laid out exactly as dstd_model_fwd_ex lays it out -- the
 * folded constants a plain forward left there can be reused by a predict on the
 * same buffer and the other way round (DSTD_FWD_REUSE_CONSTANTS).  After it, at
 * offsets rounded up to 256 bytes, two window buffers (x_{k+1} is built from x_k
 * and y_k, so they alternate) and one y buffer, B*T*V*3 floats each.
 *
 * Launches per call: the two parameter-preparation launches (unless
 * DSTD_FWD_REUSE_CONSTANTS), then K x (1 + the launches of one forward,
 * dstd_model_fwd_schedule), then 1: the window from obs, K forwards with one
 * launch between two of them that emits the earlier one's slice of out and
 * builds the later one's window, and one launch for the last slice.
 */
#ifndef DSTD_GCN_PREDICT_H
#define DSTD_GCN_PREDICT_H

#include "dstd_gcn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* More windows than this is DSTD_ELIMIT: a mistaken horizon must not enqueue
 * thousands of launches. */
#define DSTD_PREDICT_MAX_WINDOWS 64

/* rup(dstd_model_workspace_bytes(...), 256) + 3 * rup(B*T*V*3 * sizeof(float), 256) */
size_t dstd_model_predict_workspace_bytes(int B, int T, int V, int num_feature, int num_layers);

/* obs [B][input_n][V][3] -> out [B][horizon][V][3].  flags: those of
 * dstd_model_fwd_ex, handed to every window's forward; windows 1..K-1 also get
 * DSTD_FWD_REUSE_CONSTANTS (same parameters, batch and workspace within one
 * call), window 0 only if the caller passed it.  Checked before any launch, in
 * this order: DSTD_EINVAL for a NULL p / obs / out / workspace, input_n < 1,
 * input_n >= p->T, horizon < 1 or an unknown flag; DSTD_ELIMIT for more than
 * DSTD_PREDICT_MAX_WINDOWS windows; what dstd_model_fwd_ex returns for the
 * model's shape and pointers; DSTD_EWORKSPACE below the size above.  A refused
 * call writes nothing. */
int dstd_model_predict(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon, float* out,
                       void* workspace, size_t workspace_bytes, void* stream, unsigned flags);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_PREDICT_H */
