/*
 * dstd_gcn_stride.h -- predict with a stride: every window contributes its
 * first `stride` predicted frames, and the next window observes the last
 * input_n frames of what is known by then.
 *
 * dstd_model_predict (../dstd_gcn_predict.h) keeps all Tout frames of a window
 * and feeds the last input_n of them back: the frames a window is least sure
 * of.  The usual way to look further with a short-term model keeps only the
 * first few frames of each window and slides the observation forward by that
 * many.  Here that loop is one entry point.
 *
 * With T = p->T, Tin = input_n (1 <= Tin <= T - 1), Tout = T - Tin,
 * S = stride (1 <= S <= Tout), H = horizon, K = ceil(H / S) windows,
 * m(s) = min(s, Tin - 1), and the known sequence h of Tin + H frames,
 * h[b][i] = obs[b][i] for i < Tin and h[b][Tin + f] = out[b][f]:
 *
 *   x_k[b][s]        = h[b][k*S + m(s)]                s = 0..T-1
 *   y_k              = DSTDGCN(x_k)                    as dstd_model_fwd_ex computes it
 *   out[b][k*S + j]  = y_k[b][Tin + j]                 j = 0..S-1 while k*S + j < H
 *
 * Window k needs h up to k*S + Tin - 1, which is exactly what windows 0..k-1
 * have produced.  For S = Tout this is the chain of ../dstd_gcn_predict.h,
 * frame for frame.  The observed frames of a window may come from three places
 * at once: obs (while k*S < Tin), frames of out that earlier windows wrote, and
 * frames of y_k that the same launch is emitting.  y_k[:, :Tin] and
 * y_k[:, Tin+S:] are never used.
 *
 * Conventions, flags and return codes are those of dstd_model_predict: device
 * pointers to contiguous fp32, a caller-owned workspace (base aligned to 256
 * bytes), no allocation, no state, nothing synchronises, every launch is
 * enqueued on `stream`, and the call can be captured into a HIP graph on that
 * one stream.
 *
 * Workspace: the first dstd_model_workspace_bytes(...) bytes are the model
 * forward's region, laid out exactly as dstd_model_fwd_ex lays it out, so
 * DSTD_FWD_REUSE_CONSTANTS works across a plain forward, dstd_model_predict and
 * this call on one buffer.  After it, at offsets rounded up to 256 bytes, one
 * window buffer x and one y buffer, B*T*V*3 floats each: x_{k+1} reads nothing
 * of x_k, so the windows do not alternate.
 *
 * out must not alias obs or the workspace: later windows read frames of out
 * that earlier launches of the same call wrote.  This is not checked.
 *
 * Launches per call: those of ../dstd_gcn_predict.h with this K -- the two
 * parameter-preparation launches (unless DSTD_FWD_REUSE_CONSTANTS), then
 * K x (1 + the launches of one forward), then 1: the window from obs, K
 * forwards with one launch between two of them that emits the earlier one's
 * frames and builds the later one's window, and one launch for the last frames.
 *
 * DSTD_PREDICT_MAX_WINDOWS stays 64 and bounds K = ceil(H / S): H = 100 needs
 * S >= 2, H = 1000 needs S >= 16.
 */
#ifndef DSTD_GCN_STRIDE_H
#define DSTD_GCN_STRIDE_H

#include "../dstd_gcn_predict.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rup(dstd_model_workspace_bytes(...), 256) + 2 * rup(B*T*V*3 * sizeof(float), 256):
 * never more than dstd_model_predict_workspace_bytes of the same arguments. */
size_t dstd_model_predict_strided_workspace_bytes(int B, int T, int V, int num_feature, int num_layers);

/* obs [B][input_n][V][3] -> out [B][horizon][V][3].  flags: those of
 * dstd_model_fwd_ex, handed to every window's forward; windows 1..K-1 also get
 * DSTD_FWD_REUSE_CONSTANTS, window 0 only if the caller passed it.  Checked
 * before any launch, in the order of dstd_model_predict: DSTD_EINVAL for a NULL
 * p / obs / out / workspace, input_n < 1, input_n >= p->T, horizon < 1,
 * stride < 1, stride > p->T - input_n or an unknown flag; DSTD_ELIMIT for more
 * than DSTD_PREDICT_MAX_WINDOWS windows; what dstd_model_fwd_ex returns for the
 * model's shape and pointers; DSTD_EWORKSPACE below the size above.  A refused
 * call writes nothing. */
int dstd_model_predict_strided(const dstd_model_params* p, const float* obs, int B, int input_n, int horizon,
                               int stride, float* out, void* workspace, size_t workspace_bytes, void* stream,
                               unsigned flags);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_STRIDE_H */
