/*
 * dstd_gcn_loss.h -- C ABI of the engine's weighted, multi-term training loss.
 *
 * The reference's ModelWrapper sums config-weighted loss functions
 * (engine/prediction.py:29-34 -> engine/utils/loss.py); these entry points
 * evaluate any subset of them in one pass over the prediction, for the batch
 * and (optionally) its time reversal together:
 *
 *   DSTD_LOSS_JL2  <- mpjpe_error_3d       engine/utils/loss.py:52-65
 *   DSTD_LOSS_TL2  <- transition_error_3d  engine/utils/loss.py:129-146
 *   DSTD_LOSS_CL1  <- mae_error_3d         engine/utils/loss.py:24-35
 *   DSTD_LOSS_CL2  <- mse_error_3d         engine/utils/loss.py:38-49
 *
 * With d = pred - targ per joint (a 3-vector), joint weights w_j >= 0 (all 1
 * when joint_w is NULL), wbar = mean_j w_j and N = B*T*V:
 *
 *   jl2 = wbar / N            * sum w_j ||d||
 *   tl2 = wbar / (B (T-1) V)  * sum_{s < T-1} w_j ||d_{s+1} - d_s||
 *   cl1 = cl2 = 1 / (3 N)     * sum w_j |d_c|
 *
 * (wbar is the reference's `* body_weights` broadcast on the flattened norms;
 * its cl2 takes sqrt((w d)^2), the same value as cl1.)  Gradients follow
 * torch: 0 where a norm is 0, sign(0) = 0.  cl2 deviates on purpose: the
 * reference's autograd gives NaN where w_j d_c == 0, this gives 0.
 *
 * Conventions as in dstd_gcn.h / dstd_gcn_train.h (error codes there): device
 * pointers to contiguous fp32, caller-owned workspace, enqueue on `stream`,
 * no allocation and no state inside the library.  The dstd_loss_problem array
 * itself is host memory, read before the call returns.  Reductions run in a
 * fixed order without float atomics: results are bit-reproducible.
 */
#ifndef DSTD_GCN_LOSS_H
#define DSTD_GCN_LOSS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSTD_LOSS_JL2 1u
#define DSTD_LOSS_TL2 2u
#define DSTD_LOSS_CL1 4u
#define DSTD_LOSS_CL2 8u
#define DSTD_LOSS_NTERMS 4 /* slot k of a values / coef row belongs to term bit 1u << k */

/* pred [B][T][V][3]; targ [B][targ_T][V][3].  pred frame s pairs with targ
 * frame targ_t0 + targ_step * s, targ_step = +1 or -1: targets[:, -T:] is
 * (targ_T - T, +1), targets.flip(1)[:, -T:] is (T - 1, -1). */
typedef struct dstd_loss_problem {
  const float* pred;
  const float* targ;
  int B, T, V;
  int targ_T, targ_t0, targ_step;
} dstd_loss_problem;

size_t dstd_losses_workspace_bytes(void);

/* values[p * DSTD_LOSS_NTERMS + k] = term k of problem p; slots of terms not in
 * `terms` are written 0.  n_problems is 1 or 2 (same V); joint_w [V] or NULL.
 * Two launches whatever `terms` and n_problems are. */
int dstd_losses_fwd(const dstd_loss_problem* problems, int n_problems, unsigned terms, const float* joint_w,
                    float* values, void* workspace, size_t workspace_bytes, void* stream);

/* dpreds[p] (=) scale * sum_k coef[p * DSTD_LOSS_NTERMS + k] * d value_k / d pred of
 * problem p, over the terms in `terms` (coef: device, upstream gradient x
 * config weight; other slots are not read).  dpreds: host array of n_problems
 * device pointers shaped like pred.  One launch. */
int dstd_losses_bwd(const dstd_loss_problem* problems, int n_problems, unsigned terms, const float* joint_w,
                    const float* coef, float scale, float* const* dpreds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_LOSS_H */
