/*
 * dstd_gcn_eval.h -- C ABI of grouped evaluation: the per-frame test metric of
 * a batch drawn from a device-resident set (dstd_gcn_data.h), accumulated per
 * group (an action of H36M / CMU) by one launch that reads the targets straight
 * from the resident frames.
 *
 * The reference's runners build the protocol's table -- one row per action, one
 * column per evaluated frame -- by one PredictionEngine.test per action
 * (runner/h36m.py:106-135).  Here the windows of a resident set carry a group,
 * a batch mixes groups freely, and sums[group][frame] / counts[group] accumulate
 * on the device: all_seqs is never materialised and the host synchronises once
 * for the whole table.
 *
 * Conventions as in dstd_gcn_data.h and dstd_gcn_train.h (error codes in
 * dstd_gcn.h): device pointers to contiguous fp32 / int / long long, enqueue on
 * `stream`, one launch, no workspace, no allocation and no state inside the
 * library.  The dstd_seq_store itself is host memory, read before the call
 * returns.  Every element offset is 64-bit.  sums and counts accumulate (+=):
 * the caller zeroes them once.  One workgroup owns each (group, frame) pair and
 * sums in a fixed order -- no float atomics -- so a result is bit-reproducible.
 */
#ifndef DSTD_GCN_EVAL_H
#define DSTD_GCN_EVAL_H

#include "../dstd_gcn_data.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DSTD_EVAL_MAX_GROUPS 1024

/* PredictionEngine.test's metric (engine/prediction.py:366-404) for one batch drawn from a
 * resident set, per group:
 *   sums[g * n_frames + k] += (1/J) * sum over the batch rows b of group g, over joints j,
 *                             of || targ(b, frames[k], j) - pred(b, frames[k], j) ||
 *   counts[g]              += number of batch rows of group g
 * targ(b, f, :) is window index[b] of the store at window frame f, exactly the row
 * dstd_batch_gather would write to all_seqs[b][f][:] (mirrored windows included; `used` is
 * never read: all_seqs is unscaled).  pred is dstd_frame_mpjpe's fill: column d of joint
 * joint_src[j] comes from outputs[b][f - t_out0][used_pos[d]] when used_pos[d] >= 0 and
 * f >= t_out0, from targ otherwise.  J = D / 3, outputs [B][T - t_out0][n_used].
 * group: device int [number of window indices: N, or 2N with mirror_src], or NULL (every
 * window is group 0).  A row whose index is outside the store, or whose group is outside
 * [0, n_groups), is skipped: not summed, not counted, nothing read for it.
 *
 * With group == NULL, n_groups == 1 and every index valid, sums is bit-identical to
 * dstd_frame_mpjpe on the all_seqs that dstd_batch_gather writes for the same index: the
 * element loop and the reduction are that kernel's.
 *
 * DSTD_EINVAL, no launch and nothing written, for: a NULL store, frames (of the store),
 * starts, index, outputs, used_pos, joint_src, frames, sums or counts; B, n_frames,
 * n_groups or n_used <= 0; t_out0 outside [0, T); D < 3 or D % 3 != 0, T < 1, F < 1, N < 1.
 * DSTD_ELIMIT for n_groups > DSTD_EVAL_MAX_GROUPS, or B * J beyond an int.  On the device, a
 * frame outside [0, T),
 * a used_pos >= n_used, a joint_src or mirror source outside [0, J) or a window start
 * outside the stored frames writes nothing for what it concerns and reads nothing out of
 * bounds, as in dstd_batch_gather. */
int dstd_store_group_mpjpe(const dstd_seq_store* s, const long long* index, int B,
                           const float* outputs, int t_out0, const int* used_pos, int n_used,
                           const int* joint_src, const int* frames, int n_frames,
                           const int* group, int n_groups, float* sums, int* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_EVAL_H */
