/*
 * dstd_gcn_warp.h -- C ABI of the warping gather: the batch that
 * dstd_batch_gather_aug (dstd_gcn_augment.h) assembles from a device-resident
 * set, with every window resampled in time at a per-sample playback rate in
 * the same launch.
 *
 * Playing a motion faster or slower is the routine augmentation on the time
 * axis.  A faster window needs frames that lie after the window in its
 * recording, which only the resident set holds (a set built from whole
 * sequences stores every frame once), and the gather already knows the
 * window's start row, the frame maps, the mirror, the transform and the noise
 * keys: it reads two neighbouring source frames and blends them where it read
 * one, so all_seqs, targets, inputs and inputs_inv are views of one warped
 * window by construction.
 *
 * dstd_seq_store, index, the four outputs, NULL outputs, the mirrored half
 * N <= w < 2N and "an index, a start or a table entry outside its range writes
 * nothing and reads nothing out of bounds" are exactly as in dstd_gcn_data.h;
 * xf, noise_amp and seed are those of dstd_gcn_augment.h.  Conventions as there
 * (error codes in dstd_gcn.h): device pointers to contiguous fp32 / int / long
 * long, enqueue on `stream`, one launch, no workspace, no allocation and no
 * state inside the library; no LDS and no atomics; every element offset is
 * 64-bit.  The dstd_seq_store itself is host memory, read before the call
 * returns.
 *
 * Room.  room is NULL or device int32 [N]: window n may read the stored rows
 * starts[n] .. starts[n] + room[n].  NULL means T - 1 for every window: the
 * window has only its own frames.  A window with room[n] < T - 1 does not hold
 * its own frames: its batch rows are left unwritten (with or without rate).
 *
 * Rate.  rate is NULL or device fp32 [B]: the playback speed of batch row b.
 * Position of window frame f (0 <= f < T) of batch row b, with w the window
 * after the mirror fold and st = starts[w]:
 *
 *   R = min(room[w], F - 1 - st, 1 << 20)
 *   p = rate[b] * (float)f                      one fp32 rounding
 *   if !(p > 0)            i = 0, a = 0         (covers 0, negatives and NaN)
 *   else if p >= (float)R  i = R, a = 0         (past the room: the last frame in room)
 *   else                   i = (int)p, a = p - (float)i    (truncation; the subtraction is exact)
 *
 * Value of a source column, with x_i read from frames[st + i] (or
 * used[st + i]) through the mirror where the window is mirrored -- joint
 * mirror_src[j], coordinate 0 negated, exactly as in dstd_gcn_data.h:
 *
 *   a == 0 :  x_i                       copied; row i + 1 is not read; -0.0 stays -0.0
 *   else   :  x_i + a * (x_{i+1} - x_i)   difference, product and sum each rounded
 *                                       to fp32 on its own, no fused multiply-add
 *
 * The warped window replaces the plain one everywhere dstd_batch_gather_aug
 * uses it:
 *
 *   all_seqs[b][f]     = warped frame f
 *   targets[b][f][k]   = its used column k (column dim_used[k], or `used`)
 *   inputs[b][s]       = warped frame frame_in[s]
 *   inputs_inv[b][s]   = warped frame frame_inv[s]
 *
 * Order of operations: mirror, then interpolate, then transform.  With xf the
 * affine map of dstd_gcn_augment.h is applied to the interpolated (x, y, z) of
 * the joint.  Noise is keyed as there by (index value, window frame f, k), f =
 * frame_in[s] for inputs and frame_inv[s] for inputs_inv, and not by the
 * source rows the frame was blended from: padded rows stay copies, and a
 * frame seen by both input tensors carries the same noise in both.
 *
 * Identities.  rate == NULL: i = f and a = 0 with no arithmetic on any value;
 * with room NULL or room[w] >= T - 1 the results are those of
 * dstd_batch_gather_aug bit for bit.  rate[b] == 1.0f: p = f exactly, a == 0
 * at every frame, and row b equals the unwarped row bit for bit.
 */
#ifndef DSTD_GCN_WARP_H
#define DSTD_GCN_WARP_H

#include "../dstd_gcn_data.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DSTD_EINVAL, no launch, nothing written and no error left pending, for
 * everything dstd_batch_gather_aug refuses and nothing more: a NULL store,
 * frames, starts, index, dim_used, frame_in or frame_inv; B <= 0, T < 1,
 * F < 1, N < 1, D % 3 != 0, Du < 1 or Du > D; all four outputs NULL; used and
 * mirror_src both set; xf together with used; noise_amp negative, infinite or
 * NaN.  rate together with used is allowed: interpolation of standardised
 * coordinates is still linear. */
int dstd_batch_gather_warp(const dstd_seq_store* s, const int* room, const long long* index, int B,
                           const float* rate, const float* xf, float noise_amp, unsigned long long seed,
                           float* inputs, float* inputs_inv, float* targets, float* all_seqs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_WARP_H */
