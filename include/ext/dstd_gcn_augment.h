/*
 * dstd_gcn_augment.h -- C ABI of the augmenting gather: the batch that
 * dstd_batch_gather (dstd_gcn_data.h) assembles from a device-resident set,
 * with a per-sample affine transform of every joint and a counter-based jitter
 * of the observed frames applied in the same launch.
 *
 * Rotation about the vertical, scale jitter and input noise are the routine
 * augmentations of skeleton data.  The gather already touches every output
 * float once and already knows the window, the mirror and the frame maps, so
 * they cost no launch and no pass over the batch of their own.
 *
 * dstd_seq_store, index, the four outputs, NULL outputs, the mirrored half
 * N <= w < 2N and "an index, a start or a table entry outside its range writes
 * nothing and reads nothing out of bounds" are exactly as in dstd_gcn_data.h.
 * Conventions as there (error codes in dstd_gcn.h): device pointers to
 * contiguous fp32 / int / long long, enqueue on `stream`, one launch, no
 * workspace, no allocation and no state inside the library; no LDS and no
 * atomics; every element offset is 64-bit.  The dstd_seq_store itself is host
 * memory, read before the call returns.
 *
 * Affine transform.  xf is NULL or device [B][12]: row b is a row-major 3x4
 * [A | t] applied to every joint of batch row b, after the mirror.  With
 * (x, y, z) joint j of a window frame as dstd_batch_gather would emit it in
 * all_seqs,
 *
 *   q[c] = ((A[c][0]*x + A[c][1]*y) + A[c][2]*z) + t[c]
 *
 * every product and every sum rounded to fp32 on its own, in this order, no
 * fused multiply-add: the result can be restated bit for bit.
 *
 *   all_seqs[b][f][3j+c] = q[c]
 *   targets[b][f][k]     = q of joint dim_used[k] / 3, component dim_used[k] % 3
 *   inputs, inputs_inv   : frames of targets through frame_in / frame_inv, as before
 *
 * A used column reads all three source columns of its joint, whether or not
 * they are in dim_used; any strictly increasing dim_used is valid.  With
 * xf == NULL no arithmetic is done: values are copied, -0.0 stays -0.0.
 *
 * Observation noise.  noise_amp >= 0 and finite; at 0 nothing is added.  Noise
 * goes to inputs and inputs_inv only; targets and all_seqs stay clean.  For
 * element (b, s, k) of inputs, with w = index[b] (the index value: a mirrored
 * window has noise of its own) and f = frame_in[s]:
 *
 *   key = ((unsigned long long)w * T + f) * Du + k
 *   h   = mix64(seed * 0x9e3779b97f4a7c15 + key)      (the splitmix64 finaliser)
 *   u   = (float)(h >> 40) * 2^-24
 *   n   = noise_amp * (2u - 1)                         (2u - 1 is exact: one rounding)
 *   inputs[b][s][k] = clean + n                        (one rounding)
 *
 * and for inputs_inv the same with f = frame_inv[s].  mix64(z): z = (z ^ z >> 30)
 * * 0xbf58476d1ce4e5b9; z = (z ^ z >> 27) * 0x94d049bb133111eb; z ^ z >> 31, all
 * modulo 2^64.  The noise is keyed by the source frame, not by the destination
 * row: padded rows that repeat a frame stay identical copies of it, and a frame
 * seen by both inputs and inputs_inv carries the same noise in both.  Noise
 * with `used` is allowed; the amplitude is then in the scaler's units.
 */
#ifndef DSTD_GCN_AUGMENT_H
#define DSTD_GCN_AUGMENT_H

#include "../dstd_gcn_data.h"

#ifdef __cplusplus
extern "C" {
#endif

/* DSTD_EINVAL, no launch, nothing written and no error left pending, for:
 * everything dstd_batch_gather refuses (a NULL store, frames, starts, index,
 * dim_used, frame_in or frame_inv; B <= 0, T < 1, F < 1, N < 1, D % 3 != 0,
 * Du < 1 or Du > D; all four outputs NULL; used and mirror_src both set); xf
 * together with used (a rigid transform of standardised coordinates is
 * meaningless); noise_amp negative, infinite or NaN. */
int dstd_batch_gather_aug(const dstd_seq_store* s, const long long* index, int B,
                          const float* xf, float noise_amp, unsigned long long seed,
                          float* inputs, float* inputs_inv, float* targets, float* all_seqs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_AUGMENT_H */
