/*
 * dstd_gcn_data.h -- C ABI of the device-resident dataset: every batch the
 * engine consumes, assembled from frames kept in device memory by one launch.
 *
 * The reference's datasets (dataset/h36m.py:53-64, 100-116; cmu.py and pw3d.py
 * alike) hold four host arrays that are all selections of one: with
 * a = all_seqs [N][T][D] and u = a[:, :, dim_used],
 *
 *   input_seqs     = u[:, i_idx]       i_idx     = 0..input_n-1, then input_n-1 repeated
 *   input_seqs_inv = u[:, i_idx_inv]   i_idx_inv = T-1..output_n, then output_n repeated
 *   output_seqs    = u                 (without padding: i_idx = 0..T-1, i_idx_inv its reverse)
 *
 * and get_mirror appends, per window, a copy with left and right joints
 * exchanged and coordinate 0 negated.  Its windows overlap T-fold, so here the
 * distinct frames are stored once and a window is a start row:
 *
 *   window n        = frames[starts[n] .. starts[n] + T)
 *   index w < N     : window w
 *   N <= w < 2N     : window w - N mirrored (only with mirror_src): joint j reads
 *                     joint mirror_src[j], coordinate 0 negated
 *   any other w     : row b of every output is left unwritten, nothing is read
 *
 * With f = starts[w] + t:
 *
 *   all_seqs[b][t][:]   = frames[f][:]                      (mirrored if applicable)
 *   targets[b][t][k]    = all_seqs[b][t][dim_used[k]]       or used[f][k] when `used` is given
 *   inputs[b][s][:]     = targets[b][frame_in[s]][:]
 *   inputs_inv[b][s][:] = targets[b][frame_inv[s]][:]
 *
 * `used` holds the model-side values of the used columns where they are not
 * the raw ones (the datasets' scale transform, applied once in fp64 before the
 * cast to fp32); it excludes mirror_src: a scaled, mirrored set stores its
 * mirrored frames.
 *
 * Conventions as in dstd_gcn.h (error codes there): device pointers to
 * contiguous fp32 / int / long long, enqueue on `stream`, one launch, no
 * workspace, no allocation and no state inside the library.  The
 * dstd_seq_store itself is host memory, read before the call returns.  Every
 * element offset is 64-bit (F * D exceeds 2^31 for real sets).  A start, a
 * frame map entry, a column or a mirror source outside its range writes
 * nothing and reads nothing out of bounds.
 */
#ifndef DSTD_GCN_DATA_H
#define DSTD_GCN_DATA_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dstd_seq_store {
  const float* frames;      /* [F][D] fp32: all frames of all sequences, back to back            */
  const float* used;        /* NULL, or [F][Du]: model-side values of the used dims (see above)   */
  const long long* starts;  /* device [N]: window n = frames[starts[n] .. starts[n] + T)          */
  long long F, N;
  int T, D, Du;
  const int* dim_used;      /* device [Du]: columns of D, strictly increasing                     */
  const int* frame_in;      /* device [T]: inputs[s]     = window frame frame_in[s]   (i_idx)     */
  const int* frame_inv;     /* device [T]: inputs_inv[s] = window frame frame_inv[s]  (i_idx_inv) */
  const int* mirror_src;    /* NULL, or device [D/3]: joint j of a mirrored window reads joint
                               mirror_src[j], coordinate 0 negated (get_mirror of the datasets)  */
} dstd_seq_store;

/* index: device [B].  inputs, inputs_inv, targets: [B][T][Du] or NULL;
 * all_seqs: [B][T][D] or NULL; a NULL output is not written.  DSTD_EINVAL,
 * and no launch, for: a NULL store, frames, starts, index, dim_used, frame_in
 * or frame_inv; B <= 0, T < 1, F < 1, N < 1, D % 3 != 0, Du < 1 or Du > D; all
 * four outputs NULL; used and mirror_src both set. */
int dstd_batch_gather(const dstd_seq_store* s, const long long* index, int B, float* inputs, float* inputs_inv,
                      float* targets, float* all_seqs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSTD_GCN_DATA_H */
