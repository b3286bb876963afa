"""Helpers of tests/test_eval_host.py and tests/test_gpu_eval.py: the metric of
include/ext/dstd_gcn_eval.h restated in numpy fp64 over the host image of a
store (tests/data_helper.py store_arrays / expected_batch, which
tests/test_data_host.py pins to the reference's arrays bit for bit)."""
import numpy as np

import data_helper as H


def metric_tables(D, dim_used, ignore=(), equal=()):
    """(used_pos [D], joint_src [J]) as PredictionEngine._metric_indices builds them."""
    used_pos = np.full(D, -1, dtype=np.int32)
    used_pos[np.asarray(dim_used, dtype=np.int64)] = np.arange(len(dim_used), dtype=np.int32)
    joint_src = np.arange(D // 3, dtype=np.int32)
    joint_src[np.asarray(ignore, dtype=np.int64)] = np.asarray(equal, dtype=np.int32)
    return used_pos, joint_src


def row_groups(store, index, group, n_groups):
    """Group of every batch row, -1 for a skipped one (index outside the
    store, group outside [0, n_groups))."""
    N = len(store["starts"])
    n_index = 2 * N if store["mirror_src"] is not None else N
    out = np.full(len(index), -1, dtype=np.int64)
    for b, w in enumerate(np.asarray(index, dtype=np.int64)):
        if 0 <= w < n_index:
            g = 0 if group is None else int(group[w])
            if 0 <= g < n_groups:
                out[b] = g
    return out


def frame_norms(store, index, outputs, t_out0, used_pos, joint_src, frames):
    """[B][K] fp64: (1/J) * sum over joints of ||targ - pred|| at frames[k] of
    every batch row; NaN rows for indices outside the store."""
    all_seqs = H.expected_batch(store, index)[3].astype(np.float64)
    B, T, D = all_seqs.shape
    J = D // 3
    outs = np.asarray(outputs, dtype=np.float64)
    dims = np.nonzero(used_pos >= 0)[0]
    res = np.zeros((B, len(frames)))
    for k, f in enumerate(frames):
        pred = all_seqs[:, f].copy()
        if f >= t_out0:
            pred[:, dims] = outs[:, f - t_out0][:, used_pos[dims]]
        pj = pred.reshape(B, J, 3)[:, joint_src]
        res[:, k] = np.linalg.norm(all_seqs[:, f].reshape(B, J, 3) - pj, axis=-1).sum(-1) / J
    return res


def group_mpjpe_reference(store, index, outputs, t_out0, used_pos, joint_src, frames, group, n_groups):
    """(sums [G][K] fp64, counts [G]) of one dstd_store_group_mpjpe call on zeroed outputs."""
    rows = row_groups(store, index, group, n_groups)
    norms = frame_norms(store, index, outputs, t_out0, used_pos, joint_src, frames)
    sums, counts = np.zeros((n_groups, len(frames))), np.zeros(n_groups, dtype=np.int64)
    for g in range(n_groups):
        sums[g] = norms[rows == g].sum(0)
        counts[g] = int((rows == g).sum())
    return sums, counts
