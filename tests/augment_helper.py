"""Helpers of tests/test_augment_host.py and tests/test_gpu_augment.py: a numpy
restatement of include/ext/dstd_gcn_augment.h on top of data_helper.py's
restatement of the plain gather.

fp32 throughout: numpy's elementwise multiply and add are separate ufuncs, each
rounding its result to fp32, which is the header's "every product and every sum
rounded on its own"; the hash is uint64 arithmetic modulo 2^64."""
import numpy as np

from data_helper import expected_batch

GOLDEN_GAMMA = np.uint64(0x9E3779B97F4A7C15)
F32 = np.float32


def mix64(z):
    """The splitmix64 finaliser on a uint64 array."""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def jitter(seed, w, T, frames, Du, amp):
    """amp * (2u - 1) of window index value ``w`` at source frames ``frames``:
    fp32 [len(frames)][Du]."""
    with np.errstate(over="ignore"):
        f = np.asarray(frames, dtype=np.int64).astype(np.uint64)
        key = (np.uint64(w) * np.uint64(T) + f)[:, None] * np.uint64(Du) + np.arange(Du, dtype=np.uint64)[None, :]
        h = mix64(np.uint64(seed % 2 ** 64) * GOLDEN_GAMMA + key)
    u = (h >> np.uint64(40)).astype(F32) * F32(2.0 ** -24)  # 24 bits: exact
    return F32(amp) * (F32(2) * u - F32(1))  # 2u - 1 is exact


def affine(rows, m):
    """rows fp32 [..., D], m fp32 [12] row-major [A | t]: q[c] = ((A[c][0]*x +
    A[c][1]*y) + A[c][2]*z) + t[c] per joint, each operation rounded to fp32."""
    rows, m = np.asarray(rows, dtype=F32), np.asarray(m, dtype=F32).reshape(3, 4)
    p = rows.reshape(*rows.shape[:-1], -1, 3)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    q = np.stack([((m[c, 0] * x + m[c, 1] * y) + m[c, 2] * z) + m[c, 3] for c in range(3)], axis=-1)
    assert q.dtype == F32
    return q.reshape(rows.shape)


def valid_rows(s, index):
    n = len(s["starts"]) * (2 if s["mirror_src"] is not None else 1)
    index = np.asarray(index, dtype=np.int64)
    return (index >= 0) & (index < n)


def expected_aug(s, index, xf=None, noise_amp=0.0, seed=0, fill=np.nan):
    """include/ext/dstd_gcn_augment.h restated: (inputs, inputs_inv, targets,
    all_seqs) of ``index`` over the store ``s`` (data_helper.store_arrays),
    ``xf`` None or [B][12] (or [B][3][4]); rows of an index outside the set
    keep ``fill``.  With xf None and amplitude 0 this IS expected_batch."""
    inputs, inputs_inv, targets, all_seqs = expected_batch(s, index, fill)
    index = np.asarray(index, dtype=np.int64)
    ok = valid_rows(s, index)
    T, Du = s["T"], len(s["dim_used"])
    if xf is not None:
        if s["used"] is not None:
            raise ValueError("a transform of a scaled set is refused")
        xf = np.asarray(xf, dtype=F32).reshape(len(index), 12)
        all_seqs, targets = all_seqs.copy(), targets.copy()
        for b in np.nonzero(ok)[0]:
            all_seqs[b] = affine(all_seqs[b], xf[b])
            targets[b] = all_seqs[b][:, s["dim_used"]]
        inputs, inputs_inv = inputs.copy(), inputs_inv.copy()
        inputs[ok] = targets[ok][:, s["frame_in"]]
        inputs_inv[ok] = targets[ok][:, s["frame_inv"]]
    if noise_amp != 0:
        inputs, inputs_inv = inputs.copy(), inputs_inv.copy()
        for b in np.nonzero(ok)[0]:
            inputs[b] = inputs[b] + jitter(seed, index[b], T, s["frame_in"], Du, noise_amp)
            inputs_inv[b] = inputs_inv[b] + jitter(seed, index[b], T, s["frame_inv"], Du, noise_amp)
    assert all(a.dtype == F32 for a in (inputs, inputs_inv, targets, all_seqs))
    return inputs, inputs_inv, targets, all_seqs


def random_transforms(B, seed=0):
    """[B][12] general matrices (not only rotations) of moderate size; where
    the batch has room, row 1 is the identity and the last row all zeros."""
    xf = np.random.default_rng(seed).normal(size=(B, 12)).astype(F32)
    if B >= 2:
        xf[1] = np.eye(3, 4, dtype=F32).reshape(12)
    if B >= 3:
        xf[-1] = 0
    return xf
