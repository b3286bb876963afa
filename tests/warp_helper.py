"""Helpers of tests/test_warp_host.py and tests/test_gpu_warp.py: a numpy
restatement of include/ext/dstd_gcn_warp.h, with the affine map and the noise
of tests/augment_helper.py.

Explicit fp32 steps: the position is one np.float32 product, int() truncation
and one np.float32 difference; a blended value is a difference, a product and a
sum of np.float32 arrays, each a separate ufunc that rounds its result to fp32.
The mirror comes before the blend and the transform after it."""
import numpy as np

from augment_helper import F32, affine, jitter

MAX_ROOM = 1 << 20


def position(rate, f, R):
    """(i, a) of window frame ``f`` at playback rate ``rate`` with ``R`` rows
    of room; ``rate`` None: (f, 0) with no arithmetic."""
    if rate is None:
        return int(f), F32(0)
    with np.errstate(over="ignore", invalid="ignore"):
        p = F32(rate) * F32(f)  # one rounding
    assert p.dtype == F32
    if not p > 0:  # 0, negatives and NaN
        return 0, F32(0)
    if p >= F32(R):
        return int(R), F32(0)
    i = int(p)  # truncation
    a = p - F32(i)  # exact
    assert a.dtype == F32 and 0 <= i < R and float(a) == float(p) - i
    return i, a


def _mirrored(row, mirror_src):
    m = row.reshape(-1, 3)[mirror_src].copy()
    m[:, 0] = -m[:, 0]
    return m.reshape(row.shape)


def warped_row(src, st, i, a, mirror_src=None):
    """Row ``st + i`` of ``src`` blended with row ``st + i + 1`` by ``a``,
    through the mirror first; with a == 0 a copy, and row i + 1 is not read."""
    x = src[st + i] if mirror_src is None else _mirrored(src[st + i], mirror_src)
    if a == 0:
        return x.copy()
    y = src[st + i + 1] if mirror_src is None else _mirrored(src[st + i + 1], mirror_src)
    d = y - x
    t = F32(a) * d
    out = x + t
    assert d.dtype == t.dtype == out.dtype == F32
    return out


def expected_warp(s, index, rate=None, room=None, xf=None, noise_amp=0.0, seed=0, fill=np.nan):
    """include/ext/dstd_gcn_warp.h restated: (inputs, inputs_inv, targets,
    all_seqs) of ``index`` over the store ``s`` (data_helper.store_arrays) with
    the room table ``room`` (None: T - 1), rates ``rate`` (None or [B]), ``xf``
    None or [B][12]; rows that the entry point leaves unwritten keep ``fill``."""
    frames, T, du = s["frames"], s["T"], s["dim_used"]
    N, (F, D), B = len(s["starts"]), frames.shape, len(index)
    if xf is not None:
        if s["used"] is not None:
            raise ValueError("a transform of a scaled set is refused")
        xf = np.asarray(xf, dtype=F32).reshape(B, 12)
    all_seqs = np.full((B, T, D), fill, dtype=F32)
    targets = np.full((B, T, len(du)), fill, dtype=F32)
    inputs, inputs_inv = targets.copy(), targets.copy()
    for b, w0 in enumerate(np.asarray(index, dtype=np.int64)):
        w, mirror = int(w0), None
        if s["mirror_src"] is not None and w >= N:
            w, mirror = w - N, s["mirror_src"]
        if not 0 <= w < N:
            continue
        st = int(s["starts"][w])
        if st < 0 or st > F - T:
            continue
        rw = T - 1 if room is None else int(room[w])
        if rw < T - 1:
            continue
        R = min(rw, F - 1 - st, MAX_ROOM)
        pos = [position(None if rate is None else rate[b], f, R) for f in range(T)]
        win = np.stack([warped_row(frames, st, i, a, mirror) for i, a in pos])
        if xf is not None:
            win = affine(win, xf[b])
        all_seqs[b] = win
        if s["used"] is None:
            targets[b] = win[:, du]
        else:
            targets[b] = np.stack([warped_row(s["used"], st, i, a) for i, a in pos])
        inputs[b], inputs_inv[b] = targets[b][s["frame_in"]], targets[b][s["frame_inv"]]
        if noise_amp != 0:
            inputs[b] = inputs[b] + jitter(seed, w0, T, s["frame_in"], len(du), noise_amp)
            inputs_inv[b] = inputs_inv[b] + jitter(seed, w0, T, s["frame_inv"], len(du), noise_amp)
    assert all(a.dtype == F32 for a in (inputs, inputs_inv, targets, all_seqs))
    return inputs, inputs_inv, targets, all_seqs
