"""Helpers of tests/test_data_host.py and tests/test_gpu_data.py: the fixture
cases of tests/golden/dataset_batches.npz (written by make_data_golden.py from
the reference's dataset classes) and a numpy restatement of the semantics of
include/dstd_gcn_data.h, which the host test pins to that fixture bit for bit
and the GPU tests then use where the fixture holds no answer."""
import numpy as np

from conftest import group, load_npz

CASES = ("h36m_pad", "h36m_nopad_mirror", "h36m_pad_mirror_scale", "cmu_pad_scale", "cmu_nopad", "pw3d_pad_mirror",
         "pw3d_nopad")
NAMES = ("inputs", "inputs_inv", "targets", "all_seqs")
FIXTURE_KEYS = ("input_seqs", "input_seqs_inv", "output_seqs", "all_seqs")

_fixture = {}


def fixture(case):
    """One case of dataset_batches.npz as a dict (loaded once, not to be changed)."""
    if case not in _fixture:
        _fixture[case] = group(load_npz("dataset_batches.npz"), case + "/")
    return _fixture[case]


def reference_batch(c, idx):
    """The reference's four arrays at ``idx``, cast to fp32 as the engine does."""
    return tuple(np.ascontiguousarray(c[k][idx]).astype(np.float32) for k in FIXTURE_KEYS)


def mirror_lists(c):
    """(left, right) joint lists and the joint map of the recorded mirror."""
    src_dim, sign = c["mirror_src_dim"], c["mirror_sign"]
    d = len(src_dim)
    src = src_dim[0::3] // 3
    assert np.array_equal(src_dim, np.repeat(src, 3) * 3 + np.tile(np.arange(3), d // 3))  # whole joints move
    assert np.array_equal(sign, np.tile([-1, 1, 1], d // 3))  # coordinate 0 negated
    assert np.array_equal(src[src], np.arange(d // 3))  # an exchange of pairs
    left = [j for j in range(d // 3) if src[j] > j]
    return left, [int(src[j]) for j in left], src.astype(np.int32)


def bits(a):
    """int32 view of an fp32 array (or tensor): equality that tells -0.0 from 0.0."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.int32)


def store_arrays(frames, starts, T, dim_used, frame_in, frame_inv, mirror_src=None, used=None):
    """The host image of a dstd_seq_store: fp32 frames [F][D] (and used [F][Du])."""
    return dict(frames=np.asarray(frames, dtype=np.float32), starts=np.asarray(starts, dtype=np.int64), T=int(T),
                dim_used=np.asarray(dim_used, dtype=np.int64), frame_in=np.asarray(frame_in, dtype=np.int64),
                frame_inv=np.asarray(frame_inv, dtype=np.int64),
                mirror_src=None if mirror_src is None else np.asarray(mirror_src, dtype=np.int64),
                used=None if used is None else np.asarray(used, dtype=np.float32))


def store_of(seqs):
    """store_arrays of a dstd_data.DeviceSequences (reads its device tensors back)."""
    def host(t):
        return None if t is None else t.cpu().numpy()
    return store_arrays(host(seqs._frames), host(seqs._starts), seqs.seq_len, seqs.dim_used, host(seqs._frame_in),
                        host(seqs._frame_inv), host(seqs._mirror_src), host(seqs._used))


def expected_batch(s, index, fill=np.nan):
    """include/dstd_gcn_data.h restated: (inputs, inputs_inv, targets, all_seqs)
    of ``index`` over the store ``s``; rows of an index outside the set keep
    ``fill``."""
    frames, T, du = s["frames"], s["T"], s["dim_used"]
    N, D, B = len(s["starts"]), frames.shape[1], len(index)
    all_seqs = np.full((B, T, D), fill, dtype=np.float32)
    targets = np.full((B, T, len(du)), fill, dtype=np.float32)
    inputs, inputs_inv = targets.copy(), targets.copy()
    for b, w in enumerate(np.asarray(index, dtype=np.int64)):
        mirrored = s["mirror_src"] is not None and N <= w < 2 * N
        if mirrored:
            w -= N
        if not 0 <= w < N:
            continue
        f = s["starts"][w] + np.arange(T)
        rows = frames[f]
        if mirrored:
            rows = rows.reshape(T, D // 3, 3)[:, s["mirror_src"]].copy()
            rows[:, :, 0] = -rows[:, :, 0]
            rows = rows.reshape(T, D)
        all_seqs[b] = rows
        targets[b] = rows[:, du] if s["used"] is None else s["used"][f]
        inputs[b] = targets[b][s["frame_in"]]
        inputs_inv[b] = targets[b][s["frame_inv"]]
    return inputs, inputs_inv, targets, all_seqs


def build(case, device, **kw):
    """DeviceSequences.from_windows of a fixture case, as a user holding the
    un-mirrored windows and the skeleton's joint lists would build it."""
    from dstd_data import DeviceSequences
    c = fixture(case)
    n = len(c["all_seqs"]) // (2 if c["mirror"] else 1)
    mirror = mirror_lists(c)[:2] if c["mirror"] else None
    return DeviceSequences.from_windows(c["all_seqs"][:n], c["dim_used"], int(c["input_n"]), int(c["output_n"]),
                                        padding=bool(c["padding"]), device=device, mirror=mirror,
                                        scaler=True if c["scale"] else None, **kw)


def hip_last_error():
    """hipGetLastError of the HIP runtime this process has loaded (the one
    torch and the native library share)."""
    import ctypes
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert len(paths) == 1, paths
    return int(ctypes.CDLL(paths[0]).hipGetLastError())
