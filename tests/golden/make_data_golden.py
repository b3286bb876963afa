#!/usr/bin/env python
"""Generate tests/golden/dataset_batches.npz by running the REFERENCE datasets.

Runs only where a reference checkout is at hand (like make_golden.py): it
imports the reference's ``dataset.h36m.Human36M``, ``dataset.cmu.CMUMocap`` and
``dataset.pw3d.PW3D`` and lets each class build its four arrays -- window
selection, padding, mirror, scale, joint weights -- on the CPU from synthetic
float64 input:

* H36M / CMU: ``dataset.utils.load_data_3d`` / ``load_data_cmu_3d`` (file
  reading and forward kinematics) are replaced by functions returning synthetic
  windows and a synthetic choice of used joints; everything after that call is
  the class's own code.
* 3DPW: two tiny synthetic pickles in a temporary directory.

Recorded per case ``<case>/``: ``all_seqs`` (float64, the class's, mirrored
half included), ``input_seqs`` / ``input_seqs_inv`` / ``output_seqs`` (cast to
float32, what the engine's per-batch ``.float()`` makes of them), ``dim_used``,
``joint_weight_use`` / ``joint_weight_all`` (float64), ``input_n`` /
``output_n`` / ``padding`` / ``mirror`` / ``scale`` and, when scaled, the
scaler's ``mean`` / ``std``.  The mirror map is recorded as data: the class's
``get_mirror`` runs on an array whose entries are their own dimension index
plus one, which gives ``mirror_src_dim`` (source dimension) and
``mirror_sign`` per dimension.

Inputs are multiples of 1/8 (1/1024 m before the classes' own x1000 for 3DPW)
so that the archive compresses; every used dimension has non-zero std and the
joint weights have max > min (asserted).  Nothing is pickled into the archive.

Usage:  python tests/golden/make_data_golden.py <reference checkout>
"""
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N = 4  # windows per case before the mirror doubles them

sys.dont_write_bytecode = True


def synthetic_windows(rng, n, t, d):
    """A random walk per window, quantised to 1/8."""
    x = rng.normal(0, 300, (n, 1, d)) + np.cumsum(rng.normal(0, 12, (n, t, d)) * rng.uniform(0.2, 2, (1, 1, d)), 1)
    return np.round(x * 8) / 8


def used_dims(rng, joints, keep):
    used = np.sort(rng.choice(joints, keep, replace=False))
    dims = np.sort(np.concatenate((used * 3, used * 3 + 1, used * 3 + 2)))
    return np.setdiff1d(np.arange(joints * 3), dims), dims


def record(out, case, ds, input_n, output_n, padding, mirror, scale):
    assert ds.time_tsfm is None
    out[f"{case}/all_seqs"] = np.asarray(ds.all_seqs, dtype=np.float64)
    for k in ("input_seqs", "input_seqs_inv", "output_seqs"):
        a = np.asarray(getattr(ds, k))
        assert a.dtype == np.float64
        out[f"{case}/{k}"] = a.astype(np.float32)
    out[f"{case}/dim_used"] = np.asarray(ds.dim_used, dtype=np.int64)
    out[f"{case}/joint_weight_use"] = np.asarray(ds.joint_weight_use, dtype=np.float64)
    out[f"{case}/joint_weight_all"] = np.asarray(ds.joint_weight_all, dtype=np.float64)
    assert ds.joint_weight_all.max() > ds.joint_weight_all.min() and np.isfinite(ds.joint_weight_all).all()
    for k, v in (("input_n", input_n), ("output_n", output_n), ("padding", int(padding)), ("mirror", int(mirror)),
                 ("scale", int(scale))):
        out[f"{case}/{k}"] = np.int64(v)
    if scale:
        out[f"{case}/mean"] = np.asarray(ds.scale_tsfm._mean, dtype=np.float64).reshape(-1)
        out[f"{case}/std"] = np.asarray(ds.scale_tsfm._std, dtype=np.float64).reshape(-1)
        assert out[f"{case}/std"].min() > 0
    else:
        assert ds.scale_tsfm is None
    d = ds.all_seqs.shape[2]
    probe = ds.get_mirror(np.broadcast_to(np.arange(1, d + 1, dtype=np.float64), (1, 1, d)).copy())[0, 0]
    out[f"{case}/mirror_src_dim"] = (np.abs(probe) - 1).astype(np.int64)
    out[f"{case}/mirror_sign"] = np.sign(probe).astype(np.int64)


def main(ref):
    sys.path.insert(0, ref)
    from dataset import utils  # noqa: E402  (reference)
    from dataset.cmu import CMUMocap  # noqa: E402  (reference)
    from dataset.h36m import Human36M  # noqa: E402  (reference)
    from dataset.pw3d import PW3D  # noqa: E402  (reference)

    rng = np.random.default_rng(20260)
    out = {}

    h_win, h_dims = synthetic_windows(rng, N, 35, 96), used_dims(rng, 32, 22)
    utils.load_data_3d = lambda *a, **k: (h_win.copy(), h_dims[0], h_dims[1])
    for case, padding, mirror, scale in (("h36m_pad", True, False, False), ("h36m_nopad_mirror", False, True, False),
                                         ("h36m_pad_mirror_scale", True, True, True)):
        ds = Human36M(None, input_n=10, output_n=25, dct_used=0, mode="train", scale=scale, mirror=mirror,
                      padding=padding)
        record(out, case, ds, 10, 25, padding, mirror, scale)

    c_win, c_dims = synthetic_windows(rng, N, 35, 114), used_dims(rng, 38, 25)
    utils.load_data_cmu_3d = lambda *a, **k: (c_win.copy(), c_dims[0], c_dims[1])
    for case, padding, scale in (("cmu_pad_scale", True, True), ("cmu_nopad", False, False)):
        ds = CMUMocap(None, input_n=10, output_n=25, dct_used=0, scale=scale, padding=padding)
        record(out, case, ds, 10, 25, padding, False, scale)

    with tempfile.TemporaryDirectory() as tmp:
        for name in ("a.pkl", "b.pkl"):  # 41 frames at T = 40: two windows each
            pos = np.round(synthetic_windows(rng, 1, 41, 72)[0] / 1000 * 1024) / 1024
            with open(os.path.join(tmp, name), "wb") as f:
                pickle.dump({"jointPositions": [pos]}, f)
        for case, padding, mirror in (("pw3d_pad_mirror", True, True), ("pw3d_nopad", False, False)):
            ds = PW3D(tmp + os.sep, input_n=10, output_n=30, dct_used=0, mirror=mirror, padding=padding)
            record(out, case, ds, 10, 30, padding, mirror, False)

    for case in sorted({k.split("/")[0] for k in out}):
        a = out[f"{case}/all_seqs"]
        assert a.shape[0] == N * (2 if out[f"{case}/mirror"] else 1), (case, a.shape)
        assert a[:, :, out[f"{case}/dim_used"]].reshape(-1, len(out[f"{case}/dim_used"])).std(0).min() > 0
    path = os.path.join(HERE, "dataset_batches.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
