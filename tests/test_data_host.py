"""Host-side checks of the device-resident dataset (include/dstd_gcn_data.h,
dstd_data.py): exports, argument checks before any GPU work, the numpy
restatement of the gather (tests/data_helper.py) pinned bit for bit to what the
reference's dataset classes built (tests/golden/dataset_batches.npz), joint
weights, the frame-level store of from_sequences and the loader's index
bookkeeping.  No GPU needed: sets are built with device="cpu", which holds the
tables but gathers nothing."""
import ctypes

import numpy as np
import pytest
import torch

import data_helper as H
import dstd_native as native
from dstd_data import DeviceLoader, DeviceSequences, MeanStd, frame_maps, mirror_source
from test_capi_host import header_symbols

EINVAL = -1


def test_library_exports_every_data_header_symbol():
    L = native.lib()
    syms = header_symbols("dstd_gcn_data.h")
    assert syms == ["dstd_batch_gather"], syms
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(native.DATA_EXPORTS)


def test_struct_layout_matches_the_header():
    """The ctypes struct against the C one: 3 pointers, 2 long long, 3 int
    (+ padding to 8), 4 pointers on LP64."""
    assert ctypes.sizeof(native.SeqStore) == 3 * 8 + 2 * 8 + 4 * 4 + 4 * 8
    assert native.SeqStore.T.offset == 40 and native.SeqStore.dim_used.offset == 56
    assert [f for f, _ in native.SeqStore._fields_] == ["frames", "used", "starts", "F", "N", "T", "D", "Du",
                                                        "dim_used", "frame_in", "frame_inv", "mirror_src"]


# ---- refusals ---------------------------------------------------------------------
def _store(**kw):
    """A well-formed H36M store; the pointers are never dereferenced on the host."""
    f = dict(frames=0x1000, used=None, starts=0x2000, F=1000, N=900, T=35, D=96, Du=66, dim_used=0x3000,
             frame_in=0x4000, frame_inv=0x5000, mirror_src=None)
    f.update(kw)
    return native.SeqStore(**f)


def _gather(store, index=0x6000, B=4, outs=(0x7000, 0x8000, 0x9000, 0xA000)):
    ref = ctypes.byref(store) if store is not None else None
    return native.lib().dstd_batch_gather(ref, index, B, *outs, None)


BAD_STORES = {
    "null frames": dict(frames=None), "null starts": dict(starts=None), "null dim_used": dict(dim_used=None),
    "null frame_in": dict(frame_in=None), "null frame_inv": dict(frame_inv=None), "T = 0": dict(T=0),
    "T < 0": dict(T=-1), "D % 3 = 1": dict(D=97), "D % 3 = 2": dict(D=98), "Du = 0": dict(Du=0),
    "Du < 0": dict(Du=-3), "Du > D": dict(Du=97), "D = 0": dict(D=0), "F = 0": dict(F=0), "N = 0": dict(N=0),
    "used with mirror_src": dict(used=0xB000, mirror_src=0xC000),
}


@pytest.mark.parametrize("what", list(BAD_STORES))
def test_bad_store_is_einval_before_any_gpu_work(what):
    assert _gather(_store(**BAD_STORES[what])) == EINVAL


def test_bad_call_arguments_are_einval_before_any_gpu_work():
    ok = _store()
    assert _gather(None) == EINVAL
    assert _gather(ok, index=None) == EINVAL
    for B in (0, -1):
        assert _gather(ok, B=B) == EINVAL
    assert _gather(ok, outs=(None, None, None, None)) == EINVAL


def test_python_layer_refuses_malformed_sets_and_has_no_cpu_gather():
    x = np.random.default_rng(0).normal(size=(3, 4, 6))
    with pytest.raises(ValueError):
        DeviceSequences.from_windows(x, [0, 2, 1], 2, 2, device="cpu")  # not increasing
    with pytest.raises(ValueError):
        DeviceSequences.from_windows(x, [0, 1, 6], 2, 2, device="cpu")  # column outside D
    with pytest.raises(ValueError):
        DeviceSequences.from_windows(x, [0, 1, 2], 2, 3, device="cpu")  # input_n + output_n != T
    with pytest.raises(ValueError):
        DeviceSequences.from_windows(x[:, :, :5], [0, 1, 2], 2, 2, device="cpu")  # D % 3
    with pytest.raises(ValueError):
        DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [2]))  # joint outside
    with pytest.raises(ValueError):
        DeviceSequences.from_sequences([x[0]], 5, [0, 1, 2], 2, 3, device="cpu")  # shorter than a window
    s = DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.gather(torch.arange(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(DeviceLoader(s, 2)))


# ---- the restatement against the reference ----------------------------------------------
def test_fixture_holds_the_cases_the_kernel_is_built_for():
    shapes = {c: H.fixture(c)["all_seqs"].shape for c in H.CASES}
    assert shapes == {"h36m_pad": (4, 35, 96), "h36m_nopad_mirror": (8, 35, 96), "h36m_pad_mirror_scale": (8, 35, 96),
                      "cmu_pad_scale": (4, 35, 114), "cmu_nopad": (4, 35, 114), "pw3d_pad_mirror": (8, 40, 72),
                      "pw3d_nopad": (4, 40, 72)}
    assert {c: len(H.fixture(c)["dim_used"]) for c in ("h36m_pad", "cmu_nopad", "pw3d_nopad")} == {
        "h36m_pad": 66, "cmu_nopad": 75, "pw3d_nopad": 69}
    for c in H.CASES:
        f = H.fixture(c)
        assert f["all_seqs"].dtype == np.float64 and f["output_seqs"].dtype == np.float32
        assert f["joint_weight_use"].max() > f["joint_weight_use"].min()
        if f["scale"]:
            assert f["std"].min() > 0
    # the mirrored cases hold a -0.0-free but sign-carrying first coordinate: the mirror is visible
    f = H.fixture("pw3d_pad_mirror")
    assert not np.array_equal(f["all_seqs"][:4], f["all_seqs"][4:])


@pytest.mark.parametrize("case", H.CASES)
def test_restatement_equals_the_reference_for_every_index(case):
    """expected_batch over the store DeviceSequences.from_windows builds (from
    the un-mirrored windows, the caller's joint lists and, where scaled, its own
    statistics) against the reference's four arrays, every index, int32 views."""
    c = H.fixture(case)
    seqs = H.build(case, "cpu")
    n = len(c["all_seqs"])
    assert len(seqs) == n
    assert (seqs._mirror_src is not None) == bool(c["mirror"] and not c["scale"])
    assert (seqs._used is not None) == bool(c["scale"])
    if c["scale"]:
        assert np.array_equal(seqs.scale_tsfm._mean.reshape(-1), c["mean"])
        assert np.array_equal(seqs.scale_tsfm._std.reshape(-1), c["std"])
    store = H.store_of(seqs)
    order = np.concatenate([np.arange(n), np.arange(n)[::-1], [0, 0, n - 1]])
    got = H.expected_batch(store, order)
    ref = H.reference_batch(c, order)
    for name, g, r in zip(H.NAMES, got, ref):
        assert g.shape == r.shape and g.dtype == np.float32, name
        assert np.array_equal(H.bits(g), H.bits(r)), (case, name)
    # one index at a time gives the same rows, and an index outside the set none
    one = H.expected_batch(store, [n - 1])
    assert all(np.array_equal(H.bits(a[0]), H.bits(r[n - 1])) for a, r in zip(one, ref))
    out = H.expected_batch(store, [-1, n, 2 * n, 0])
    assert all(np.isnan(a[:3]).all() and np.array_equal(H.bits(a[3]), H.bits(r[0])) for a, r in zip(out, ref))


def test_restatement_tells_minus_zero_from_zero():
    frames = np.zeros((2, 3))
    s = H.store_arrays(frames, [0], 2, [0, 1, 2], [0, 0], [1, 1], mirror_src=[0])
    plain, mirrored = H.expected_batch(s, [0])[3], H.expected_batch(s, [1])[3]
    assert np.array_equal(plain, mirrored) and not np.array_equal(H.bits(plain), H.bits(mirrored))
    assert H.bits(mirrored)[0, 0, 0] == np.int32(-2 ** 31) and H.bits(mirrored)[0, 0, 1] == 0


def test_from_dataset_takes_the_reference_object_as_it_is():
    c = H.fixture("h36m_pad_mirror_scale")

    class _DS:
        all_seqs, dim_used = c["all_seqs"], c["dim_used"]
        scale_tsfm = MeanStd(c["mean"], c["std"])
        joint_weight_use, joint_weight_all = c["joint_weight_use"], c["joint_weight_all"]

    seqs = DeviceSequences.from_dataset(_DS, 10, 25, padding=True, device="cpu")
    assert len(seqs) == 8 and seqs.scale_tsfm is _DS.scale_tsfm and seqs.time_tsfm is None
    assert seqs.joint_weight_use is c["joint_weight_use"]
    got = H.expected_batch(H.store_of(seqs), np.arange(8))
    for g, r in zip(got, H.reference_batch(c, np.arange(8))):
        assert np.array_equal(H.bits(g), H.bits(r))


def test_frame_maps_and_mirror_source():
    fwd, inv = frame_maps(3, 2, True)
    assert fwd.tolist() == [0, 1, 2, 2, 2] and inv.tolist() == [4, 3, 2, 2, 2]
    fwd, inv = frame_maps(3, 2, False)
    assert fwd.tolist() == [0, 1, 2, 3, 4] and inv.tolist() == [4, 3, 2, 1, 0]
    assert frame_maps(1, 1, True)[1].tolist() == [1, 1]
    assert mirror_source(5, [1, 2], [3, 4]).tolist() == [0, 3, 4, 1, 2]
    for case in ("h36m_nopad_mirror", "pw3d_pad_mirror"):
        left, right, src = H.mirror_lists(H.fixture(case))
        assert np.array_equal(mirror_source(len(src), left, right), src)


def test_mean_std_follows_the_reference_interface():
    m = MeanStd([1.0, 2.0], [2.0, 4.0])
    x = np.array([[[3.0, 10.0]]])
    assert m.transform(x).tolist() == [[[1.0, 2.0]]] and m.inverse(m.transform(x)).tolist() == x.tolist()
    t = torch.tensor(x, dtype=torch.float32)
    assert m.transform(t).dtype == torch.float32 and m.inverse(m.transform(t)).tolist() == x.tolist()


# ---- joint weights ----------------------------------------------------------------------
@pytest.mark.parametrize("case", H.CASES)
def test_from_windows_weights_equal_the_fixtures_exactly(case):
    c, seqs = H.fixture(case), H.build(case, "cpu")
    assert np.array_equal(seqs.joint_weight_use, c["joint_weight_use"])
    assert np.array_equal(seqs.joint_weight_all, c["joint_weight_all"])
    assert np.array_equal(seqs.dim_used, c["dim_used"])
    assert seqs.time_tsfm is None and (seqs.scale_tsfm is not None) == bool(c["scale"])


def _two_sequences():
    rng = np.random.default_rng(7)
    return [np.cumsum(rng.normal(size=(f, 12)), 0) * rng.uniform(0.5, 3, 12) for f in (50, 41)]


@pytest.mark.parametrize("mirror", [None, ([1], [3])])
def test_from_sequences_is_the_window_set_without_the_copies(mirror):
    """Sequences of 50 and 41 frames at T = 35: 16 + 7 windows over 91 stored
    frames; the same batches, and within 1e-12 the same weights (a mean of a
    few thousand float64 terms in another order), as the materialised windows.
    The bound is relative to the weights' scale, max(joint_weight_all) = 1: the
    mirrored set moves joints 1 and 3 alike, so both are the minimum, 0 up to
    that rounding, and no bound relative to themselves could hold."""
    T, du = 35, [3, 4, 5, 9, 10, 11]
    seqs = _two_sequences()
    windows = np.concatenate([np.stack([s[i:i + T] for i in range(len(s) - T + 1)]) for s in seqs])
    assert windows.shape == (16 + 7, T, 12)
    a = DeviceSequences.from_sequences(seqs, T, du, 10, 25, device="cpu", mirror=mirror)
    b = DeviceSequences.from_windows(windows, du, 10, 25, device="cpu", mirror=mirror)
    n = 23 * (2 if mirror else 1)
    assert len(a) == len(b) == n
    assert a.n_frames == 91 and b.n_frames == 23 * T and a.nbytes < b.nbytes / 5
    assert a.starts.tolist() == list(range(16)) + list(range(50, 57))
    idx = np.arange(n)
    for x, y in zip(H.expected_batch(H.store_of(a), idx), H.expected_batch(H.store_of(b), idx)):
        assert np.array_equal(H.bits(x), H.bits(y))
    for k in ("joint_weight_all", "joint_weight_use"):
        wa, wb = getattr(a, k), getattr(b, k)
        assert wa.shape == wb.shape == ((4,) if k == "joint_weight_all" else (2,))
        assert np.abs(wa - wb).max() <= 1e-12 * b.joint_weight_all.max(), k
    assert b.joint_weight_all.max() == 1.0 and b.joint_weight_all.min() == 0.0


def test_from_sequences_with_a_scaler_stores_the_mirrored_frames():
    T, du = 35, [3, 4, 5, 9, 10, 11]
    seqs = _two_sequences()
    windows = np.concatenate([np.stack([s[i:i + T] for i in range(len(s) - T + 1)]) for s in seqs])
    scaler = (np.arange(6) * 0.5, np.arange(1, 7) * 0.25)
    a = DeviceSequences.from_sequences(seqs, T, du, 10, 25, device="cpu", mirror=([1], [3]), scaler=scaler)
    b = DeviceSequences.from_windows(windows, du, 10, 25, device="cpu", mirror=([1], [3]), scaler=scaler)
    assert len(a) == len(b) == 46 and a._mirror_src is None and a.n_frames == 182
    idx = np.arange(46)
    for x, y in zip(H.expected_batch(H.store_of(a), idx), H.expected_batch(H.store_of(b), idx)):
        assert np.array_equal(H.bits(x), H.bits(y))
    assert np.abs(a.joint_weight_all - b.joint_weight_all).max() <= 1e-12


# ---- loader bookkeeping (index generation only) ---------------------------------------------
def _set(n):
    x = np.random.default_rng(1).normal(size=(n, 4, 6))
    return DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu")


def test_loader_len_drop_last_and_ragged_batch():
    s = _set(10)
    for bs, drop, want in ((3, False, [3, 3, 3, 1]), (3, True, [3, 3, 3]), (5, False, [5, 5]), (5, True, [5, 5]),
                           (16, False, [10]), (16, True, [])):
        ld = DeviceLoader(s, bs, drop_last=drop)
        got = list(ld.index_batches())
        assert len(ld) == len(want) == len(got), (bs, drop)
        assert [len(i) for i in got] == want
        assert all(i.dtype == torch.int64 and i.is_contiguous() for i in got)
        if got:
            assert torch.cat(got).tolist() == list(range(sum(want)))
    with pytest.raises(ValueError):
        DeviceLoader(s, 0)


def test_loader_counts_the_mirrored_half():
    x = np.random.default_rng(1).normal(size=(5, 4, 6))
    s = DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]))
    assert len(s) == 10 and torch.cat(list(DeviceLoader(s, 4).index_batches())).tolist() == list(range(10))


def test_loader_shuffle_is_seeded_per_epoch_and_a_permutation():
    s = _set(37)
    a, b, c = (DeviceLoader(s, 8, shuffle=True, seed=k) for k in (5, 5, 6))
    ea = [torch.cat(list(a.index_batches())).tolist() for _ in range(3)]
    eb = [torch.cat(list(b.index_batches())).tolist() for _ in range(3)]
    ec = [torch.cat(list(c.index_batches())).tolist() for _ in range(2)]
    assert ea == eb  # the same seed, the same order, epoch by epoch
    assert all(sorted(e) == list(range(37)) for e in ea + ec)  # each epoch a permutation
    assert ea[0] != ea[1] and ea[1] != ea[2] and ea[0] != list(range(37))
    assert ec[0] == ea[1] and ec[1] == ea[2]  # seed + epoch
    assert a.epoch == 3 and [len(i) for i in a.index_batches()] == [8, 8, 8, 8, 5]
