"""MI355X checks of the device-resident dataset (include/dstd_gcn_data.h,
dstd_data.py): dstd_batch_gather against the reference's own arrays
(tests/golden/dataset_batches.npz) and, for inputs the fixture does not hold,
against tests/data_helper.py expected_batch, which tests/test_data_host.py pins
to that fixture bit for bit.

A gather copies (and, mirrored, negates) fp32 values: every comparison is
equality of int32 views, no tolerance anywhere.

Shapes: the fixture's row lengths 66 / 69 / 75 (and 96 / 114 / 72 for all_seqs)
are no multiple of the wave's 64 lanes, one row takes one to two passes; T = 2
and D = 3 are the smallest the header admits; B = 257 at T = 35 is 8995 rows,
more than one wave per CU of rows and no multiple of the 4 rows of a block.
"""
import itertools

import numpy as np
import pytest
import torch

import data_helper as H
from dstd_data import DeviceLoader, DeviceSequences
from model import get_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7FC0BEEF  # as fp32 a NaN that no gather of these sets produces
GUARD_FLOATS = 1024  # 4 KiB on either side

_sets = {}


def fixture_set(case):
    if case not in _sets:
        seqs = H.build(case, DEV)
        _sets[case] = (seqs, H.store_of(seqs))
    return _sets[case]


def synthetic_set(N, T, D, dim_used, input_n, padding=True, mirror=None, seed=0):
    x = np.random.default_rng(seed).normal(size=(N, T, D)) * 100
    seqs = DeviceSequences.from_windows(x, dim_used, input_n, T - input_n, padding=padding, device=DEV, mirror=mirror)
    return seqs, H.store_of(seqs)


def index(values):
    return torch.tensor(list(values), dtype=torch.int64, device=DEV)


def same(got, want, what):
    for name, g, w in zip(H.NAMES, got, want):
        if g is None:
            continue
        assert tuple(g.shape) == w.shape and g.dtype == torch.float32 and g.is_contiguous(), (what, name)
        bad = np.nonzero(H.bits(g).reshape(-1) != H.bits(w).reshape(-1))[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} of {w.size} elements, first flat index {bad[0]}"


def gather_and_check(seqs, store, idx, what, **kw):
    got = seqs.gather(index(idx), **kw)
    torch.cuda.synchronize()
    same(got, H.expected_batch(store, idx), what)
    return got


# ---- the fixture, through the loader ------------------------------------------------------
@pytest.mark.parametrize("case", H.CASES)
def test_loader_reproduces_the_reference_arrays(case):
    """DeviceLoader(shuffle=False, batch_size=3) over every fixture case, the
    ragged last batch included, against the reference's arrays cast to fp32."""
    c = H.fixture(case)
    seqs, _ = fixture_set(case)
    n = len(c["all_seqs"])
    loader = DeviceLoader(seqs, 3, shuffle=False)
    assert len(loader) == -(-n // 3)
    seen = 0
    for i, batch in enumerate(loader):
        idx = np.arange(3 * i, min(n, 3 * i + 3))
        assert loader.last_index.tolist() == idx.tolist()
        assert all(t.is_cuda and t.shape[0] == len(idx) for t in batch)
        same(batch, H.reference_batch(c, idx), f"{case} batch {i}")
        seen += len(idx)
    assert seen == n and i == len(loader) - 1 and n % 3 != 0


def test_shuffled_epoch_is_the_same_rows_in_the_loaders_order():
    c = H.fixture("h36m_nopad_mirror")
    seqs, _ = fixture_set("h36m_nopad_mirror")
    loader = DeviceLoader(seqs, 3, shuffle=True, seed=3)
    order = []
    for batch in loader:
        idx = loader.last_index.cpu().numpy()
        same(batch, H.reference_batch(c, idx), "shuffled")
        order += idx.tolist()
    assert sorted(order) == list(range(8)) and loader.last_index.is_cuda


# ---- smallest shapes ------------------------------------------------------------------
SMALL = {
    "T=2 D=3 Du=3 B=1": dict(N=2, T=2, D=3, dim_used=[0, 1, 2], input_n=1, idx=[1]),
    "T=3 D=6 Du=3 dim_used 3..5": dict(N=3, T=3, D=6, dim_used=[3, 4, 5], input_n=2, idx=[2, 0, 1]),
    "Du = D": dict(N=3, T=4, D=9, dim_used=list(range(9)), input_n=2, idx=[0, 1, 2, 2]),
    "Du = 1": dict(N=3, T=4, D=6, dim_used=[4], input_n=1, idx=[2, 1]),
    "Du = 1 no padding, mirrored": dict(N=3, T=5, D=9, dim_used=[3], input_n=2, idx=[5, 0, 3], padding=False,
                                        mirror=([0], [1])),
    "D > 64, scattered dim_used": dict(N=2, T=3, D=132, dim_used=list(range(1, 132, 2)), input_n=1, idx=[1, 0, 3],
                                       mirror=([0, 5], [43, 7])),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_smallest_shapes(name):
    kw = dict(SMALL[name])
    idx = kw.pop("idx")
    seqs, store = synthetic_set(**kw)
    gather_and_check(seqs, store, idx, name)


@pytest.mark.parametrize("B", [1, 3, 257])
def test_batch_sizes(B):
    seqs, store = fixture_set("h36m_nopad_mirror")
    idx = np.random.default_rng(B).integers(0, len(seqs), B)
    gather_and_check(seqs, store, idx, f"B = {B}")


# ---- alignment, sentinel and guard bands ------------------------------------------------
def carved(shapes, offset):
    """Tensors of ``shapes`` carved from one sentinel-filled int32 buffer, each
    ``offset`` floats past a 256-byte boundary with at least 4 KiB of sentinel
    before and after it.  Returns (buffer, {name: fp32 view}, {name: (lo, hi)})."""
    sizes = {n: int(np.prod(s)) for n, s in shapes.items()}
    span = {n: GUARD_FLOATS + 64 + (sz + 63) // 64 * 64 for n, sz in sizes.items()}
    buf = torch.full((sum(span.values()) + GUARD_FLOATS + 64,), SENTINEL, dtype=torch.int32, device=DEV)
    base = (-buf.data_ptr() // 4) % 64  # first element on a 256-byte boundary
    views, where, at = {}, {}, base + GUARD_FLOATS
    for n, s in shapes.items():
        lo = at + offset
        views[n] = buf[lo:lo + sizes[n]].view(torch.float32).view(s)
        assert views[n].data_ptr() % 256 == 4 * offset
        where[n] = (lo, lo + sizes[n])
        at += span[n]
    return buf, views, where


def untouched_outside(buf, where):
    keep = torch.ones_like(buf, dtype=torch.bool)
    for lo, hi in where.values():
        keep[lo:hi] = False
    return bool((buf[keep] == SENTINEL).all())


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("case", ["h36m_pad", "pw3d_nopad", "cmu_nopad"])  # rows of 66, 69 and 75 floats
def test_every_output_alignment_inside_guard_bands(case, offset):
    """Outputs 0..3 floats past a 256-byte boundary, pre-filled with a NaN
    sentinel: every element of every row is overwritten with the right value
    and nothing outside the tensors changes."""
    seqs, store = fixture_set(case)
    idx = [3, 0, 2, 2, 1]
    T, D, Du = seqs.seq_len, seqs.n_dims, len(seqs.dim_used)
    assert Du == {"h36m_pad": 66, "pw3d_nopad": 69, "cmu_nopad": 75}[case]
    buf, views, where = carved({n: (len(idx), T, D if n == "all_seqs" else Du) for n in H.NAMES}, offset)
    got = seqs.gather(index(idx), out=views)
    torch.cuda.synchronize()
    assert all(g is views[n] for g, n in zip(got, H.NAMES))
    same(got, H.expected_batch(store, idx), f"{case} +{offset}")
    assert untouched_outside(buf, where)


# ---- indices ----------------------------------------------------------------------------
def test_duplicates_descending_and_the_mirrored_half():
    seqs, store = fixture_set("pw3d_pad_mirror")
    assert len(seqs) == 8 and seqs.n_windows == 4
    gather_and_check(seqs, store, [2, 2, 2, 6, 6, 2], "duplicates")
    gather_and_check(seqs, store, list(range(7, -1, -1)), "descending")
    got = gather_and_check(seqs, store, [4, 5, 6, 7], "mirrored half")
    same(got, H.reference_batch(H.fixture("pw3d_pad_mirror"), np.arange(4, 8)), "mirrored half against the fixture")


def test_overlapping_windows_of_a_sequence_store():
    rng = np.random.default_rng(11)
    a, b = rng.normal(size=(7, 9)), rng.normal(size=(5, 9))
    seqs = DeviceSequences.from_sequences([a, b], 5, [0, 1, 2, 6, 7, 8], 2, 3, device=DEV, mirror=([0], [2]))
    assert seqs.starts.tolist() == [0, 1, 2, 7] and len(seqs) == 8 and seqs.n_frames == 12
    store = H.store_of(seqs)
    got = gather_and_check(seqs, store, [0, 1, 2, 3, 6, 5, 4, 7, 1], "overlapping")
    # window 1 is window 0 one frame on
    assert torch.equal(got[3][0, 1:], got[3][1, :-1]) and torch.equal(got[2][1, 1:], got[2][2, :-1])
    assert np.array_equal(H.bits(got[3][3]), H.bits(b.astype(np.float32)))


@pytest.mark.parametrize("case", ["h36m_pad", "h36m_nopad_mirror", "h36m_pad_mirror_scale"])
def test_indices_outside_the_set_leave_their_rows_alone(case):
    """-1 and 2N (N for a set without on-the-fly mirror) in a batch: those rows
    keep the NaN sentinel, every other row is right, no error is pending."""
    seqs, store = fixture_set(case)
    n = len(seqs)
    idx = [1, -1, 0, 2 * seqs.n_windows, n - 1, n, -2 ** 40, 2 ** 40]
    T, D, Du = seqs.seq_len, seqs.n_dims, len(seqs.dim_used)
    buf, views, where = carved({k: (len(idx), T, D if k == "all_seqs" else Du) for k in H.NAMES}, 0)
    got = seqs.gather(index(idx), out=views)
    torch.cuda.synchronize()
    assert H.hip_last_error() == 0
    want = H.expected_batch(store, idx)
    valid = [b for b, w in enumerate(idx) if 0 <= w < n]
    assert valid == [0, 2, 4]
    for name, g, w in zip(H.NAMES, got, want):
        g = H.bits(g)
        assert np.array_equal(g[valid], H.bits(w)[valid]), name
        rest = np.delete(g, valid, axis=0)
        assert (rest == np.int32(SENTINEL)).all(), name
    assert untouched_outside(buf, where)


# ---- outputs -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["h36m_nopad_mirror", "cmu_pad_scale"])
def test_each_subset_of_outputs(case):
    seqs, store = fixture_set(case)
    idx = [3, 1, len(seqs) - 1]
    want = H.expected_batch(store, idx)
    for k in range(1, 5):
        for subset in itertools.combinations(H.NAMES, k):
            got = seqs.gather(index(idx), outputs=subset)
            assert [g is not None for g in got] == [n in subset for n in H.NAMES]
            same(got, want, f"{case} {subset}")
    with pytest.raises(RuntimeError, match="dstd_batch_gather"):
        seqs.gather(index(idx), outputs=())
    torch.cuda.synchronize()


def test_gather_is_ordered_on_the_callers_stream():
    """On a side stream: the index is produced on it, the gather follows, and a
    consumer reads the batch, with no synchronisation in between."""
    seqs, store = fixture_set("cmu_nopad")
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        big = torch.randn(2048, 2048, device=DEV)
        for _ in range(4):
            big = big @ big * 1e-3  # work ahead of the index on this stream
        idx = (torch.arange(4, device=DEV) * 3 + (big.isnan().sum() > -1).long()) % 4  # 1, 0, 3, 2
        inputs, inputs_inv, targets, all_seqs = seqs.gather(idx)
        doubled = targets * 2 + inputs - inputs_inv
        tail = all_seqs[:, -1].clone()
    stream.synchronize()
    want = H.expected_batch(store, [1, 0, 3, 2])
    assert idx.tolist() == [1, 0, 3, 2]
    assert np.array_equal(H.bits(doubled), H.bits(want[2] * 2 + want[0] - want[1]))
    assert np.array_equal(H.bits(tail), H.bits(want[3][:, -1]))


# ---- the engine takes the loader as it takes the reference's ---------------------------------
class _Log:
    def info(self, *a, **k):
        pass


def test_engine_trains_and_tests_from_the_device_loader_bit_for_bit():
    """Three steps at B = 2 (inverse pass, jl2 + tl2) and one test pass: from
    float64 host 4-tuples, what a DataLoader over the reference's dataset
    yields, and from DeviceLoader over the same windows.  Losses, parameters,
    BatchNorm buffers and metrics are bit-equal."""
    from engine import PredictionEngine
    c = H.fixture("h36m_nopad_mirror")
    windows = c["all_seqs"][:6]  # float64 [6][35][96]
    du = c["dim_used"]
    seqs = DeviceSequences.from_windows(windows, du, 10, 25, padding=True, device=DEV)
    fin, finv = seqs._frame_in.cpu().numpy(), seqs._frame_inv.cpu().numpy()
    used = windows[:, :, du]
    host = [tuple(torch.from_numpy(np.ascontiguousarray(a[i:i + 2])) for a in
                  (used[:, fin], used[:, finv], used, windows)) for i in (0, 2, 4)]
    assert all(t.dtype == torch.float64 and not t.is_cuda for b in host for t in b)
    opts = dict(input_channels=6, input_time_frame=10, output_time_frame=25, st_gcnn_dropout=0.0,
                joints_to_consider=22, num_feature=16, num_layers=1, layout="h36m")
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5),
               loss=dict(joint=["jl2", 1], transition=["tl2", 1]), n_out=1, transform="tsc", use_weight=False,
               inverse=True)
    frames = [1, 3, 7, 9, 13, 24]

    def run(loader):
        torch.manual_seed(0)
        m = get_model("dstdgcn", dstdgcn=opts).to(DEV)
        eng = PredictionEngine(cfg, m.train(), _Log())
        steps = []
        step = eng._step
        eng._step = lambda *a: steps.append(step(*a)) or steps[-1]
        total = eng.train(loader, 0)
        err, per_frame = eng.test(loader, input_n=10, eval_frame=frames, dim_used=du)
        out = {"total": torch.tensor(total, dtype=torch.float64), "err": torch.tensor(err, dtype=torch.float64),
               "per_frame": torch.from_numpy(np.asarray(per_frame, dtype=np.float64)),
               "losses": torch.stack([torch.stack([v.detach().reshape(()) for v in s]) for s in steps]).cpu()}
        out.update({"param " + n: p.detach().cpu() for n, p in m.named_parameters()})
        out.update({"buffer " + n: t.detach().cpu() for n, t in m.named_buffers()})
        return out

    a = run(host)
    b = run(DeviceLoader(seqs, 2, shuffle=False))
    assert a["losses"].shape == (3, 2) and bool(torch.isfinite(a["losses"]).all())
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert any(k.startswith("buffer ") and k.endswith("running_mean") for k in a)
    assert float(a["err"]) > 0
