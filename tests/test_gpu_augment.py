"""MI355X checks of the augmenting gather (include/ext/dstd_gcn_augment.h,
DeviceSequences.gather(transform=, noise=), DeviceLoader(augment=)).

Every comparison is equality of int32 views, no tolerance anywhere: against
tests/augment_helper.py expected_aug (the header restated in numpy, which
tests/test_augment_host.py pins to data_helper.expected_batch), or against
dstd_batch_gather itself.

Shapes: D = 3 with T = 2 is the smallest the header admits (one joint, one lane
of a wave busy); rows of 66 / 75 floats take two passes of the 64 lanes, 96 and
114 two for all_seqs; dim_used [1, 3, 5, 8] of D = 9 takes single columns of
joints, so a used column reads source columns that are not used.  B = 257 at
T = 35 is 8995 rows, no multiple of the 4 rows of a block; B = 131073 at T = 2
is 262146 rows, two more than the launch's grid cap (65536 blocks of 4 waves)
covers in one pass of its grid-stride loop.
"""
import itertools

import numpy as np
import pytest
import torch

import augment_helper as A
import data_helper as H
from conftest import load_npz
from dstd_data import Augment, DeviceLoader, DeviceSequences
from model import get_model
from test_gpu_data import SENTINEL, carved, fixture_set, index, same, synthetic_set, untouched_outside

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID_CAP_ROWS = (1 << 16) * 4  # kMaxBlocks * DSTD_WAVES of csrc/dstd_augment.hip


def device_xf(xf):
    return None if xf is None else torch.from_numpy(np.ascontiguousarray(xf, dtype=np.float32)).to(DEV)


def aug_and_check(seqs, store, idx, xf, amp, seed, what, **kw):
    got = seqs.gather(index(idx), transform=device_xf(xf), noise=amp, noise_seed=seed, **kw)
    torch.cuda.synchronize()
    same(got, A.expected_aug(store, idx, xf, amp, seed), what)
    return got


def equal_bits(a, b):
    return np.array_equal(H.bits(a), H.bits(b))


# ---- no augmentation ------------------------------------------------------------------------
@pytest.mark.parametrize("case", H.CASES)
def test_without_augmentation_the_entry_point_is_the_plain_gather(case):
    """dstd_batch_gather_aug with xf NULL and amplitude 0, called directly (the
    Python layer would route this to dstd_batch_gather), against
    dstd_batch_gather bit for bit."""
    import dstd_native as native
    seqs, store = fixture_set(case)
    idx = list(range(len(seqs) - 1, -1, -1)) + [0, 0]
    ix = index(idx)
    want = seqs.gather(ix)
    got = [torch.full_like(w, float("nan")) for w in want]
    code = native.lib().dstd_batch_gather_aug(native.ext_augment.seq_store_ref(seqs._store), ix.data_ptr(), len(idx),
                                              None, 0.0, 12345, *(g.data_ptr() for g in got),
                                              native.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    assert code == 0 and H.hip_last_error() == 0
    for name, g, w in zip(H.NAMES, got, want):
        assert equal_bits(g, w), name
    same(got, H.expected_batch(store, idx), case)


# ---- transform, noise, both -----------------------------------------------------------------
def _dim_used(case):
    return [int(c) for c in H.fixture(case)["dim_used"]]


SHAPES = {
    "D=3 T=2": dict(N=3, T=2, D=3, dim_used=[0, 1, 2], input_n=1, mirror=([], [])),
    "D=96 Du=66": dict(N=3, T=5, D=96, dim_used=lambda: _dim_used("h36m_pad"), input_n=2, mirror=([1, 6], [17, 25])),
    "D=75=Du": dict(N=3, T=4, D=75, dim_used=list(range(75)), input_n=3, mirror=([0, 3], [24, 9])),
    "D=114 Du=75": dict(N=2, T=4, D=114, dim_used=lambda: _dim_used("cmu_nopad"), input_n=2, mirror=([2], [37])),
    "single columns of joints": dict(N=4, T=3, D=9, dim_used=[1, 3, 5, 8], input_n=2, mirror=([0], [2])),
}
_shape_sets = {}


def shape_set(name, mirrored, padding):
    key = (name, mirrored, padding)
    if key not in _shape_sets:
        kw = dict(SHAPES[name])
        if callable(kw["dim_used"]):
            kw["dim_used"] = kw["dim_used"]()
        mirror = kw.pop("mirror")
        assert len(kw["dim_used"]) == {"D=96 Du=66": 66, "D=114 Du=75": 75}.get(name, len(kw["dim_used"]))
        _shape_sets[key] = synthetic_set(padding=padding, mirror=mirror if mirrored else None, seed=len(name), **kw)
    return _shape_sets[key]


def shape_index(seqs, seed):
    """Seven rows: every window of the set at least once (the mirrored half
    included), a duplicate pair at rows 0 and 6."""
    n = len(seqs)
    idx = np.random.default_rng(seed).permutation(n)[np.arange(6) % n].tolist()
    return idx + [idx[0]]


@pytest.mark.parametrize("padding", [True, False])
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
def test_transform_only(name, mirrored, padding):
    """General matrices, row 1 the identity and the last row all zeros."""
    seqs, store = shape_set(name, mirrored, padding)
    idx = shape_index(seqs, 1)
    xf = A.random_transforms(len(idx), seed=2)
    assert np.array_equal(xf[1].reshape(3, 4), np.eye(3, 4)) and not xf[-1].any()
    got = aug_and_check(seqs, store, idx, xf, 0.0, 0, name)
    assert not got[3][-1].any() and not got[0][-1].any()  # the zero transform
    clean = seqs.gather(index(idx))
    assert torch.equal(got[3][1], clean[3][1])  # the identity: equal in value
    assert not torch.equal(got[3][0], clean[3][0])
    # [B, 3, 4] is the same argument
    again = seqs.gather(index(idx), transform=device_xf(xf).view(-1, 3, 4))
    assert all(equal_bits(a, b) for a, b in zip(again, got))


def _noise_properties(seqs, store, idx, xf, what):
    amp, seed = 1.5, 2 ** 63 + 11
    clean = seqs.gather(index(idx), transform=device_xf(xf))
    got = aug_and_check(seqs, store, idx, xf, amp, seed, what)
    # targets and all_seqs are those of the noise-free gather
    assert equal_bits(got[2], clean[2]) and equal_bits(got[3], clean[3]), what
    assert not equal_bits(got[0], clean[0]) and not equal_bits(got[1], clean[1]), what
    # padded rows of inputs / inputs_inv are bit-equal to the row they repeat
    for k, fmap in ((0, store["frame_in"]), (1, store["frame_inv"])):
        first = {}
        for s, f in enumerate(fmap.tolist()):
            if f in first:
                assert equal_bits(got[k][:, s], got[k][:, first[f]]), (what, k, s)
            first.setdefault(f, s)
    if seqs.padding:
        assert len(set(store["frame_in"].tolist())) < seqs.seq_len or seqs.output_n == 0
    # the same seed repeats, another seed differs
    again = seqs.gather(index(idx), transform=device_xf(xf), noise=amp, noise_seed=seed)
    other = seqs.gather(index(idx), transform=device_xf(xf), noise=amp, noise_seed=seed + 1)
    assert equal_bits(again[0], got[0]) and equal_bits(again[1], got[1]), what
    assert not equal_bits(other[0], got[0]) and not equal_bits(other[1], got[1]), what
    assert equal_bits(other[2], got[2]) and equal_bits(other[3], got[3]), what
    # duplicate indices in one batch (rows 0 and 6, under one transform) give equal rows
    assert idx[0] == idx[6]
    for k in range(4):
        assert equal_bits(got[k][0], got[k][6]), (what, k)


@pytest.mark.parametrize("padding", [True, False])
@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("both", [False, True], ids=["noise", "transform+noise"])
def test_noise_only_and_with_a_transform(both, name, mirrored, padding):
    seqs, store = shape_set(name, mirrored, padding)
    idx = shape_index(seqs, 3)
    xf = None
    if both:
        xf = A.random_transforms(len(idx), seed=4)
        xf[6] = xf[0]
    _noise_properties(seqs, store, idx, xf, f"{name} {'both' if both else 'noise'}")


@pytest.mark.parametrize("case", ["cmu_pad_scale", "h36m_pad_mirror_scale"])
def test_noise_on_a_scaled_set_and_its_transform_refused(case):
    seqs, store = fixture_set(case)
    assert store["used"] is not None
    idx = shape_index(seqs, 5)
    _noise_properties(seqs, store, idx, None, case)
    with pytest.raises(ValueError, match="scaled"):
        seqs.gather(index(idx), transform=device_xf(A.random_transforms(len(idx))))
    torch.cuda.synchronize()
    assert H.hip_last_error() == 0


# ---- batch sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 257])
def test_batch_sizes(B):
    seqs, store = fixture_set("h36m_nopad_mirror")
    idx = np.random.default_rng(B).integers(0, len(seqs), B)
    aug_and_check(seqs, store, idx, A.random_transforms(B, seed=B), 0.75, B, f"B = {B}")


def test_rows_beyond_the_grid_cap():
    """B = 131073 windows of T = 2, D = 3: 262146 rows, two past what the capped
    grid holds at once, so the last rows come from the grid-stride loop's second
    pass.  The restatement is computed on the distinct (window, transform) pairs
    -- six windows under four transforms -- and expanded by index: the noise
    is keyed by the window, not by the batch row."""
    seqs, store = shape_set("D=3 T=2", True, True)
    T = seqs.seq_len
    B = GRID_CAP_ROWS // T + 1
    assert T == 2 and (B - 1) * T == GRID_CAP_ROWS and B * T > GRID_CAP_ROWS
    rng = np.random.default_rng(8)
    idx = rng.integers(0, len(seqs), B)
    palette = A.random_transforms(4, seed=9)
    which = rng.integers(0, 4, B)
    idx[-1], which[-1] = len(seqs) - 1, 0  # the last row: a mirrored window under a general matrix
    pairs, inverse = np.unique(np.stack([idx, which], 1), axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    assert len(pairs) == len(seqs) * 4
    want = [a[inverse] for a in A.expected_aug(store, pairs[:, 0], palette[pairs[:, 1]], 0.5, 21)]
    got = seqs.gather(index(idx), transform=device_xf(palette[which]), noise=0.5, noise_seed=21)
    torch.cuda.synchronize()
    same(got, want, "beyond the grid cap")
    assert H.hip_last_error() == 0


# ---- memory and ordering --------------------------------------------------------------------
@pytest.mark.parametrize("case", ["h36m_nopad_mirror", "cmu_pad_scale"])
def test_each_subset_of_outputs(case):
    seqs, store = fixture_set(case)
    idx = [3, 1, len(seqs) - 1]
    xf = None if store["used"] is not None else A.random_transforms(3, seed=6)
    want = A.expected_aug(store, idx, xf, 0.25, 3)
    for k in range(1, 5):
        for subset in itertools.combinations(H.NAMES, k):
            got = seqs.gather(index(idx), outputs=subset, transform=device_xf(xf), noise=0.25, noise_seed=3)
            assert [g is not None for g in got] == [n in subset for n in H.NAMES]
            same(got, want, f"{case} {subset}")
    with pytest.raises(RuntimeError, match="dstd_batch_gather_aug"):
        seqs.gather(index(idx), outputs=(), noise=0.25)
    torch.cuda.synchronize()
    assert H.hip_last_error() == 0  # a refusal leaves no error pending


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("case", ["h36m_pad", "pw3d_nopad", "cmu_nopad"])  # rows of 66, 69 and 75 floats
def test_every_output_alignment_inside_guard_bands(case, offset):
    seqs, store = fixture_set(case)
    idx = [3, 0, 2, 2, 1]
    T, D, Du = seqs.seq_len, seqs.n_dims, len(seqs.dim_used)
    buf, views, where = carved({n: (len(idx), T, D if n == "all_seqs" else Du) for n in H.NAMES}, offset)
    xf = A.random_transforms(len(idx), seed=offset)
    got = seqs.gather(index(idx), out=views, transform=device_xf(xf), noise=3.0, noise_seed=offset)
    torch.cuda.synchronize()
    assert all(g is views[n] for g, n in zip(got, H.NAMES))
    same(got, A.expected_aug(store, idx, xf, 3.0, offset), f"{case} +{offset}")
    assert untouched_outside(buf, where)


@pytest.mark.parametrize("case", ["h36m_pad", "h36m_nopad_mirror", "h36m_pad_mirror_scale"])
def test_indices_outside_the_set_leave_their_rows_alone(case):
    """-1, 2N (N without on-the-fly mirror) and +-2^40 in a batch: those rows
    keep the NaN sentinel -- the contract's defined behaviour -- every other row
    is right, nothing outside the tensors changes, no error is pending."""
    seqs, store = fixture_set(case)
    n = len(seqs)
    idx = [1, -1, 0, 2 * seqs.n_windows, n - 1, n, -2 ** 40, 2 ** 40]
    T, D, Du = seqs.seq_len, seqs.n_dims, len(seqs.dim_used)
    buf, views, where = carved({k: (len(idx), T, D if k == "all_seqs" else Du) for k in H.NAMES}, 0)
    xf = None if store["used"] is not None else A.random_transforms(len(idx), seed=7)
    got = seqs.gather(index(idx), out=views, transform=device_xf(xf), noise=0.5, noise_seed=7)
    torch.cuda.synchronize()
    assert H.hip_last_error() == 0
    want = A.expected_aug(store, idx, xf, 0.5, 7)
    valid = [b for b, w in enumerate(idx) if 0 <= w < n]
    assert valid == [0, 2, 4]
    for name, g, w in zip(H.NAMES, got, want):
        g = H.bits(g)
        assert np.array_equal(g[valid], H.bits(w)[valid]), name
        assert (np.delete(g, valid, axis=0) == np.int32(SENTINEL)).all(), name
    assert untouched_outside(buf, where)


def test_gather_is_ordered_on_the_callers_stream():
    """On a side stream: index and transform are produced on it, the gather
    follows, and a consumer reads the batch, with no synchronisation in between."""
    seqs, store = fixture_set("cmu_nopad")
    xf = A.random_transforms(4, seed=12)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        big = torch.randn(2048, 2048, device=DEV)
        for _ in range(4):
            big = big @ big * 1e-3  # work ahead of the index on this stream
        late = (big.isnan().sum() > -1)  # 1, known only when the work is done
        idx = (torch.arange(4, device=DEV) * 3 + late.long()) % 4  # 1, 0, 3, 2
        t = device_xf(xf) * late.float()
        inputs, inputs_inv, targets, all_seqs = seqs.gather(idx, transform=t, noise=1.0, noise_seed=5)
        mixed = targets * 2 + inputs - inputs_inv
        tail = all_seqs[:, -1].clone()
    stream.synchronize()
    want = A.expected_aug(store, [1, 0, 3, 2], xf, 1.0, 5)
    assert idx.tolist() == [1, 0, 3, 2]
    assert equal_bits(mixed, want[2] * 2 + want[0] - want[1])
    assert equal_bits(tail, want[3][:, -1])
    assert H.hip_last_error() == 0


# ---- the loader -----------------------------------------------------------------------------
def _epoch(loader):
    out = []
    for batch in loader:
        out.append((loader.last_index.clone(), loader.last_transform.clone(), loader.last_noise_seed,
                    [t.clone() for t in batch]))
    return out


def test_loader_augments_reproducibly_and_describes_each_batch():
    seqs, store = fixture_set("h36m_nopad_mirror")
    aug = Augment(rotate=(1, 3.14159), scale=(0.9, 1.1), noise=2.0)

    def loader(seed):
        return DeviceLoader(seqs, 3, shuffle=True, seed=seed, augment=aug)

    a, b, c = _epoch(loader(4)), _epoch(loader(4)), _epoch(loader(5))
    assert len(a) == len(b) == len(c) == 3
    for i, ((ia, xa, sa, ta), (ib, xb, sb, tb), (ic, xc, sc, tc)) in enumerate(zip(a, b, c)):
        assert torch.equal(ia, ib) and torch.equal(xa, xb) and sa == sb == DeviceLoader.noise_seed(4, 0, i)
        assert all(equal_bits(u, v) for u, v in zip(ta, tb))
        assert not torch.equal(xa, xc) and sa != sc
        assert not any(u.shape == v.shape and equal_bits(u, v) for u, v in zip(ta, tc))
        # each batch is the gather its description names
        again = seqs.gather(ia, transform=xa, noise=2.0, noise_seed=sa)
        assert all(equal_bits(u, v) for u, v in zip(again, ta))
        same(ta, A.expected_aug(store, ia.tolist(), xa.cpu().numpy(), 2.0, sa), f"loader batch {i}")
        assert xa.is_cuda and tuple(xa.shape) == (len(ia), 12)
    # the order of windows is that of the loader without augment; the second epoch is another one
    plain = DeviceLoader(seqs, 3, shuffle=True, seed=4)
    assert [i.tolist() for i in plain.index_batches()] == [t[0].tolist() for t in a]
    two = loader(4)
    first, second = _epoch(two), _epoch(two)
    assert all(equal_bits(u, v) for x, y in zip(first, a) for u, v in zip(x[3], y[3]))
    assert second[0][2] == DeviceLoader.noise_seed(4, 1, 0) and not torch.equal(second[0][1], first[0][1])
    same_as_seed_5 = _epoch(loader(5))  # epoch 1 of seed 4 is epoch 0 of seed 5: seed + epoch
    assert all(torch.equal(x[1], y[1]) and x[2] == y[2] for x, y in zip(second, same_as_seed_5))


# ---- the engine -----------------------------------------------------------------------------
class _Log:
    def info(self, *a, **k):
        pass


@pytest.mark.parametrize("horizon", [None, 50])
def test_engine_trains_from_the_augmenting_loader_as_from_its_batches(horizon):
    """Two training steps of the H36M fixture model from the augmenting loader, and two
    from a list of the same batches gathered beforehand: the steps' losses and
    every parameter and buffer afterwards are equal.  Plain (windows of 10 + 25
    frames) and through the rollout (10 + 50, horizon = 50)."""
    from engine import PredictionEngine
    c = H.fixture("h36m_nopad_mirror")
    du = c["dim_used"]
    out_n = horizon or 25
    x = np.random.default_rng(13).normal(size=(4, 10 + out_n, 96)) * 100
    seqs = DeviceSequences.from_windows(x, du, 10, out_n, padding=True, device=DEV)
    aug = Augment(rotate=(1, 3.14159), scale=(0.9, 1.1), shift=20.0, noise=2.0)
    d = load_npz("model_h36m.npz")  # the H36M fixture model: 5 layers of 64 features, dropout 0.1
    opts = {k[4:]: d[k].item() for k in d.files if k.startswith("opt/")}
    assert (opts["input_time_frame"], opts["output_time_frame"], opts["joints_to_consider"]) == (10, 25, 22)
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5),
               loss=dict(joint=["jl2", 1], transition=["tl2", 1]), n_out=1, transform="tsc", use_weight=False,
               inverse=True)
    name = "_step_rollout" if horizon else "_step"

    def run(loader):
        m = get_model("dstdgcn", dstdgcn=opts)
        m.load_state_dict({k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd/")})
        m = m.to(DEV)
        eng = PredictionEngine(cfg, m.train(), _Log())
        torch.manual_seed(0)  # the dropout seeds of both runs
        steps = []
        step = getattr(eng, name)
        setattr(eng, name, lambda *a: steps.append(step(*a)) or steps[-1])
        total = eng.train(loader, 0, horizon=horizon)
        out = {"total": torch.tensor(total, dtype=torch.float64),
               "losses": torch.stack([torch.stack([v.detach().reshape(()) for v in s]) for s in steps]).cpu()}
        out.update({"param " + n: p.detach().cpu() for n, p in m.named_parameters()})
        out.update({"buffer " + n: t.detach().cpu() for n, t in m.named_buffers()})
        return out, eng

    def loader():
        return DeviceLoader(seqs, 2, shuffle=True, seed=6, augment=aug)

    batches = [tuple(t.clone() for t in batch) for batch in loader()]
    plain = [tuple(t.clone() for t in batch) for batch in DeviceLoader(seqs, 2, shuffle=True, seed=6)]
    assert len(batches) == 2 and not any(torch.equal(u, v) for p, q in zip(batches, plain) for u, v in zip(p, q))
    (a, eng), (b, _) = run(loader()), run(batches)
    assert a["losses"].shape[0] == 2 and bool(torch.isfinite(a["losses"]).all()) and bool((a["losses"] > 0).all())
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError, match="augment"):
        eng.test_groups(loader(), input_n=10, eval_frame=[0, 1], horizon=horizon)
