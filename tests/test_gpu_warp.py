"""MI355X checks of the warping gather (include/ext/dstd_gcn_warp.h,
DeviceSequences.gather(rate=), fit_rate, DeviceLoader(augment=Augment(speed=))).

Every comparison is equality of int32 views, no tolerance anywhere: the header
fixes every rounding, and tests/warp_helper.py expected_warp restates it in
explicit fp32 steps (tests/test_warp_host.py pins the restatement).

The ABI-level tests run on exact-size buffers between guard bands
(tests/guard_helper.py Guarded): the frames, every table, the index, the rates,
the transforms and all four outputs.  The bands hold a NaN sentinel word, so
the bytes directly after the last stored frame are poison that must never show
up in an output; outputs start as 0xFF bytes, which an unwritten row keeps.

Shapes: two sequences of 9 and 7 frames at T = 4 (2 in + 2 out) give windows
with 3 to 8 rows of room, so that 1.75 stays inside the room of the early
windows and runs past it on the late ones; D = 9 with dim_used [1, 3, 5, 7, 8]
splits joints; 112 to 128 batch rows are 448 to 512 destination rows, more than
a hundred blocks.  H36M's shape (T = 35, D = 96, 66 used columns, B = 32) runs
once.
"""
import numpy as np
import pytest
import torch

import augment_helper as A
import data_helper as H
import dstd_native as native
import guard_helper as G
import warp_helper as W
from dstd_data import Augment, DeviceLoader, DeviceSequences
from model import get_model
from test_gpu_data import index, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1
F32 = np.float32
UNWRITTEN = np.int32(-1)  # an output word before the call: 0xFF bytes
POISON = np.int32(G.SENTINEL)  # what lies directly after every guarded buffer
T, DIM_USED = 4, [1, 3, 5, 7, 8]
LENGTHS = (9, 7)
ROOM = [8, 7, 6, 5, 4, 3, 6, 5, 4, 3]


def device_xf(xf):
    return None if xf is None else torch.from_numpy(np.ascontiguousarray(xf, dtype=F32)).to(DEV)


def _sequences(lengths=LENGTHS, d=9, seed=0):
    """Random sequences with a -0.0 and a large-magnitude entry."""
    rng = np.random.default_rng(seed)
    seqs = [rng.normal(size=(n, d)) * 100 for n in lengths]
    seqs[0][2, 4] = -0.0
    seqs[0][6, 7] = 3e30
    seqs[-1][-1, 0] = -0.0
    return seqs


_sets = {}


def base_set(kind):
    """(DeviceSequences, host store arrays) of the base set: "plain", "mirror"
    (on the fly), "nopad" (every frame in both input tensors) or "scaled"
    (the `used` path)."""
    if kind not in _sets:
        kw = dict(mirror=([0], [2])) if kind == "mirror" else {}
        if kind == "scaled":
            kw = dict(scaler=(np.linspace(-50, 50, 5), np.linspace(20, 90, 5)))
        seqs = DeviceSequences.from_sequences(_sequences(), T, DIM_USED, 2, 2, padding=kind != "nopad", device=DEV, **kw)
        assert seqs.room.tolist() == ROOM and (seqs._used is not None) == (kind == "scaled")
        _sets[kind] = (seqs, H.store_of(seqs))
    return _sets[kind]


# ---- guarded buffers ------------------------------------------------------------------------
def _guarded(arr, dtype):
    a = np.ascontiguousarray(arr, dtype=dtype)
    g = G.Guarded(a.nbytes, 0x00, DEV)
    g.tensor.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))
    return g, a


class GuardedStore:
    """A dstd_seq_store whose frames and tables (the room table included) are
    exact-size guarded buffers."""

    def __init__(self, store, room):
        self.store, self.room = store, None if room is None else np.asarray(room)
        self.bufs = {}
        F, D = store["frames"].shape
        fields = {}
        for name, dtype in (("frames", F32), ("used", F32), ("starts", np.int64), ("dim_used", np.int32),
                            ("frame_in", np.int32), ("frame_inv", np.int32), ("mirror_src", np.int32)):
            fields[name] = self._put(name, store[name], dtype)
        self.room_ptr = self._put("room", self.room, np.int32)
        self.c = native.SeqStore(F=F, N=len(store["starts"]), T=store["T"], D=D, Du=len(store["dim_used"]), **fields)

    def _put(self, name, arr, dtype):
        if arr is None:
            return None
        self.bufs[name] = _guarded(arr, dtype)
        return self.bufs[name][0].ptr

    def check(self, what):
        for name, (g, host) in self.bufs.items():
            g.check(f"{what}: {name}")
            assert np.array_equal(g.tensor.cpu().numpy(), host.reshape(-1).view(np.uint8)), f"{what}: {name} was written"


_guarded_stores = {}


def guarded_store(kind, room="own"):
    key = (kind, room if isinstance(room, str) or room is None else tuple(room))
    if key not in _guarded_stores:
        seqs, store = base_set(kind)
        _guarded_stores[key] = GuardedStore(store, seqs.room if isinstance(room, str) else room)
    return _guarded_stores[key]


def warp_call(gs, idx, rate, xf, amp, seed, names=H.NAMES, room=True, what="", expect=0):
    """dstd_batch_gather_warp on guarded buffers: returns {name: fp32 tensor};
    checks the return code, that no error is pending, every guard band, and
    that no input was written."""
    B = len(idx)
    ins = {"index": _guarded(idx, np.int64)}
    if rate is not None:
        ins["rate"] = _guarded(rate, F32)
    if xf is not None:
        ins["xf"] = _guarded(np.asarray(xf, dtype=F32).reshape(B, 12), F32)
    outs = {n: G.Guarded(4 * B * gs.c.T * (gs.c.D if n == "all_seqs" else gs.c.Du), 0xFF, DEV) for n in names}

    def p(d, n):
        g = d.get(n)
        return None if g is None else (g[0] if isinstance(g, tuple) else g).ptr

    code = native.lib().dstd_batch_gather_warp(
        native.ext_warp.seq_store_ref(gs.c), gs.room_ptr if room else None, p(ins, "index"), B, p(ins, "rate"),
        p(ins, "xf"), amp, seed, *(p(outs, n) for n in H.NAMES), native.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    assert code == expect and H.hip_last_error() == 0, (what, code)
    gs.check(what)
    for name, (g, host) in ins.items():
        g.check(f"{what}: {name}")
        assert np.array_equal(g.tensor.cpu().numpy(), host.reshape(-1).view(np.uint8)), f"{what}: {name} was written"
    for name, g in outs.items():
        g.check(f"{what}: {name}")
    return {n: g.view(torch.float32, (B, gs.c.T, gs.c.D if n == "all_seqs" else gs.c.Du)) for n, g in outs.items()}


def check_outputs(got, want, what):
    """got {name: tensor} against the helper's four arrays (NaN: unwritten),
    bit for bit; the poison around the buffers shows up nowhere."""
    for name, w in zip(H.NAMES, want):
        if name not in got:
            continue
        g = H.bits(got[name])
        wb = np.where(np.isnan(w), UNWRITTEN, H.bits(w))
        bad = np.nonzero(g.reshape(-1) != wb.reshape(-1))[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} of {w.size} elements, first flat index {bad[0]}"
        assert not (g == POISON).any(), f"{what}: {name} holds poison"


def exact_rate(room, frames=T - 1):
    """An fp32 rate whose fp32 product with ``frames`` is ``room`` exactly."""
    r = F32(room) / F32(frames)
    if r * F32(frames) != room:
        r = np.nextafter(r, F32(np.inf))
    assert r.dtype == F32 and r * F32(frames) == room
    return r


RATES = (1.0, 0.5, 1 / 3, 1.75, "exact", 0.0, -2.0, float("nan"))


def contract_batch(seqs):
    """Every window, two mirrored windows where the set has them, a repeated
    window and indices outside the set, each at every rate of RATES."""
    n, full = seqs.n_windows, len(seqs)
    base = list(range(n)) + ([n + 3, full - 1] if full > n else []) + [3, 3, full, -1]
    idx = np.tile(base, len(RATES))
    rate = np.empty(len(idx), dtype=F32)
    for k, r in enumerate(RATES):
        for j, w in enumerate(base):
            rate[k * len(base) + j] = exact_rate(ROOM[w % n] if 0 <= w < full else 3) if r == "exact" else r
    return idx, rate


# ---- the contract ---------------------------------------------------------------------------
@pytest.mark.parametrize("augmented", [False, True], ids=["warp", "warp+xf+noise"])
@pytest.mark.parametrize("kind", ["plain", "mirror", "nopad"])
def test_contract_all_outputs_and_each_alone(kind, augmented):
    seqs, store = base_set(kind)
    gs = guarded_store(kind)
    idx, rate = contract_batch(seqs)
    assert len(idx) * T > 4 * 64  # more than one block, more than one pass of a small grid
    xf = A.random_transforms(len(idx), seed=2) if augmented else None
    amp, seed = (1.5, 2 ** 63 + 11) if augmented else (0.0, 0)
    want = W.expected_warp(store, idx, rate, seqs.room, xf, amp, seed)
    # the rates do what the shapes were chosen for: 1.75 blends inside the early windows' room and is
    # past it on the late ones; every unwritten row is an index outside the set
    unwritten = np.isnan(want[3]).all(axis=(1, 2))
    assert np.array_equal(unwritten, (idx < 0) | (idx >= len(seqs))) and not np.isnan(want[3][~unwritten]).any()
    assert W.position(1.75, 3, ROOM[0]) == (5, 0.25) and W.position(1.75, 3, ROOM[5]) == (3, 0)
    got = warp_call(gs, idx, rate, xf, amp, seed, what=kind)
    check_outputs(got, want, kind)
    for name in H.NAMES:
        alone = warp_call(gs, idx, rate, xf, amp, seed, names=(name,), what=f"{kind} {name} alone")
        check_outputs(alone, want, f"{kind} {name} alone")
    # rate 1 rows are the unwarped rows; rate 0, negative and NaN rows repeat the window's first frame
    plain = H.bits(A.expected_aug(store, idx, xf, amp, seed)[3])
    per = len(idx) // len(RATES)
    a, ok = H.bits(got["all_seqs"]), ~unwritten[:per]
    assert np.array_equal(a[:per][ok], plain[:per][ok])
    for k in (5, 6, 7):
        rows, unwarped = a[k * per:(k + 1) * per][ok], plain[k * per:(k + 1) * per][ok]
        assert (rows == rows[:, :1]).all() and np.array_equal(rows[:, 0], unwarped[:, 0])


def test_composition_padded_rows_and_shared_frames():
    """Mirror, rate, transform and noise together: padded input rows are copies
    of the frame they repeat; without padding every frame is seen by both input
    tensors and carries the same noise in both."""
    seqs, store = base_set("mirror")
    idx, rate = contract_batch(seqs)
    xf = A.random_transforms(len(idx), seed=4)
    got = warp_call(guarded_store("mirror"), idx, rate, xf, 2.0, 77, what="composition")
    check_outputs(got, W.expected_warp(store, idx, rate, seqs.room, xf, 2.0, 77), "composition")
    ok = (idx >= 0) & (idx < len(seqs))
    i, v = H.bits(got["inputs"])[ok], H.bits(got["inputs_inv"])[ok]
    assert store["frame_in"].tolist() == [0, 1, 1, 1] and store["frame_inv"].tolist() == [3, 2, 2, 2]
    for s in (2, 3):
        assert np.array_equal(i[:, s], i[:, 1]) and np.array_equal(v[:, s], v[:, 1])
    clean = warp_call(guarded_store("mirror"), idx, rate, xf, 0.0, 77, what="composition, clean")
    assert not np.array_equal(H.bits(clean["inputs"])[ok], i)
    assert np.array_equal(H.bits(clean["targets"]), H.bits(got["targets"]))  # noise goes to the inputs alone
    seqs, store = base_set("nopad")
    idx, rate = contract_batch(seqs)
    got = warp_call(guarded_store("nopad"), idx, rate, None, 2.0, 77, what="shared frames")
    assert store["frame_in"].tolist() == [0, 1, 2, 3] and store["frame_inv"].tolist() == [3, 2, 1, 0]
    assert np.array_equal(H.bits(got["inputs"]), H.bits(got["inputs_inv"])[:, ::-1])
    assert not np.array_equal(H.bits(got["inputs"]), H.bits(got["targets"]))


# ---- identities -----------------------------------------------------------------------------
@pytest.mark.parametrize("augmented", [False, True], ids=["plain", "xf+noise"])
@pytest.mark.parametrize("kind", ["mirror", "scaled"])
def test_no_rate_and_unit_rates_are_the_augmenting_gather(kind, augmented):
    """rate NULL, and all-ones rates, against dstd_batch_gather_aug on the
    same arguments (a scaled set takes no transform: noise alone)."""
    seqs, store = base_set(kind)
    idx = list(range(len(seqs))) + [3, 3, -1, len(seqs)]
    B = len(idx)
    ix = index(idx)
    xf = device_xf(A.random_transforms(B, seed=6)) if augmented and kind != "scaled" else None
    amp, seed = (0.75, 99) if augmented else (0.0, 0)
    ones = torch.ones(B, dtype=torch.float32, device=DEV)
    stream = native.stream_handle(torch.device(DEV))
    shapes = [(B, T, 9 if n == "all_seqs" else 5) for n in H.NAMES]

    def fresh():
        return [torch.full(s, float("nan"), device=DEV) for s in shapes]

    want = fresh()
    code = native.lib().dstd_batch_gather_aug(native.ext_augment.seq_store_ref(seqs._store), ix.data_ptr(), B,
                                              xf.data_ptr() if xf is not None else None, amp, seed,
                                              *(t.data_ptr() for t in want), stream)
    assert code == 0
    for room in (seqs._room.data_ptr(), None):
        for rate in (None, ones):
            got = fresh()
            code = native.lib().dstd_batch_gather_warp(
                native.ext_warp.seq_store_ref(seqs._store), room, ix.data_ptr(), B,
                rate.data_ptr() if rate is not None else None, xf.data_ptr() if xf is not None else None, amp, seed,
                *(t.data_ptr() for t in got), stream)
            torch.cuda.synchronize()
            assert code == 0 and H.hip_last_error() == 0
            for name, g, w in zip(H.NAMES, got, want):
                assert np.array_equal(H.bits(g), H.bits(w)), (kind, name, room is None, rate is None)
    same(want, A.expected_aug(store, idx, None if xf is None else xf.cpu().numpy(), amp, seed), kind)
    if xf is None:
        assert (H.bits(want[3]) == np.int32(-2 ** 31)).any()  # the -0.0 is in the batch and survived


# ---- the scaled set -------------------------------------------------------------------------
def test_scaled_set_takes_rates_and_noise_and_refuses_a_transform():
    seqs, store = base_set("scaled")
    gs = guarded_store("scaled")
    idx, rate = contract_batch(seqs)
    want = W.expected_warp(store, idx, rate, seqs.room, None, 0.5, 21)
    got = warp_call(gs, idx, rate, None, 0.5, 21, what="scaled")
    check_outputs(got, want, "scaled")
    assert not np.array_equal(H.bits(got["targets"]), H.bits(got["all_seqs"][:, :, DIM_USED]))  # the `used` values
    # through the Python layer, too
    out = {n: torch.full(w.shape, float("nan"), device=DEV) for n, w in zip(H.NAMES, want)}
    same(seqs.gather(index(idx), out=out, noise=0.5, noise_seed=21, rate=torch.from_numpy(rate).to(DEV)), want,
         "scaled, gather(rate=)")
    xf = A.random_transforms(len(idx))
    refused = warp_call(gs, idx, rate, xf, 0.5, 21, what="scaled with xf", expect=EINVAL)
    assert all((H.bits(t) == UNWRITTEN).all() for t in refused.values())  # nothing written
    with pytest.raises(ValueError, match="scaled"):
        seqs.gather(index(idx), transform=device_xf(xf), rate=torch.from_numpy(rate).to(DEV))
    torch.cuda.synchronize()
    assert H.hip_last_error() == 0


# ---- room ----------------------------------------------------------------------------------
def test_without_a_room_table_a_window_freezes_at_its_own_last_frame():
    """room = NULL: every rate above 1 ends at frame T - 1 of the window itself,
    also for windows with stored frames after them; the set's last window has a
    guard band after its last frame, and none of it is read."""
    seqs, store = base_set("plain")
    gs = guarded_store("plain")
    n = seqs.n_windows
    idx = np.array(list(range(n)) * 3)
    rate = np.repeat(np.array([1.75, 3.0, 1e30], dtype=F32), n)
    assert int(store["starts"][n - 1]) + T == store["frames"].shape[0]  # the last window ends the stored frames
    got = warp_call(gs, idx, rate, None, 0.0, 0, room=False, what="room NULL")
    check_outputs(got, W.expected_warp(store, idx, rate, None), "room NULL")
    last = store["frames"][store["starts"][idx] + T - 1]
    a = got["all_seqs"].cpu().numpy()
    assert np.array_equal(H.bits(a[:, T - 1]), H.bits(last)) and np.array_equal(H.bits(a[:, 2]), H.bits(last))
    # with the table the early windows do read on: the two calls differ there and only there
    roomy = warp_call(gs, idx, rate, None, 0.0, 0, what="room table")
    differs = (H.bits(roomy["all_seqs"]) != H.bits(a)).any(axis=(1, 2))
    assert differs[0] and not differs[n - 1] and not differs[5]  # windows 5 and 9 have room 3 = T - 1


def test_room_table_entries_beyond_the_stored_frames_and_below_the_window():
    """At the ABI a table may lie: an entry that reaches past the last stored
    frame is capped there (the poison directly after it never shows up), and
    an entry below T - 1 leaves its rows unwritten."""
    seqs, store = base_set("mirror")
    room = np.array(ROOM)
    room[9], room[5], room[2] = 2 ** 31 - 1, 1000, 2
    gs = guarded_store("mirror", room)
    idx, rate = contract_batch(seqs)
    idx = np.concatenate((idx, [9, 19, 5, 15, 9]))
    rate = np.concatenate((rate, np.array([1e6, 3e38, 50.0, float("inf"), 1.9], dtype=F32)))
    want = W.expected_warp(store, idx, rate, room)
    assert np.isnan(want[3][idx % 10 == 2]).all() and not np.isnan(want[3][-5:]).any()
    assert np.array_equal(H.bits(want[3][-5, 3]), H.bits(store["frames"][15]))  # the last stored frame
    got = warp_call(gs, idx, rate, None, 0.0, 0, what="lying room table")
    check_outputs(got, want, "lying room table")


# ---- a real shape ---------------------------------------------------------------------------
def _h36m_set():
    du = [int(c) for c in H.fixture("h36m_pad")["dim_used"]]
    rng = np.random.default_rng(5)
    seqs = [np.cumsum(rng.normal(0, 10, (n, 96)), 0) for n in (50, 41, 77)]
    left, right = [1, 2, 3, 4, 5, 17, 18, 19, 20, 21, 22, 23], [6, 7, 8, 9, 10, 25, 26, 27, 28, 29, 30, 31]
    s = DeviceSequences.from_sequences(seqs, 35, du, 10, 25, device=DEV, mirror=(left, right))
    assert (s.seq_len, s.n_dims, len(s.dim_used), s.n_windows, len(s)) == (35, 96, 66, 66, 132)
    return s


def test_h36m_shape_with_the_loaders_rates():
    seqs = _h36m_set()
    store = H.store_of(seqs)
    aug = Augment(rotate=(1, 3.14159), scale=(0.9, 1.1), shift=20.0, noise=2.0, speed=(0.7, 1.5))
    loader = DeviceLoader(seqs, 32, shuffle=True, seed=3, augment=aug)
    batch = next(iter(loader))
    torch.cuda.synchronize()
    idx, rate = loader.last_index.cpu().numpy(), loader.last_rate.cpu().numpy()
    assert len(idx) == 32 and rate.dtype == F32 and rate.min() >= F32(0.7) and rate.max() > 1 and rate.min() < 1
    want = W.expected_warp(store, idx, rate, seqs.room, loader.last_transform.cpu().numpy(), 2.0,
                           loader.last_noise_seed)
    same(batch, want, "h36m shape")
    plain = seqs.gather(loader.last_index, transform=loader.last_transform, noise=2.0,
                        noise_seed=loader.last_noise_seed)
    assert not np.array_equal(H.bits(plain[3]), H.bits(batch[3]))
    assert np.array_equal(H.bits(plain[3][:, 0]), H.bits(batch[3][:, 0]))  # frame 0 is the window's start at any rate
    assert H.hip_last_error() == 0


# ---- the loader -----------------------------------------------------------------------------
def _epochs(loader, n=2):
    out = []
    for _ in range(n):
        for batch in loader:
            rate = loader.last_rate
            out.append((loader.last_index.clone(), None if rate is None else rate.clone(), [t.clone() for t in batch]))
    return out


def test_loader_is_reproducible_fits_every_rate_and_unit_speed_changes_nothing():
    seqs, store = base_set("mirror")
    kw = dict(rotate=(1, 0.5), scale=(0.9, 1.1), noise=1.0)

    def loader(**more):
        return DeviceLoader(seqs, 6, shuffle=True, seed=4, augment=Augment(**kw, **more))

    a, b = _epochs(loader(speed=(0.5, 2.5))), _epochs(loader(speed=(0.5, 2.5)))
    assert len(a) == len(b) == 8
    room = np.concatenate((seqs.room, seqs.room))
    capped = 0
    for (ia, ra, ta), (ib, rb, tb) in zip(a, b):
        assert torch.equal(ia, ib) and torch.equal(ra, rb)
        assert all(np.array_equal(H.bits(u), H.bits(v)) for u, v in zip(ta, tb))
        r = ra.double().cpu().numpy()
        assert (r * (T - 1) <= room[ia.cpu().numpy()]).all() and r.min() >= 0.5  # no drawn window freezes
        capped += int((r * (T - 1) == room[ia.cpu().numpy()]).sum())
    assert capped > 0 and not torch.equal(a[0][1], a[4][1])  # caps were needed; the second epoch draws anew
    # a yielded batch is the gather its description names
    two = loader(speed=(0.5, 2.5))
    batch = next(iter(two))
    same(batch, W.expected_warp(store, two.last_index.cpu().numpy(), two.last_rate.cpu().numpy(), seqs.room,
                                two.last_transform.cpu().numpy(), 1.0, two.last_noise_seed), "loader batch")
    # speed = (1, 1) against the same loader without speed
    unit, none = _epochs(loader(speed=(1, 1))), _epochs(loader())
    for (iu, ru, tu), (i0, r0, t0) in zip(unit, none):
        assert torch.equal(iu, i0) and r0 is None and ru.tolist() == [1.0] * len(iu)
        assert all(np.array_equal(H.bits(u), H.bits(v)) for u, v in zip(tu, t0))
    assert not all(np.array_equal(H.bits(u), H.bits(v)) for (_, _, x), (_, _, y) in zip(a, none) for u, v in zip(x, y))


# ---- the engine -----------------------------------------------------------------------------
class _Log:
    def info(self, *a, **k):
        pass


@pytest.mark.parametrize("horizon", [None, 12])
def test_engine_trains_from_a_speed_augmenting_loader(horizon):
    """Two steps of train() on the small T = 6 model of tests/test_gpu_rollout.py from a from_sequences
    set under speed, rotation and noise: finite losses, changed parameters -- plain (windows of 3 + 3)
    and through the rollout (3 + 12, horizon = 12); test_groups refuses the loader as it refuses any
    augmenting one."""
    from engine import PredictionEngine
    opts = dict(input_channels=6, input_time_frame=3, output_time_frame=3, st_gcnn_dropout=0.0,
                joints_to_consider=22, num_feature=16, num_layers=1, layout="h36m")
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5),
               loss=dict(joint=["jl2", 1], transition=["tl2", 0.5]), n_out=1, transform="tsc", use_weight=False,
               inverse=True)
    rng = np.random.default_rng(17)
    out_n = horizon or 3
    frames = 3 + out_n
    dim_used = np.sort(rng.choice(96, 66, replace=False))
    seqs = DeviceSequences.from_sequences([np.cumsum(rng.normal(0, 10, (frames + k, 96)), 0) for k in (6, 5)],
                                          frames, dim_used, 3, out_n, device=DEV)
    assert len(seqs) == 13 and seqs.room.max() == frames + 5
    loader = DeviceLoader(seqs, 6, shuffle=True, drop_last=True, seed=2,
                          augment=Augment(speed=(0.8, 1.25), rotate=(1, 0.5), noise=1.0))
    torch.manual_seed(0)
    m = get_model("dstdgcn", dstdgcn=opts).to(DEV).train()
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    eng = PredictionEngine(cfg, m, _Log())
    steps = []
    name = "_step_rollout" if horizon else "_step"
    step = getattr(eng, name)
    setattr(eng, name, lambda *a: steps.append(step(*a)) or steps[-1])
    total = eng.train(loader, 0, horizon=horizon)
    losses = torch.stack([torch.stack([v.detach().reshape(()) for v in s]) for s in steps]).cpu()
    assert losses.shape[0] == 2 and bool(torch.isfinite(losses).all()) and bool((losses > 0).all())
    assert np.isfinite(np.asarray(total, dtype=np.float64)).all()
    assert loader.last_rate is not None and float(loader.last_rate.min()) >= 0.8
    changed = [n for n, p in m.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[n])]
    assert changed and all(bool(torch.isfinite(p).all()) for p in m.parameters())
    with pytest.raises(ValueError, match="augment"):
        eng.test_groups(loader, input_n=3, eval_frame=[0, 1], horizon=horizon)
