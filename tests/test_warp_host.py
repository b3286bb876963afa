"""Host-side checks of the warping gather (include/ext/dstd_gcn_warp.h,
dstd_native.ext_warp, the room table of dstd_data.DeviceSequences, fit_rate,
Augment(speed=) and the speed side of DeviceLoader), and of the numpy
restatement the GPU tests compare against (tests/warp_helper.py).  No GPU
needed: the entry point's refusals come before any HIP call, the draws run on
the CPU device and sets are built with device="cpu"."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import augment_helper as A
import data_helper as H
import dstd_native as native
import warp_helper as W
from abi_reader import compare, parse
from conftest import ROOT
from dstd_data import Augment, DeviceLoader, DeviceSequences, frame_maps
from dstd_native import abi
from test_augment_host import BAD_ARGS, BAD_STORES, _store

EINVAL = -1  # include/dstd_gcn.h
HEADER = "ext/dstd_gcn_warp.h"
NAME = "dstd_batch_gather_warp"
F32 = np.float32


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", *HEADER.split("/"))).read()


# ---- header and binding -------------------------------------------------------------
def test_binding_agrees_with_the_warp_header(header):
    assert compare({HEADER: header}, native.ext_warp) == []
    defines, structs, callbacks, protos = parse(header)
    assert list(protos) == [NAME] and native.ext_warp.WARP_EXPORTS == (NAME,)
    ret, params = protos[NAME]
    assert ret == ("int", 0)
    assert [p[2] for p in params] == ["s", "room", "index", "B", "rate", "xf", "noise_amp", "seed", "inputs",
                                      "inputs_inv", "targets", "all_seqs", "stream"]
    assert [(p[0], p[1]) for p in params] == [
        ("dstd_seq_store", 1), ("int", 1), ("long long", 1), ("int", 0), ("float", 1), ("float", 1), ("float", 0),
        ("unsigned long long", 0), ("float", 1), ("float", 1), ("float", 1), ("float", 1), ("void", 1)]
    i, f, u64, p = ctypes.c_int, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_void_p
    assert native.ext_warp.ABI == {HEADER: {NAME: (i, [p, p, p, i, p, p, f, u64, p, p, p, p, p])}}
    assert (defines, structs, callbacks) == ({}, {}, {}) and native.ext_warp.C_TYPES == {}
    assert '#include "../dstd_gcn_data.h"' in header and "typedef" not in header  # the struct is not redeclared


def test_an_altered_warp_header_is_reported_by_name(header):
    for old, new in (("const int* room, ", ""), ("const float* rate, ", ""), ("const float* rate", "float rate"),
                     ("float noise_amp", "double noise_amp"), ("unsigned long long seed", "unsigned seed")):
        assert old in header
        reports = compare({HEADER: header.replace(old, new, 1)}, native.ext_warp)
        assert {r.split(":")[0] for r in reports} == {NAME}, reports


def test_library_exports_the_entry_point_and_the_other_tables_are_as_they_were():
    L = native.lib()
    restype, argtypes = native.ext_warp.ABI[HEADER][NAME]
    fn = getattr(L, NAME)  # exported, and declared by lib()
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # a table of its own: nothing added to the pinned ones
    assert set(native.ext.ALL) == {"ext/dstd_gcn_rollout.h", "ext/dstd_gcn_teacher.h"}
    assert sum(len(t) for t in native.ext.ALL.values()) == 10
    assert set(native.ext.ABI) == {"ext/dstd_gcn_rollout.h"} and len(native.ext.ABI["ext/dstd_gcn_rollout.h"]) == 6
    pinned = {native.ext_eval: ("ext/dstd_gcn_eval.h", 1), native.ext_augment: ("ext/dstd_gcn_augment.h", 1),
              native.ext_stride: ("ext/dstd_gcn_stride.h", 2), native.ext_stride_train: ("ext/dstd_gcn_stride_train.h", 5)}
    for mod, (name, n) in pinned.items():
        assert list(mod.ABI) == [name] and len(mod.ABI[name]) == n and NAME not in mod.ABI[name], name
    assert set(abi.ABI) == {"dstd_gcn.h", "dstd_gcn_train.h", "dstd_gcn_aux.h", "dstd_gcn_loss.h", "dstd_gcn_taps.h",
                            "dstd_gcn_data.h", "dstd_gcn_predict.h"}
    assert sum(len(t) for t in abi.ABI.values()) == 61 and len(abi.C_TYPES) == 15
    assert not any(NAME in t for t in (*abi.ABI.values(), *native.ext.ALL.values()))
    assert native.ext_warp.seq_store_ref is native.ext_eval.seq_store_ref
    mk = open(os.path.join(ROOT, "dstd-gcn_amd", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "csrc/dstd_warp.hip" in srcs and "csrc/dstd_augment.hip" in srcs
    assert L.dstd_source_hash().decode() == native.source_hash()  # the new sources are hashed


def test_a_library_without_the_symbol_is_a_load_error():
    class Lib:
        _name = "libold.so"

        def __getattr__(self, name):
            if name == NAME:
                raise AttributeError(name)
            return type("Fn", (), {})()

    extra = {**native.ext.ALL, **native.ext_eval.ABI, **native.ext_augment.ABI, **native.ext_warp.ABI}
    with pytest.raises(RuntimeError, match=NAME):
        native.declare(Lib(), extra=extra)
    native.declare(Lib(), allow_missing=True, extra=extra)


# ---- refusals of the entry point ----------------------------------------------------
def _call(store, **kw):
    a = dict(room=0x5800, index=0x6000, B=4, rate=0x6800, xf=0x7000, noise_amp=0.5, seed=7, inputs=0x8000,
             inputs_inv=0x9000, targets=0xA000, all_seqs=0xB000)
    a.update(kw)
    ref = native.ext_warp.seq_store_ref(store) if store is not None else None
    return native.lib().dstd_batch_gather_warp(ref, a["room"], a["index"], a["B"], a["rate"], a["xf"], a["noise_amp"],
                                               a["seed"], a["inputs"], a["inputs_inv"], a["targets"], a["all_seqs"],
                                               None)


# with and without rate, room and xf (pointers that are never dereferenced on the host)
COMBOS = [dict(rate=r, room=m, xf=x) for r in (0x6800, None) for m in (0x5800, None) for x in (0x7000, None)]


@pytest.mark.parametrize("what", list(BAD_STORES))
def test_bad_store_is_einval_before_any_gpu_work(what):
    for combo in COMBOS:
        assert _call(_store(**BAD_STORES[what]), **combo) == EINVAL, combo


@pytest.mark.parametrize("what", list(BAD_ARGS))
def test_bad_argument_is_einval_before_any_gpu_work(what):
    for combo in COMBOS:
        assert _call(_store(), **{**combo, **BAD_ARGS[what]}) == EINVAL, combo


def test_null_store_and_a_transform_of_a_scaled_set_before_any_gpu_work():
    assert _call(None) == EINVAL
    assert native.lib().dstd_batch_gather_warp(None, None, None, 0, None, None, 0.0, 0, None, None, None, None,
                                               None) == EINVAL
    for combo in COMBOS:
        if combo["xf"] is not None:  # xf together with used stays refused, with or without a rate
            assert _call(_store(used=0xC000), **combo) == EINVAL
            assert _call(_store(used=0xC000), noise_amp=0.0, **combo) == EINVAL
    with pytest.raises(TypeError, match="SeqStore"):
        native.ext_warp.seq_store_ref(object())


# ---- room tables ----------------------------------------------------------------------
def _sequences(lengths=(9, 7), d=9, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(n, d)) * 100 for n in lengths]


def test_room_tables_of_the_constructors():
    s = DeviceSequences.from_sequences(_sequences(), 4, [0, 1, 2], 2, 2, device="cpu")
    assert isinstance(s.room, np.ndarray) and s.room.tolist() == [8, 7, 6, 5, 4, 3, 6, 5, 4, 3]
    assert s._room.dtype == torch.int32 and s._room.tolist() == s.room.tolist()
    assert s.starts.tolist() == [0, 1, 2, 3, 4, 5, 9, 10, 11, 12]
    m = DeviceSequences.from_sequences(_sequences(), 4, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]))
    assert m.room.tolist() == s.room.tolist() and len(m) == 20  # on-the-fly mirror: one entry per stored window
    # the stored-mirror case: the doubled sequence list
    sc = DeviceSequences.from_sequences(_sequences(), 4, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]),
                                        scaler=(np.zeros(3), np.ones(3)))
    assert sc.room.tolist() == s.room.tolist() * 2 and len(sc) == 20 and sc.n_frames == 32
    assert int((sc.starts.numpy() + sc.room).max()) == 31
    w = DeviceSequences.from_windows(np.random.default_rng(1).normal(size=(5, 4, 9)), [0, 1, 2], 2, 2, device="cpu")
    assert w.room is None and w._room is None
    # nbytes counts the table: one int32 per stored window
    frames = np.concatenate(_sequences())
    bare = DeviceSequences(frames, s.starts.numpy(), 4, [0, 1, 2], 2, 2, True, "cpu")
    assert bare.room is None and s.nbytes == bare.nbytes + 4 * 10


@pytest.mark.parametrize("bad", [[3, 3, 2], [3, 3], [3, 3, 3, 3], [12, 3, 3], [3, 8, 3], [3, 3, 4], [3.0, 3.0, 3.0], [[3, 3, 3]],
                                 [3, 3, -1]])
def test_a_bad_room_is_a_value_error(bad):
    frames = np.zeros((12, 3))
    with pytest.raises(ValueError, match="room"):
        DeviceSequences(frames, np.array([0, 4, 8]), 4, [0, 1, 2], 2, 2, True, "cpu", room=bad)


def test_room_at_its_bounds_is_accepted():
    frames = np.zeros((12, 3))
    s = DeviceSequences(frames, np.array([0, 4, 8]), 4, [0, 1, 2], 2, 2, True, "cpu", room=[11, 7, 3])
    assert s.room.tolist() == [11, 7, 3] and s.room.dtype == np.int32


# ---- fit_rate -------------------------------------------------------------------------
def test_fit_rate_caps_folds_and_leaves_outside_indices_alone():
    s = DeviceSequences.from_sequences(_sequences(), 4, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]))
    # window 0 has room 8 (cap 8/3), window 5 room 3 (cap 1), window 7 room 5 (cap 5/3); 15 = 10 + 5, 17 = 10 + 7
    idx = torch.tensor([0, 5, 7, 15, 17, -1, 20, 2 ** 40, 0, 0])
    rate = torch.tensor([3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 3.0, 0.5, float("nan")])
    got = s.fit_rate(idx, rate)
    assert got.dtype == torch.float32 and tuple(got.shape) == (10,)
    down = lambda q: float(F32(q) if float(F32(q)) <= q else np.nextafter(F32(q), F32(0)))  # noqa: E731
    want = [down(8 / 3), 1.0, down(5 / 3), 1.0, down(5 / 3), 3.0, 3.0, 3.0, 0.5]
    assert got[:9].tolist() == want and bool(got[9].isnan())
    # the cap times T - 1 never passes the room, in exact arithmetic
    room = np.concatenate((s.room, s.room))
    assert (got[:5].double().numpy() * 3 <= room[idx[:5].numpy()]).all()
    assert rate[0] == 3.0  # the argument is not changed
    # every room of 3..40 at T - 1 = 3, 7 and 34: the cap is the largest fp32 not above room / (T - 1)
    for T in (4, 8, 35):
        n = 38
        t = DeviceSequences(np.zeros((T + n, 3)), np.zeros(n, dtype=np.int64), T, [0], T - 1, 1, True, "cpu",
                            room=np.arange(n) + T - 1)
        cap = t.fit_rate(torch.arange(n), torch.full((n,), 1e9)).double().numpy()
        exact = (np.arange(n) + T - 1) / (T - 1)
        assert (cap * (T - 1) <= np.arange(n) + T - 1).all() and (cap > exact * (1 - 2.0 ** -23)).all()
    # without a room table the cap is 1
    w = DeviceSequences.from_windows(np.zeros((5, 4, 9)), [0, 1, 2], 2, 2, device="cpu")
    assert w.fit_rate(torch.arange(3), torch.tensor([0.5, 1.0, 1.5])).tolist() == [0.5, 1.0, 1.0]
    assert w.fit_rate(torch.tensor([4, -1, 5]), torch.full((3,), 1.5)).tolist() == [1.0, 1.5, 1.5]


# ---- Augment(speed=) --------------------------------------------------------------------
@pytest.mark.parametrize("bad", [(0.0, 1.0), (-0.5, 1.0), (1.1, 0.9), (1.0, float("inf")), (float("nan"), 1.0),
                                 (1.0, float("nan")), 1.0, (1.0,), (0.5, 1.0, 1.5), "fast", (float("inf"),) * 2])
def test_augment_refuses_a_bad_speed(bad):
    with pytest.raises(ValueError, match="speed"):
        Augment(speed=bad)


def test_draw_speed_and_draw_untouched():
    def gen(seed):
        g = torch.Generator(device="cpu")
        g.manual_seed(seed)
        return g

    aug = Augment(speed=(0.8, 1.25))
    assert aug.speed == (0.8, 1.25) and Augment().speed is None
    a, b, c = aug.draw_speed(1000, gen(3), "cpu"), aug.draw_speed(1000, gen(3), "cpu"), aug.draw_speed(1000, gen(4), "cpu")
    assert a.dtype == torch.float32 and tuple(a.shape) == (1000,) and a.is_contiguous() and a.device.type == "cpu"
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert float(a.min()) >= 0.8 and float(a.max()) <= 1.25
    assert float(a.min()) < 0.8 + 0.05 * 0.45 and float(a.max()) > 1.25 - 0.05 * 0.45  # the range is used
    assert Augment(speed=(1, 1)).draw_speed(5, gen(0), "cpu").tolist() == [1.0] * 5
    assert Augment(speed=(0.3, 0.3)).draw_speed(4, gen(0), "cpu").tolist() == [float(F32(0.3))] * 4  # clamped like scale
    assert Augment(rotate=(1, 1.0), noise=2.0).draw_speed(5, gen(0), "cpu") is None
    assert Augment(speed=(0.5, 2.0)).draw(5, gen(0), "cpu") is None  # speed alone configures no transform
    # draw returns the same bits with and without speed, for the same generator state
    for kw in (dict(rotate=(1, 3.0), scale=(0.9, 1.1), shift=1.0), dict(rotate="so3"), dict(scale=(0.5, 2.0))):
        assert torch.equal(Augment(**kw).draw(9, gen(7), "cpu"), Augment(speed=(0.5, 2.0), **kw).draw(9, gen(7), "cpu"))


# ---- DeviceLoader -------------------------------------------------------------------------
def _recorded_epochs(loader, epochs=2):
    """Iterate a loader of a CPU set with the set's gather replaced by a
    recorder: what the loader hands to the gather, per batch."""
    calls = []
    seqs = loader.seqs

    def record(idx, **kw):
        calls.append((idx.clone(), kw))
        return (None,) * 4

    seqs.gather = record
    try:
        for _ in range(epochs):
            for _ in loader:
                pass
    finally:
        del seqs.gather
    return calls


def test_loader_streams_are_the_same_with_and_without_speed():
    s = DeviceSequences.from_sequences(_sequences(), 4, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]))
    kw = dict(rotate=(1, 3.0), scale=(0.9, 1.1), shift=2.0, noise=1.0)
    for shuffle in (False, True):
        plain = DeviceLoader(s, 6, shuffle=shuffle, seed=11, augment=Augment(**kw))
        fast = DeviceLoader(s, 6, shuffle=shuffle, seed=11, augment=Augment(speed=(0.5, 2.5), **kw))
        a = [[i.tolist() for i in plain.index_batches()] for _ in range(2)]
        b = [[i.tolist() for i in fast.index_batches()] for _ in range(2)]
        assert a == b and sorted(sum(a[0], [])) == list(range(20))
        plain.epoch = fast.epoch = 0
        pa, fa = _recorded_epochs(plain), _recorded_epochs(fast)
        assert len(pa) == len(fa) == 8 and plain.last_rate is None
        room = np.concatenate((s.room, s.room))
        rates = []
        for (ia, ka), (ib, kb) in zip(pa, fa):
            assert torch.equal(ia, ib) and torch.equal(ka["transform"], kb["transform"])
            assert ka["noise_seed"] == kb["noise_seed"] and ka["noise"] == kb["noise"] == 1.0
            assert ka["rate"] is None and kb["rate"].dtype == torch.float32 and tuple(kb["rate"].shape) == (len(ib),)
            assert (kb["rate"].double().numpy() * 3 <= room[ib.numpy()]).all() and float(kb["rate"].min()) >= 0.5
            rates.append(kb["rate"])
        assert fast.last_rate is rates[-1]
        assert not torch.equal(rates[0], rates[4])  # the second epoch draws other rates
        # a loader of the same seed repeats them; the rates come from a stream of their own
        again = _recorded_epochs(DeviceLoader(s, 6, shuffle=shuffle, seed=11, augment=Augment(speed=(0.5, 2.5), **kw)))
        assert all(torch.equal(r, k["rate"]) for r, (_, k) in zip(rates, again))
        alone = _recorded_epochs(DeviceLoader(s, 6, shuffle=shuffle, seed=11, augment=Augment(speed=(0.5, 2.5))))
        assert all(torch.equal(r, k["rate"]) and k["transform"] is None for r, (_, k) in zip(rates, alone))


def test_rates_are_not_drawn_from_the_transforms_uniforms():
    """The transform generator is seeded seed + epoch and its first draw is one
    rand(B) (the angle of a single-axis rotation, or the scale without one), as
    a rate draw is: the rate generator's seed carries a tag, so that a sample's
    rate is not an affine image of its angle or scale."""
    f = DeviceLoader.rate_seed
    for seed, epoch in ((0, 0), (4, 1), (2 ** 40 + 3, 9), (-1, 0), (2 ** 64 - 1, 1)):
        assert f(seed, epoch) == ((seed + epoch) ^ DeviceLoader.RATE_STREAM) % 2 ** 64 and 0 <= f(seed, epoch) < 2 ** 64
        assert f(seed, epoch) != (seed + epoch) % 2 ** 64 and f(seed, epoch) == f(seed + epoch, 0)
    # speed (0.5, 1) is never capped (a cap is at least 1): last_rate is the draw itself
    s = DeviceSequences.from_sequences(_sequences(), 4, [0, 1, 2], 2, 2, device="cpu")
    lo, hi = 0.5, 1.0
    for shuffle in (False, True):
        # scale (lo, hi) is lo + (hi - lo) * rand(B), the very formula of the rates
        calls = _recorded_epochs(DeviceLoader(s, 5, shuffle=shuffle, seed=11, augment=Augment(speed=(lo, hi), scale=(lo, hi))))
        assert len(calls) == 4
        for idx, kw in calls:
            scale, rate = kw["transform"][:, 0], kw["rate"]
            assert float((scale - rate).abs().max()) > 0.1 * (hi - lo)
        # a single-axis rotation: theta = (2u - 1) * max_angle from the first rand(B)
        calls = _recorded_epochs(DeviceLoader(s, 5, shuffle=shuffle, seed=11,
                                              augment=Augment(speed=(lo, hi), rotate=(1, 3.0), noise=2.0)))
        us = []
        for idx, kw in calls:
            m = kw["transform"].view(-1, 3, 4).double()
            u_theta = (torch.atan2(m[:, 0, 2], m[:, 2, 2]) / 3.0 + 1) / 2  # right-handed about axis 1
            u_rate = (kw["rate"].double() - lo) / (hi - lo)
            assert bool(((u_theta >= 0) & (u_theta <= 1) & (u_rate >= 0) & (u_rate <= 1)).all())
            assert float((u_theta - u_rate).abs().max()) > 0.1
            us.append(torch.stack((u_theta, u_rate)))
        assert abs(float(torch.corrcoef(torch.cat(us, 1))[0, 1])) < 0.9  # 20 samples: not one line


def test_gather_refuses_a_bad_rate_before_any_gpu_work():
    s = DeviceSequences.from_sequences(_sequences(), 4, [0, 1, 2], 2, 2, device="cpu")
    idx = torch.arange(3)
    for bad in (torch.ones(2), torch.ones(3, 1), torch.ones(3).double(), torch.ones(6)[::2], np.ones(3, dtype=F32),
                1.0, torch.ones(3, device="meta")):
        with pytest.raises(ValueError, match="rate"):
            s.gather(idx, rate=bad)
        with pytest.raises(ValueError, match="rate"):  # before the other arguments are looked at
            s.gather(idx, rate=bad, noise=-1.0)
    with pytest.raises(ValueError, match="index"):  # an index that is no tensor, next to a rate
        s.gather([0, 1, 2], rate=torch.ones(3))
    scaled = DeviceSequences.from_sequences(_sequences(), 4, [0, 1, 2], 2, 2, device="cpu",
                                            scaler=(np.zeros(3), np.ones(3)))
    with pytest.raises(ValueError, match="scaled"):
        scaled.gather(idx, rate=torch.ones(3), transform=torch.zeros(3, 12))
    for seqs in (s, scaled):  # a valid rate goes on to the device: there is no CPU gather
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            seqs.gather(idx, rate=torch.ones(3), noise=0.5)


# ---- the restatement itself ---------------------------------------------------------------
def _store_case(mirror=True, seed=3):
    """Sequences of 9 and 7 frames, T = 4, 3 joints, dim_used splitting joints."""
    rng = np.random.default_rng(seed)
    frames = (rng.normal(size=(16, 9)) * 100).astype(F32)
    frames[2, 4] = -0.0
    fwd, inv = frame_maps(2, 2, True)
    starts = np.array([0, 1, 2, 3, 4, 5, 9, 10, 11, 12])
    room = np.array([8, 7, 6, 5, 4, 3, 6, 5, 4, 3])
    return H.store_arrays(frames, starts, 4, [1, 3, 5, 7, 8], fwd, inv, mirror_src=[2, 1, 0] if mirror else None), room


def test_position_rule():
    assert W.position(None, 3, 3) == (3, 0)
    assert W.position(1.0, 3, 8) == (3, 0) and W.position(0.5, 3, 8) == (1, 0.5) and W.position(0.5, 2, 8) == (1, 0)
    assert W.position(1.75, 3, 8) == (5, 0.25) and W.position(1.75, 3, 5) == (5, 0) and W.position(1.75, 3, 4) == (4, 0)
    for rate in (0.0, -2.0, float("nan"), -0.0, float("-inf")):
        assert W.position(rate, 3, 8) == (0, 0)
    assert W.position(float("inf"), 0, 8) == (0, 0) and W.position(float("inf"), 1, 8) == (8, 0)
    i, a = W.position(1 / 3, 2, 8)
    p = F32(1 / 3) * F32(2)
    assert i == 0 and a == p and a.dtype == F32


def test_restated_rate_one_and_no_rate_reproduce_the_window_in_bits():
    for mirror in (False, True):
        s, room = _store_case(mirror)
        idx = [9, 0, 13 if mirror else 3, -1, 5, 5]
        want = H.expected_batch(s, idx)
        for rate in (None, np.ones(6, dtype=F32)):
            for r in (room, None):
                for g, w in zip(W.expected_warp(s, idx, rate, r), want):
                    assert np.array_equal(H.bits(g), H.bits(w))
        xf = A.random_transforms(6, seed=1)
        want = A.expected_aug(s, idx, xf, 1.5, 9)
        for g, w in zip(W.expected_warp(s, idx, np.ones(6, dtype=F32), room, xf, 1.5, 9), want):
            assert np.array_equal(H.bits(g), H.bits(w))
    assert (H.bits(H.expected_batch(s, [0])[3]) == np.int32(-2 ** 31)).any()  # the -0.0 is in a batch and survives


def test_restated_half_speed_is_frames_and_exact_midpoints():
    s, room = _store_case(mirror=False)
    got = W.expected_warp(s, [1, 6], np.full(2, 0.5, dtype=F32), room)
    fr = s["frames"]
    for b, st in ((0, 1), (1, 9)):
        assert np.array_equal(H.bits(got[3][b, 0]), H.bits(fr[st])) and np.array_equal(H.bits(got[3][b, 2]), H.bits(fr[st + 1]))
        for f, i in ((1, 0), (3, 1)):
            x, y = fr[st + i], fr[st + i + 1]
            assert np.array_equal(H.bits(got[3][b, f]), H.bits(x + F32(0.5) * (y - x)))
            mid = (x.astype(np.float64) + y.astype(np.float64)) / 2
            assert (np.abs(got[3][b, f] - mid) <= 2.0 ** -23 * np.maximum(np.abs(x), np.abs(y))).all()
    assert np.array_equal(H.bits(got[2]), H.bits(got[3][:, :, s["dim_used"]]))
    assert np.array_equal(H.bits(got[0]), H.bits(got[2][:, s["frame_in"]]))
    assert np.array_equal(H.bits(got[1]), H.bits(got[2][:, s["frame_inv"]]))


def test_restated_positions_past_the_room_show_the_last_frame_in_room():
    s, room = _store_case(mirror=False)
    fr = s["frames"]
    # window 5 (start 5, room 3) at rate 1.75: frames 0, 1.75, then past the room: row 8, twice
    got = W.expected_warp(s, [5], np.full(1, 1.75, dtype=F32), room)[3][0]
    assert np.array_equal(H.bits(got[0]), H.bits(fr[5]))
    assert np.array_equal(H.bits(got[1]), H.bits(fr[6] + F32(0.75) * (fr[7] - fr[6])))
    assert np.array_equal(H.bits(got[2]), H.bits(fr[8])) and np.array_equal(H.bits(got[3]), H.bits(fr[8]))
    # without a room table every window freezes at its own last frame, also one with frames after it
    got = W.expected_warp(s, [0], np.full(1, 2.0, dtype=F32), None)[3][0]
    assert [np.array_equal(H.bits(g), H.bits(fr[i])) for g, i in zip(got, (0, 2, 3, 3))] == [True] * 4
    # rate * (T - 1) == room exactly: the last frame in room, copied
    got = W.expected_warp(s, [3], np.full(1, 5 / 3, dtype=F32), room)
    assert F32(5 / 3) * F32(3) == 5 and np.array_equal(H.bits(got[3][0, 3]), H.bits(fr[8]))
    # the room is capped by the stored frames, whatever the table says; a room below T - 1 leaves the row alone
    big = room.copy()
    big[9] = 1000
    got = W.expected_warp(s, [9], np.full(1, 100.0, dtype=F32), big)[3][0]
    assert np.array_equal(H.bits(got[1]), H.bits(fr[15]))
    small = room.copy()
    small[2] = 2
    assert np.isnan(W.expected_warp(s, [2], None, small)[3]).all()


def test_restated_mirror_comes_before_the_blend_and_the_transform_after():
    s, room = _store_case(mirror=True)
    rate = np.array([0.5, 1 / 3], dtype=F32)
    xf = A.random_transforms(2, seed=5)
    plain = W.expected_warp(dict(s, mirror_src=None), [4, 7], rate, room)
    mirrored = W.expected_warp(s, [14, 17], rate, room)
    m = plain[3].reshape(2, 4, 3, 3)[:, :, [2, 1, 0]].copy()
    m[..., 0] = -m[..., 0]
    assert np.array_equal(m.reshape(2, 4, 9), mirrored[3])  # equal in value: the blend of negated values
    both = W.expected_warp(s, [14, 17], rate, room, xf, 2.0, 4)
    assert np.array_equal(H.bits(both[3][0]), H.bits(A.affine(mirrored[3][0], xf[0])))
    assert np.array_equal(H.bits(both[2]), H.bits(both[3][:, :, s["dim_used"]]))
    noise = A.jitter(4, 14, 4, s["frame_in"], 5, 2.0)
    assert np.array_equal(H.bits(both[0][0]), H.bits(both[2][0][s["frame_in"]] + noise))
    assert np.array_equal(H.bits(both[0][:, 1]), H.bits(both[0][:, 2]))  # padded rows stay copies
