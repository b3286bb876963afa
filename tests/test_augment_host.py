"""Host-side checks of the augmenting gather (include/ext/dstd_gcn_augment.h,
dstd_native.ext_augment, dstd_data.Augment and the augment side of DeviceLoader /
DeviceSequences.gather), and of the numpy restatement the GPU tests compare
against (tests/augment_helper.py).  No GPU needed: the entry point's refusals
come before any HIP call, Augment.draw runs on the CPU device and sets are built
with device="cpu"."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import augment_helper as A
import data_helper as H
import dstd_native as native
from abi_reader import compare, parse
from conftest import ROOT
from dstd_data import Augment, DeviceLoader, DeviceSequences
from dstd_native import abi

EINVAL = -1  # include/dstd_gcn.h
HEADER = "ext/dstd_gcn_augment.h"
NAME = "dstd_batch_gather_aug"
U = 2.0 ** -24  # unit roundoff of fp32


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", *HEADER.split("/"))).read()


# ---- header and binding -------------------------------------------------------------
def test_binding_agrees_with_the_augment_header(header):
    assert compare({HEADER: header}, native.ext_augment) == []
    defines, structs, callbacks, protos = parse(header)
    assert list(protos) == [NAME] and native.ext_augment.AUGMENT_EXPORTS == (NAME,)
    ret, params = protos[NAME]
    assert ret == ("int", 0)
    assert [p[2] for p in params] == ["s", "index", "B", "xf", "noise_amp", "seed", "inputs", "inputs_inv", "targets",
                                      "all_seqs", "stream"]
    assert [(p[0], p[1]) for p in params] == [
        ("dstd_seq_store", 1), ("long long", 1), ("int", 0), ("float", 1), ("float", 0), ("unsigned long long", 0),
        ("float", 1), ("float", 1), ("float", 1), ("float", 1), ("void", 1)]
    i, f, u64, p = ctypes.c_int, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_void_p
    assert native.ext_augment.ABI == {HEADER: {NAME: (i, [p, p, i, p, f, u64, p, p, p, p, p])}}
    assert (defines, structs, callbacks) == ({}, {}, {}) and native.ext_augment.C_TYPES == {}
    assert '#include "../dstd_gcn_data.h"' in header and "typedef" not in header  # the struct is not redeclared


def test_an_altered_augment_header_is_reported_by_name(header):
    for old, new in (("const float* xf, ", ""), ("unsigned long long seed", "unsigned seed"),
                     ("float noise_amp", "double noise_amp")):
        assert old in header
        reports = compare({HEADER: header.replace(old, new, 1)}, native.ext_augment)
        assert {r.split(":")[0] for r in reports} == {NAME}, reports


def test_library_exports_the_entry_point_and_the_other_tables_are_as_they_were():
    L = native.lib()
    restype, argtypes = native.ext_augment.ABI[HEADER][NAME]
    fn = getattr(L, NAME)  # exported, and declared by lib()
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # a table of its own: nothing added to the pinned ones
    assert set(native.ext.ALL) == {"ext/dstd_gcn_rollout.h", "ext/dstd_gcn_teacher.h"}
    assert sum(len(t) for t in native.ext.ALL.values()) == 10
    assert set(native.ext.ABI) == {"ext/dstd_gcn_rollout.h"} and len(native.ext.ABI["ext/dstd_gcn_rollout.h"]) == 6
    assert list(native.ext_eval.ABI) == ["ext/dstd_gcn_eval.h"] and len(native.ext_eval.ABI["ext/dstd_gcn_eval.h"]) == 1
    assert set(abi.ABI) == {"dstd_gcn.h", "dstd_gcn_train.h", "dstd_gcn_aux.h", "dstd_gcn_loss.h", "dstd_gcn_taps.h",
                            "dstd_gcn_data.h", "dstd_gcn_predict.h"}
    assert sum(len(t) for t in abi.ABI.values()) == 61 and len(abi.C_TYPES) == 15
    assert not any(NAME in t for t in (*abi.ABI.values(), *native.ext.ALL.values(), *native.ext_eval.ABI.values()))
    assert native.ext_augment.seq_store_ref is native.ext_eval.seq_store_ref
    mk = open(os.path.join(ROOT, "dstd-gcn_amd", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "csrc/dstd_augment.hip" in srcs and "csrc/dstd_data.hip" in srcs
    assert L.dstd_source_hash().decode() == native.source_hash()  # the new sources are hashed


def test_a_library_without_the_symbol_is_a_load_error():
    class Lib:
        _name = "libold.so"

        def __getattr__(self, name):
            if name == NAME:
                raise AttributeError(name)
            return type("Fn", (), {})()

    extra = {**native.ext.ALL, **native.ext_eval.ABI, **native.ext_augment.ABI}
    with pytest.raises(RuntimeError, match=NAME):
        native.declare(Lib(), extra=extra)
    native.declare(Lib(), allow_missing=True, extra=extra)


# ---- refusals of the entry point ----------------------------------------------------
def _store(**kw):
    """A well-formed H36M store; the pointers are never dereferenced on the host."""
    f = dict(frames=0x1000, used=None, starts=0x2000, F=1000, N=900, T=35, D=96, Du=66, dim_used=0x3000,
             frame_in=0x4000, frame_inv=0x5000, mirror_src=None)
    f.update(kw)
    return native.SeqStore(**f)


def _call(store, **kw):
    a = dict(index=0x6000, B=4, xf=0x7000, noise_amp=0.5, seed=7, inputs=0x8000, inputs_inv=0x9000, targets=0xA000,
             all_seqs=0xB000)
    a.update(kw)
    ref = native.ext_augment.seq_store_ref(store) if store is not None else None
    return native.lib().dstd_batch_gather_aug(ref, a["index"], a["B"], a["xf"], a["noise_amp"], a["seed"],
                                              a["inputs"], a["inputs_inv"], a["targets"], a["all_seqs"], None)


BAD_STORES = {"null frames": dict(frames=None), "null starts": dict(starts=None), "null dim_used": dict(dim_used=None),
              "null frame_in": dict(frame_in=None), "null frame_inv": dict(frame_inv=None), "T = 0": dict(T=0),
              "T < 0": dict(T=-1), "F = 0": dict(F=0), "N = 0": dict(N=0), "D % 3 = 1": dict(D=97),
              "D % 3 = 2": dict(D=98), "Du = 0": dict(Du=0), "Du > D": dict(Du=97),
              "used and mirror_src": dict(used=0xC000, mirror_src=0xD000)}
BAD_ARGS = {"null index": dict(index=None), "B = 0": dict(B=0), "B < 0": dict(B=-1),
            "all outputs null": dict(inputs=None, inputs_inv=None, targets=None, all_seqs=None),
            "noise < 0": dict(noise_amp=-1e-30), "noise = -1": dict(noise_amp=-1.0),
            "noise = inf": dict(noise_amp=float("inf")), "noise = -inf": dict(noise_amp=float("-inf")),
            "noise = nan": dict(noise_amp=float("nan"))}


@pytest.mark.parametrize("what", list(BAD_STORES))
def test_bad_store_is_einval_before_any_gpu_work(what):
    for xf in (0x7000, None):
        assert _call(_store(**BAD_STORES[what]), xf=xf) == EINVAL


@pytest.mark.parametrize("what", list(BAD_ARGS))
def test_bad_argument_is_einval_before_any_gpu_work(what):
    for xf in (0x7000, None):
        assert _call(_store(), xf=xf, **BAD_ARGS[what]) == EINVAL


def test_null_store_and_a_transform_of_a_scaled_set_before_any_gpu_work():
    assert _call(None) == EINVAL
    assert native.lib().dstd_batch_gather_aug(None, None, 0, None, 0.0, 0, None, None, None, None, None) == EINVAL
    assert _call(_store(used=0xC000)) == EINVAL  # xf together with used
    assert _call(_store(used=0xC000), noise_amp=0.0) == EINVAL
    with pytest.raises(TypeError, match="SeqStore"):
        native.ext_augment.seq_store_ref(object())


# ---- Augment.draw ---------------------------------------------------------------------
def _draw(aug, B, seed=5):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    m = aug.draw(B, g, "cpu")
    assert m.dtype == torch.float32 and tuple(m.shape) == (B, 12) and m.is_contiguous() and m.device.type == "cpu"
    m = m.numpy().astype(np.float64).reshape(B, 3, 4)
    return m[:, :, :3], m[:, :, 3]


def _orthogonality(Am, s2):
    """max over the batch of |A A^T - s^2 I| / s^2, in fp64 on the fp32 entries."""
    dev = np.einsum("bik,bjk->bij", Am, Am) - s2[:, None, None] * np.eye(3)
    return float((np.abs(dev).max(axis=(1, 2)) / s2).max())


@pytest.mark.parametrize("B", [1, 1000])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_draw_single_axis_rotation_with_scale_and_shift(B, axis):
    max_angle, lo, hi, shift = 2.5, 0.75, 1.25, 30.0
    Am, t = _draw(Augment(rotate=(axis, max_angle), scale=(lo, hi), shift=shift), B)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    s = Am[:, axis, axis]  # the scale as drawn: 1 * s is exact
    # the axis row and column are exact: s on the diagonal, true zeros elsewhere
    for k in (i, j):
        assert not Am[:, axis, k].any() and not Am[:, k, axis].any()
    assert (s >= np.float32(lo)).all() and (s <= np.float32(hi)).all()
    # the issue's bound: a scaled single-axis rotation is (cos, sin) to an ulp,
    # one product with s each, and A A^T sums two squares of them
    assert _orthogonality(Am, s * s) <= 16 * U
    assert (np.linalg.det(Am) > 0).all()
    theta = np.arctan2(Am[:, j, i], Am[:, i, i])  # right-handed about `axis`
    assert np.abs(theta).max() <= max_angle * (1 + 8 * U)  # the recovered angle carries the entries' rounding
    assert np.array_equal(Am[:, i, j], -Am[:, j, i]) and np.array_equal(Am[:, i, i], Am[:, j, j])
    assert np.abs(t).max() <= shift
    if B == 1000:  # the ranges are used, not only respected
        assert theta.min() < -0.9 * max_angle and theta.max() > 0.9 * max_angle
        assert s.min() < lo + 0.05 * (hi - lo) and s.max() > hi - 0.05 * (hi - lo)
        assert t.min() < -0.9 * shift and t.max() > 0.9 * shift and np.abs(t.mean(0)).max() < 0.15 * shift


@pytest.mark.parametrize("B", [1, 1000])
def test_draw_so3(B):
    """Bound of this construction.  q = g / |g|: |q|^2 = 1 + d with |d| <= 10u
    (the sum of four squares, the root and the quotient: each component is off
    by at most 5u relative).  The homogeneous matrix of q is |q|^2 times a
    rotation, so R R^T = (1 + d)^2 I: off by 2|d| <= 20u.  Each entry is two to
    four products summed, |error| <= 4u |q|^2; through R R^T that is at most
    2 * 4u * sum_k |R_ik| <= 8 sqrt(3) u < 14u.  The scale's one product per
    entry adds 2u relative: 36u, and 40u is asserted."""
    Am, t = _draw(Augment(rotate="so3"), B)
    assert not t.any()
    assert _orthogonality(Am, np.ones(B)) <= 40 * U
    assert (np.linalg.det(Am) > 0).all()
    Am, _ = _draw(Augment(rotate="so3", scale=(0.5, 2.0)), B)
    s2 = np.einsum("bik,bik->b", Am, Am) / 3  # trace(A A^T) / 3
    assert _orthogonality(Am, s2) <= 40 * U
    assert (np.linalg.det(Am) > 0).all()
    s = np.sqrt(s2)
    assert s.min() >= 0.5 * (1 - 40 * U) and s.max() <= 2.0 * (1 + 40 * U)
    if B == 1000:  # uniform on SO(3): every entry has mean 0 and variance 1/3
        R, _ = _draw(Augment(rotate="so3"), B)
        assert np.abs(R.mean(0)).max() < 0.08 and np.abs((R * R).mean(0) - 1 / 3).max() < 0.05


def test_draw_parts_alone_reproducibility_and_nothing_configured():
    Am, t = _draw(Augment(scale=(1.5, 1.5)), 4)
    assert np.array_equal(Am, np.broadcast_to(1.5 * np.eye(3), (4, 3, 3))) and not t.any()
    Am, t = _draw(Augment(shift=2.0), 4)
    assert np.array_equal(Am, np.broadcast_to(np.eye(3), (4, 3, 3))) and t.any() and np.abs(t).max() <= 2.0
    Am, t = _draw(Augment(rotate=(2, 0.0)), 4)
    assert np.array_equal(Am, np.broadcast_to(np.eye(3), (4, 3, 3)))
    aug = Augment(rotate=(1, 3.0), scale=(0.9, 1.1), shift=1.0, noise=2.0)
    a, b, c = _draw(aug, 7, seed=3), _draw(aug, 7, seed=3), _draw(aug, 7, seed=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[0], c[0])
    g = torch.Generator(device="cpu")
    assert Augment().draw(5, g, "cpu") is None and Augment(noise=3.0).draw(5, g, "cpu") is None
    assert Augment(noise=3.0).noise == 3.0


@pytest.mark.parametrize("bad", [dict(rotate=(3, 1.0)), dict(rotate=(-1, 1.0)), dict(rotate=1.0), dict(rotate="z"),
                                 dict(rotate=(1, -0.1)), dict(rotate=(1, float("nan"))), dict(scale=(0.0, 1.0)),
                                 dict(scale=(1.1, 0.9)), dict(scale=1.0), dict(scale=(1.0, float("inf"))),
                                 dict(shift=-1.0), dict(shift=float("nan")), dict(noise=-1.0),
                                 dict(noise=float("inf")), dict(noise=float("nan"))])
def test_augment_refuses_parameters_outside_their_ranges(bad):
    with pytest.raises(ValueError, match=next(iter(bad))):
        Augment(**bad)


# ---- DeviceLoader and DeviceSequences.gather --------------------------------------------------
def _windows(n=5, t=4, d=6, seed=0):
    return np.random.default_rng(seed).normal(size=(n, t, d))


def test_index_batches_are_the_same_with_and_without_augment():
    s = DeviceSequences.from_windows(_windows(), [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]))
    aug = Augment(rotate=(1, 3.0), noise=1.0)
    for shuffle in (False, True):
        plain = DeviceLoader(s, 3, shuffle=shuffle, seed=11)
        augm = DeviceLoader(s, 3, shuffle=shuffle, seed=11, augment=aug)
        assert augm.augment is aug and plain.augment is None
        for _ in range(2):  # two epochs
            a, b = [i.tolist() for i in plain.index_batches()], [i.tolist() for i in augm.index_batches()]
            assert a == b and sorted(sum(a, [])) == list(range(10))
        assert plain.epoch == augm.epoch == 2
    assert augm.last_transform is None and augm.last_noise_seed is None
    with pytest.raises(TypeError, match="augment"):
        DeviceLoader(s, 3, augment=dict(noise=1.0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the augmenting iteration goes on to the device
        next(iter(augm))


def test_noise_seed_formula_on_python_ints():
    f = DeviceLoader.noise_seed
    assert f(0, 0, 0) == 0 and f(0, 0, 5) == 5 and f(3, 2, 7) == (5 << 32) | 7
    assert f(1, 0, 1 << 32) == 0  # the batch counter is xor-ed, not added
    assert f(2 ** 32 - 1, 1, 3) == 3  # (2^32 << 32) mod 2^64
    assert f(-1, 0, 0) == 2 ** 64 - 2 ** 32 and f(-1, 0, 1) == 2 ** 64 - 2 ** 32 + 1
    for seed, epoch, i in ((12345, 6, 789), (2 ** 40 + 3, 9, 2 ** 20)):
        assert f(seed, epoch, i) == (((seed + epoch) << 32) ^ i) % 2 ** 64 and 0 <= f(seed, epoch, i) < 2 ** 64


def test_gather_refuses_bad_augmentation_arguments_before_any_gpu_work():
    s = DeviceSequences.from_windows(_windows(), [0, 1, 2], 2, 2, device="cpu")
    idx = torch.arange(3)
    good = torch.zeros(3, 12)
    for bad in (torch.zeros(3, 11), torch.zeros(2, 12), torch.zeros(3, 4, 3), torch.zeros(36),
                torch.zeros(3, 12).double(), torch.zeros(12, 3).t(), np.zeros((3, 12), dtype=np.float32),
                torch.zeros(3, 12, device="meta")):
        with pytest.raises(ValueError, match="transform"):
            s.gather(idx, transform=bad)
    for bad in (-1.0, float("nan"), float("inf"), -1e-300, 1e39, "much"):
        with pytest.raises(ValueError, match="noise"):
            s.gather(idx, noise=bad)
        with pytest.raises(ValueError, match="noise"):
            s.gather(idx, transform=good, noise=bad)
    scaled = DeviceSequences.from_windows(_windows(), [0, 1, 2], 2, 2, device="cpu", scaler=True)
    with pytest.raises(ValueError, match="scaled"):
        scaled.gather(idx, transform=good)
    # valid arguments go on to the device: there is no CPU gather
    for kw in (dict(transform=good), dict(transform=good.view(3, 3, 4), noise=1.0), dict(noise=0.5, noise_seed=-3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            s.gather(idx, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scaled.gather(idx, noise=0.5)


class _Log:
    def info(self, *a, **k):
        pass


def test_test_groups_refuses_an_augmenting_loader():
    from engine.prediction import PredictionEngine
    from model import get_model
    opts = dict(input_channels=6, input_time_frame=2, output_time_frame=2, st_gcnn_dropout=0.1, joints_to_consider=22,
                num_feature=8, num_layers=1, layout="h36m")
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5), loss=dict(joint=["jl2", 1]),
               n_out=1, transform="tsc", use_weight=False, inverse=True)
    eng = PredictionEngine(cfg, get_model("dstdgcn", dstdgcn=opts), _Log())
    s = DeviceSequences.from_windows(_windows(3, 4, 96), list(range(66)), 2, 2, device="cpu", groups=[0, 1, 1])
    with pytest.raises(ValueError, match="augment"):
        eng.test_groups(DeviceLoader(s, 2, augment=Augment(noise=1.0)), input_n=2, eval_frame=[0, 1])


# ---- the restatement itself ---------------------------------------------------------------
def _store_case(padding=True, mirror=True, seed=3):
    """A small host store: 4 windows of 5 frames, 4 joints, dim_used taking
    single columns of joints."""
    from dstd_data import frame_maps
    rng = np.random.default_rng(seed)
    frames = (rng.normal(size=(20, 12)) * 100).astype(np.float32)
    frames[3, 4] = -0.0
    fwd, inv = frame_maps(2, 3, padding)
    return H.store_arrays(frames, np.arange(4) * 5, 5, [1, 3, 5, 8, 9, 10], fwd, inv,
                          mirror_src=[1, 0, 2, 3] if mirror else None)


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("padding", [False, True])
def test_restatement_without_augmentation_is_expected_batch_in_bits(padding, mirror):
    s = _store_case(padding, mirror)
    idx = [3, 0, 5 if mirror else 1, -1, 2, 2]
    want = H.expected_batch(s, idx)
    for got in (A.expected_aug(s, idx), A.expected_aug(s, idx, None, 0.0, seed=9)):
        for g, w in zip(got, want):
            assert np.array_equal(H.bits(g), H.bits(w))
    assert (H.bits(want[3]) == np.int32(-2 ** 31)).any()  # the -0.0 is in the batch and survives
    # the identity and zero noise: equal in value (-0.0 becomes +0.0 through "+ 0")
    ident = np.tile(np.eye(3, 4, dtype=np.float32).reshape(12), (len(idx), 1))
    for g, w in zip(A.expected_aug(s, idx, ident), want):
        assert np.array_equal(g, w, equal_nan=True)
    with pytest.raises(ValueError, match="scaled"):
        A.expected_aug(dict(s, mirror_src=None, used=s["frames"][:, :6]), idx, ident)


def test_restated_transform_is_the_fp64_affine_map_to_fp32_rounding():
    s = _store_case()
    idx = [0, 6, 3]
    xf = A.random_transforms(3, seed=1)
    got = A.expected_aug(s, idx, xf)
    clean = H.expected_batch(s, idx)
    p = clean[3].astype(np.float64).reshape(3, 5, 4, 3)
    m = xf.astype(np.float64).reshape(3, 3, 4)
    ref = np.einsum("bck,btjk->btjc", m[:, :, :3], p) + m[:, None, None, :, 3]
    mag = np.einsum("bck,btjk->btjc", np.abs(m[:, :, :3]), np.abs(p)) + np.abs(m[:, None, None, :, 3])
    assert (np.abs(got[3].reshape(3, 5, 4, 3) - ref) <= 4.01 * U * mag).all()  # a value passes at most four roundings
    assert np.array_equal(got[3][1], clean[3][1]) and not got[3][2].any()  # the identity row, the zero row
    assert np.array_equal(H.bits(got[2]), H.bits(got[3][:, :, s["dim_used"]]))
    assert np.array_equal(H.bits(got[0]), H.bits(got[2][:, s["frame_in"]]))
    assert np.array_equal(H.bits(got[1]), H.bits(got[2][:, s["frame_inv"]]))


def test_restated_noise_padded_rows_shared_frames_and_statistics():
    s = _store_case(padding=True)
    idx = [2, 6, 2]  # window 2, its mirrored twin, window 2 again
    amp = 2.0
    xf = A.random_transforms(3)
    xf[2] = xf[0]  # the duplicated window under the same transform
    clean = A.expected_aug(s, idx, xf)
    got = A.expected_aug(s, idx, xf, amp, seed=77)
    for k in (2, 3):  # targets and all_seqs stay clean
        assert np.array_equal(H.bits(got[k]), H.bits(clean[k]))
    n_in, n_inv = got[0] - clean[0], got[1] - clean[1]
    assert np.abs(n_in).max() <= amp * (1 + 4 * U) + 1e-4 and n_in.any()  # (clean + n) - clean, to the sum's rounding
    # padded rows repeat frame input_n - 1 = 1 (inputs) / frame output_n = 3 (inputs_inv): identical copies
    assert s["frame_in"].tolist() == [0, 1, 1, 1, 1] and s["frame_inv"].tolist() == [4, 3, 3, 3, 3]
    for r in (2, 3, 4):
        assert np.array_equal(H.bits(got[0][:, r]), H.bits(got[0][:, 1]))
        assert np.array_equal(H.bits(got[1][:, r]), H.bits(got[1][:, 1]))
    # keyed by the index value: the duplicate equals, the mirrored twin has noise of its own
    assert np.array_equal(H.bits(got[0][0]), H.bits(got[0][2]))
    j = A.jitter(77, 2, 5, [0, 1, 3, 4], 6, amp)
    assert not np.array_equal(j, A.jitter(77, 6, 5, [0, 1, 3, 4], 6, amp))
    assert not np.array_equal(j, A.jitter(78, 2, 5, [0, 1, 3, 4], 6, amp))
    # a frame seen by both tensors carries the same noise in both (no padding: every frame is shared)
    s2 = _store_case(padding=False)
    c2, g2 = A.expected_aug(s2, idx), A.expected_aug(s2, idx, None, amp, seed=77)
    assert np.array_equal(H.bits(g2[0]), H.bits(g2[1][:, ::-1]))
    assert np.array_equal(H.bits(g2[0][0]), H.bits(c2[0][0] + A.jitter(77, 2, 5, np.arange(5), 6, amp)))
    # the uniform itself: 24 bits in [0, 1), n = amp * (2u - 1) in [-amp, amp)
    big = A.jitter(1, 0, 1000, np.arange(1000), 66, 1.0)
    assert big.dtype == np.float32 and big.min() >= -1.0 and big.max() < 1.0
    assert abs(float(big.mean())) < 0.01 and abs(float(big.var()) - 1 / 3) < 0.01
    assert np.array_equal(big * np.float32(2 ** 23), np.round(big * np.float32(2 ** 23)))  # multiples of 2^-23


def test_mix64_is_the_splitmix64_finaliser():
    def ref(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
        return z ^ (z >> 31)

    zs = [0, 1, 2 ** 64 - 1, 0x9E3779B97F4A7C15, 123456789012345678]
    assert A.mix64(np.array(zs, dtype=np.uint64)).tolist() == [ref(z) for z in zs]
    # the key of the header on Python ints, for one element
    seed, w, T, f, Du, k = 2 ** 63 + 5, 7, 35, 9, 66, 65
    h = ref((seed * 0x9E3779B97F4A7C15 + ((w * T + f) * Du + k)) % 2 ** 64)
    n = np.float32(1.5) * (np.float32(2) * (np.float32(h >> 40) * np.float32(2.0 ** -24)) - np.float32(1))
    assert A.jitter(seed, w, T, [f], Du, 1.5)[0, k] == n
