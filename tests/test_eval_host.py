"""Host-side checks of grouped evaluation (include/ext/dstd_gcn_eval.h,
dstd_native.ext_eval, the groups of dstd_data.DeviceSequences and the table
arithmetic of PredictionEngine.test_groups).  No GPU needed: the entry point's
refusals come before any HIP call, and sets are built with device="cpu"."""
import ctypes
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import dstd_native as native
from abi_reader import compare, parse
from conftest import ROOT
from dstd_data import DeviceLoader, DeviceSequences, MeanStd, group_table
from dstd_native import abi
from engine.prediction import PredictionEngine, combine_groups

EINVAL, ELIMIT = -1, -3  # include/dstd_gcn.h
HEADER = "ext/dstd_gcn_eval.h"
NAME = "dstd_store_group_mpjpe"


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", *HEADER.split("/"))).read()


# ---- the binding -----------------------------------------------------------------
def test_binding_agrees_with_the_eval_header(header):
    assert compare({HEADER: header}, native.ext_eval) == []
    defines, structs, callbacks, protos = parse(header)
    assert list(protos) == [NAME] and native.ext_eval.EVAL_EXPORTS == (NAME,)
    (ret, params) = protos[NAME]
    assert ret == ("int", 0) and len(params) == 15
    assert [p[2] for p in params] == ["s", "index", "B", "outputs", "t_out0", "used_pos", "n_used", "joint_src",
                                      "frames", "n_frames", "group", "n_groups", "sums", "counts", "stream"]
    assert [(p[0], p[1]) for p in params] == [
        ("dstd_seq_store", 1), ("long long", 1), ("int", 0), ("float", 1), ("int", 0), ("int", 1), ("int", 0),
        ("int", 1), ("int", 1), ("int", 0), ("int", 1), ("int", 0), ("float", 1), ("int", 1), ("void", 1)]
    i, p = ctypes.c_int, ctypes.c_void_p
    assert native.ext_eval.ABI == {HEADER: {NAME: (i, [p, p, i, p, i, p, i, p, p, i, p, i, p, p, p])}}
    assert defines == {"DSTD_EVAL_MAX_GROUPS": "1024"} and native.ext_eval.EVAL_MAX_GROUPS == 1024
    assert (structs, callbacks) == ({}, {}) and native.ext_eval.C_TYPES == {}


def test_an_altered_eval_header_is_reported_by_name(header):
    for old, new in (("const int* group, ", ""), ("int n_groups", "size_t n_groups")):
        assert old in header
        reports = compare({HEADER: header.replace(old, new, 1)}, native.ext_eval)
        assert {r.split(":")[0] for r in reports} == {NAME}, reports
    reports = compare({HEADER: header.replace("MAX_GROUPS 1024", "MAX_GROUPS 512")}, native.ext_eval)
    assert {r.split(":")[0] for r in reports} == {"DSTD_EVAL_MAX_GROUPS"}, reports


def test_library_exports_the_entry_point_and_the_other_tables_are_as_they_were():
    L = native.lib()
    restype, argtypes = native.ext_eval.ABI[HEADER][NAME]
    fn = getattr(L, NAME)  # exported, and declared by lib()
    assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # a table of its own: nothing added to the pinned ones
    assert set(native.ext.ALL) == {"ext/dstd_gcn_rollout.h", "ext/dstd_gcn_teacher.h"}
    assert sum(len(t) for t in native.ext.ALL.values()) == 10
    assert set(native.ext.ABI) == {"ext/dstd_gcn_rollout.h"} and len(native.ext.ABI["ext/dstd_gcn_rollout.h"]) == 6
    assert set(abi.ABI) == {"dstd_gcn.h", "dstd_gcn_train.h", "dstd_gcn_aux.h", "dstd_gcn_loss.h", "dstd_gcn_taps.h",
                            "dstd_gcn_data.h", "dstd_gcn_predict.h"}
    assert sum(len(t) for t in abi.ABI.values()) == 61 and len(abi.C_TYPES) == 15
    assert not any(NAME in t for t in (*abi.ABI.values(), *native.ext.ALL.values()))
    assert not hasattr(native.ext, "EVAL_EXPORTS")
    mk = open(os.path.join(ROOT, "dstd-gcn_amd", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "csrc/dstd_eval.hip" in srcs
    assert L.dstd_source_hash().decode() == native.source_hash()  # the new sources are hashed


def test_a_library_without_the_symbol_is_a_load_error():
    class Lib:
        _name = "libold.so"

        def __getattr__(self, name):
            if name == NAME:
                raise AttributeError(name)
            return type("Fn", (), {})()

    with pytest.raises(RuntimeError, match=NAME):
        native.declare(Lib(), extra={**native.ext.ALL, **native.ext_eval.ABI})
    native.declare(Lib(), allow_missing=True, extra={**native.ext.ALL, **native.ext_eval.ABI})
    with pytest.raises(TypeError, match="SeqStore"):
        native.ext_eval.seq_store_ref(object())


# ---- refusals of the entry point ----------------------------------------------------
def _store(**kw):
    """A well-formed H36M store; the pointers are never dereferenced on the host."""
    f = dict(frames=0x1000, used=None, starts=0x2000, F=1000, N=900, T=35, D=96, Du=66, dim_used=0x3000,
             frame_in=0x4000, frame_inv=0x5000, mirror_src=None)
    f.update(kw)
    return native.SeqStore(**f)


def _call(store, **kw):
    a = dict(index=0x6000, B=4, outputs=0x7000, t_out0=10, used_pos=0x8000, n_used=66, joint_src=0x9000,
             frames=0xA000, n_frames=4, group=0xB000, n_groups=15, sums=0xC000, counts=0xD000)
    a.update(kw)
    ref = native.ext_eval.seq_store_ref(store) if store is not None else None
    return native.lib().dstd_store_group_mpjpe(ref, a["index"], a["B"], a["outputs"], a["t_out0"], a["used_pos"],
                                               a["n_used"], a["joint_src"], a["frames"], a["n_frames"], a["group"],
                                               a["n_groups"], a["sums"], a["counts"], None)


BAD_STORES = {"null frames": dict(frames=None), "null starts": dict(starts=None), "T = 0": dict(T=0),
              "T < 0": dict(T=-1), "D % 3 = 1": dict(D=97), "D % 3 = 2": dict(D=98), "D = 0": dict(D=0),
              "F = 0": dict(F=0), "N = 0": dict(N=0)}
BAD_ARGS = {"null index": dict(index=None), "null outputs": dict(outputs=None), "null used_pos": dict(used_pos=None),
            "null joint_src": dict(joint_src=None), "null frames": dict(frames=None), "null sums": dict(sums=None),
            "null counts": dict(counts=None), "B = 0": dict(B=0), "B < 0": dict(B=-1), "n_frames = 0": dict(n_frames=0),
            "n_frames < 0": dict(n_frames=-2), "n_groups = 0": dict(n_groups=0), "n_groups < 0": dict(n_groups=-1),
            "n_used = 0": dict(n_used=0), "n_used < 0": dict(n_used=-66), "t_out0 < 0": dict(t_out0=-1),
            "t_out0 = T": dict(t_out0=35), "t_out0 > T": dict(t_out0=36)}


@pytest.mark.parametrize("what", list(BAD_STORES))
def test_bad_store_is_einval_before_any_gpu_work(what):
    assert _call(_store(**BAD_STORES[what])) == EINVAL


@pytest.mark.parametrize("what", list(BAD_ARGS))
def test_bad_argument_is_einval_before_any_gpu_work(what):
    assert _call(_store(), **BAD_ARGS[what]) == EINVAL


def test_null_store_and_group_limit_before_any_gpu_work():
    """The checks come before any HIP call (this test runs on machines without
    a device): a NULL store is DSTD_EINVAL, more than DSTD_EVAL_MAX_GROUPS
    groups DSTD_ELIMIT, and an argument error wins over the limit."""
    assert _call(None) == EINVAL
    assert native.lib().dstd_store_group_mpjpe(None, None, 0, None, 0, None, 0, None, None, 0, None, 0, None, None,
                                               None) == EINVAL
    assert _call(_store(), n_groups=native.ext_eval.EVAL_MAX_GROUPS + 1) == ELIMIT
    assert _call(_store(), n_groups=native.ext_eval.EVAL_MAX_GROUPS + 1, group=None) == ELIMIT
    assert _call(_store(), n_groups=native.ext_eval.EVAL_MAX_GROUPS + 1, sums=None) == EINVAL
    assert _call(_store(D=3 * (1 << 20)), B=1 << 11) == ELIMIT  # B * J does not fit the kernel's int loop


# ---- groups of a resident set -------------------------------------------------------
def _windows(n=3, t=4, d=6, seed=0):
    return np.random.default_rng(seed).normal(size=(n, t, d))


def test_group_table_and_default_names():
    table, names = group_table([2, 0, 2], 3)
    assert table.dtype == np.int32 and table.tolist() == [2, 0, 2] and names == ["0", "1", "2"]
    table, names = group_table(np.array([1, 0]), 2, mirrored=True, group_names=["walk", "eat"])
    assert table.tolist() == [1, 0, 1, 0] and names == ["walk", "eat"]
    for bad in ([0, 1], [0, 1, 2, 0], [0.0, 1.0, 2.0], [[0, 1, 2]], [0, -1, 1]):
        with pytest.raises(ValueError, match="groups"):
            group_table(bad, 3)
    for bad in (["a"], ["a", "b", "c"], ["a", "a"], ["a", 1]):
        with pytest.raises(ValueError, match="group_names"):
            group_table([0, 1, 1], 3, group_names=bad)


def test_a_set_without_groups_is_unchanged():
    x = _windows()
    s = DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]))
    assert s.groups is None and s.group_names == ["all"] and s.n_groups == 1
    g = DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]), groups=[0, 0, 1])
    assert g.nbytes == s.nbytes + 4 * 6 and len(g) == len(s) == 6
    assert torch.equal(g._frames, s._frames) and torch.equal(g._starts, s._starts)
    assert list(DeviceLoader(g, 4).index_batches())[1].tolist() == [4, 5]
    with pytest.raises(ValueError, match="group_names without groups"):
        DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu", group_names=["a"])


def test_from_windows_groups_and_the_mirrored_half():
    x = _windows()
    s = DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]), groups=[2, 0, 2])
    assert s.groups.dtype == torch.int32 and s.groups.tolist() == [2, 0, 2, 2, 0, 2]  # window w + N: the group of w
    assert s.group_names == ["0", "1", "2"] and s.n_groups == 3
    # a scaled set stores its mirrored frames: the groups are doubled with them
    sc = DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]), scaler=True,
                                      groups=[1, 0, 1], group_names=["a", "b"])
    assert sc._mirror_src is None and sc.n_windows == 6 and sc.groups.tolist() == [1, 0, 1, 1, 0, 1]
    assert sc.group_names == ["a", "b"]
    plain = DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu", groups=np.array([0, 1, 1]))
    assert plain.groups.tolist() == [0, 1, 1]
    for bad in ([0, 1], [0, 1, 1, 0, 1, 1]):
        with pytest.raises(ValueError, match="groups"):
            DeviceSequences.from_windows(x, [0, 1, 2], 2, 2, device="cpu", mirror=([0], [1]), groups=bad)


def test_from_sequences_windows_inherit_the_group_of_their_sequence():
    rng = np.random.default_rng(1)
    seqs = [rng.normal(size=(f, 6)) for f in (5, 3, 4)]
    s = DeviceSequences.from_sequences(seqs, 3, [0, 1, 2], 1, 2, device="cpu", groups=[1, 0, 1], group_names=["a", "b"])
    assert s.n_windows == 3 + 1 + 2 and s.groups.tolist() == [1, 1, 1, 0, 1, 1]
    m = DeviceSequences.from_sequences(seqs, 3, [0, 1, 2], 1, 2, device="cpu", groups=[1, 0, 1], mirror=([0], [1]))
    assert m.groups.tolist() == [1, 1, 1, 0, 1, 1] * 2 and len(m) == 12
    sc = DeviceSequences.from_sequences(seqs, 3, [0, 1, 2], 1, 2, device="cpu", groups=[1, 0, 1], mirror=([0], [1]),
                                        scaler=(np.zeros(3), np.ones(3)))
    assert sc.n_windows == 12 and sc.groups.tolist() == [1, 1, 1, 0, 1, 1] * 2
    with pytest.raises(ValueError, match="groups"):
        DeviceSequences.from_sequences(seqs, 3, [0, 1, 2], 1, 2, device="cpu", groups=[1, 0])
    assert DeviceSequences.from_sequences(seqs, 3, [0, 1, 2], 1, 2, device="cpu").groups is None


class _Dataset:
    def __init__(self, all_seqs, dim_used, scale_tsfm=None):
        self.all_seqs, self.dim_used = all_seqs, np.asarray(dim_used)
        if scale_tsfm is not None:
            self.scale_tsfm = scale_tsfm


def test_from_datasets_concatenates_in_mapping_order():
    a, b, c = _windows(2, 4, 6, 1), _windows(1, 4, 6, 2), _windows(3, 4, 6, 3)
    sets = OrderedDict([("walking", _Dataset(a, [0, 1, 2])), ("eating", _Dataset(b, [0, 1, 2])),
                        ("smoking", _Dataset(c, [0, 1, 2]))])
    s = DeviceSequences.from_datasets(sets, 2, 2, device="cpu")
    assert s.group_names == ["walking", "eating", "smoking"] and s.n_groups == 3
    assert s.groups.tolist() == [0, 0, 1, 2, 2, 2] and len(s) == 6
    want = np.concatenate([a, b, c]).reshape(24, 6).astype(np.float32)
    assert np.array_equal(s._frames.numpy(), want) and s._starts.tolist() == [0, 4, 8, 12, 16, 20]
    assert s.joint_weight_use is None and s.joint_weight_all is None and s.scale_tsfm is None
    assert s.seq_len == 4 and (s.input_n, s.output_n) == (2, 2)
    # the other order is the other set
    r = DeviceSequences.from_datasets(OrderedDict(reversed(list(sets.items()))), 2, 2, device="cpu")
    assert r.group_names == ["smoking", "eating", "walking"] and r.groups.tolist() == [0, 0, 0, 1, 2, 2]
    # one shared scale transform: taken from the first entry, equal statistics accepted
    st = [MeanStd(np.arange(3.0), np.ones(3) * 2) for _ in range(2)]
    sc = DeviceSequences.from_datasets({"x": _Dataset(a, [0, 1, 2], st[0]), "y": _Dataset(b, [0, 1, 2], st[1])}, 2, 2,
                                       device="cpu")
    assert sc.scale_tsfm is st[0] and sc._used is not None and sc.groups.tolist() == [0, 0, 1]


def test_from_datasets_refuses_sets_that_do_not_agree():
    a, b = _windows(2, 4, 6, 1), _windows(1, 4, 6, 2)
    with pytest.raises(ValueError, match="dim_used"):
        DeviceSequences.from_datasets({"x": _Dataset(a, [0, 1, 2]), "y": _Dataset(b, [0, 1, 3])}, 2, 2, device="cpu")
    with pytest.raises(ValueError, match="all_seqs"):  # window length
        DeviceSequences.from_datasets({"x": _Dataset(a, [0, 1, 2]), "y": _Dataset(_windows(1, 5, 6), [0, 1, 2])}, 2, 2,
                                      device="cpu")
    with pytest.raises(ValueError, match="all_seqs"):  # D
        DeviceSequences.from_datasets({"x": _Dataset(a, [0, 1, 2]), "y": _Dataset(_windows(1, 4, 9), [0, 1, 2])}, 2, 2,
                                      device="cpu")
    st = MeanStd(np.arange(3.0), np.ones(3))
    with pytest.raises(ValueError, match="scale_tsfm"):
        DeviceSequences.from_datasets({"x": _Dataset(a, [0, 1, 2], st),
                                       "y": _Dataset(b, [0, 1, 2], MeanStd(np.arange(3.0), np.ones(3) * 2))}, 2, 2,
                                      device="cpu")
    with pytest.raises(ValueError, match="scale_tsfm"):
        DeviceSequences.from_datasets({"x": _Dataset(a, [0, 1, 2], st), "y": _Dataset(b, [0, 1, 2])}, 2, 2,
                                      device="cpu")
    with pytest.raises(ValueError, match="no dataset"):
        DeviceSequences.from_datasets({}, 2, 2, device="cpu")


# ---- the table arithmetic -----------------------------------------------------------
def test_combine_groups_leaves_empty_groups_out_and_averages_the_rest():
    sums = np.array([[3.0, 6.0], [0.0, 0.0], [10.0, 30.0]])
    counts = np.array([3, 0, 5])
    avg, t_metric, table = combine_groups(sums, counts)
    assert list(table) == [0, 2]  # group order, the empty one left out
    assert np.array_equal(table[0][1], [1.0, 2.0]) and table[0][0] == 1.5
    assert np.array_equal(table[2][1], [2.0, 6.0]) and table[2][0] == 4.0
    assert np.array_equal(t_metric, [1.5, 4.0])  # unweighted over the non-empty groups, not over the 8 windows
    assert avg == 2.75 == np.mean([table[0][0], table[2][0]])
    avg1, t1, table1 = combine_groups(sums[:1], counts[:1])
    assert avg1 == 1.5 and np.array_equal(t1, [1.0, 2.0]) and list(table1) == [0]
    with pytest.raises(ValueError, match="empty"):
        combine_groups(np.zeros((2, 3)), np.zeros(2, dtype=np.int64))
    with pytest.raises(ValueError, match="sums"):
        combine_groups(np.zeros(3), np.zeros(3))


# ---- refusals of the engine method that need no device ---------------------------------
class _Log:
    def info(self, *a, **k):
        pass


def test_test_groups_refusals_before_any_gpu_work():
    from model import get_model
    opts = dict(input_channels=6, input_time_frame=2, output_time_frame=2, st_gcnn_dropout=0.1, joints_to_consider=22,
                num_feature=8, num_layers=1, layout="h36m")
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5), loss=dict(joint=["jl2", 1]),
               n_out=1, transform="tsc", use_weight=False, inverse=True)
    eng = PredictionEngine(cfg, get_model("dstdgcn", dstdgcn=opts), _Log())
    x = _windows(3, 4, 96)
    s = DeviceSequences.from_windows(x, list(range(66)), 2, 2, device="cpu", groups=[0, 1, 1])
    loader = DeviceLoader(s, 2)
    with pytest.raises(TypeError, match="DeviceLoader"):
        eng.test_groups([(None, None, None, None)], input_n=2, eval_frame=[0])
    with pytest.raises(ValueError, match="frames"):  # windows of 4 frames, not 2 + 5
        eng.test_groups(loader, input_n=2, eval_frame=[0], horizon=5)
    for bad in ([0, 2], [-3]):
        with pytest.raises(ValueError, match="eval frame"):
            eng.test_groups(loader, input_n=2, eval_frame=bad)
    s.time_tsfm = object()
    with pytest.raises(ValueError, match="time"):
        eng.test_groups(loader, input_n=2, eval_frame=[0])
    s.time_tsfm = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # all valid: the call goes on to the device
        eng.test_groups(loader, input_n=2, eval_frame=[0, 1])
