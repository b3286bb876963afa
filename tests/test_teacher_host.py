"""Host-side checks of scheduled sampling over the rollout
(include/ext/dstd_gcn_teacher.h, dstd_native.ext.TEACHER_ABI, the teacher
arguments of DSTDGCN.rollout / rollout_pair and PredictionEngine.train) and of
the restatements the GPU tests compare against (no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dstd_native as native
from abi_reader import compare, parse
from conftest import ROOT
from model import get_model
from rollout_helper import rollout_backward, windows
from teacher_helper import (glue_dy_tf, glue_fold_tf, mixed_mask, teacher_backward, teacher_forward, teacher_reference,
                            truth_frames)
from test_taps_host import FAKE, H36M, _fake, _model_params

EINVAL, EWORKSPACE, ELIMIT = -1, -2, -3  # include/dstd_gcn.h
BIG = 1 << 40
HEADER = "ext/dstd_gcn_teacher.h"
SHAPES = [(5, 1), (1, 5), (3, 3), (4, 2)]  # (Tin, Tout), as tests/test_rollout_host.py
EXPORTS = ("dstd_model_rollout_tf_fwd", "dstd_model_rollout_tf_bwd", "dstd_model_rollout_tf_bwd_window",
           "dstd_model_rollout_tf_glue_bwd")


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", *HEADER.split("/"))).read()


# ---- the binding -----------------------------------------------------------------
def test_binding_agrees_with_the_teacher_header(header):
    assert compare({HEADER: header}, native.ext.teacher) == []
    protos = parse(header)[3]
    assert sorted(protos) == sorted(EXPORTS) and native.ext.TEACHER_EXPORTS == EXPORTS
    assert parse(header)[:3] == ({}, {}, {})  # no define, no struct, no callback: no size export either
    assert native.ext.teacher.C_TYPES == {} and set(native.ext.TEACHER_ABI) == {HEADER}
    assert set(native.ext.ALL) == {"ext/dstd_gcn_rollout.h", HEADER}


@pytest.mark.parametrize("what,marker,old,new,name", [
    ("parameter dropped", "int dstd_model_rollout_tf_bwd(", "const unsigned char* mask, ", "", "dstd_model_rollout_tf_bwd"),
    ("type changed", "int dstd_model_rollout_tf_fwd(", "int truth_T", "size_t truth_T", "dstd_model_rollout_tf_fwd"),
    ("prototype added", "int dstd_model_rollout_tf_glue_bwd(", "int dstd_model_rollout_tf_glue_bwd(",
     "int dstd_model_rollout_tf_new(int B);\nint dstd_model_rollout_tf_glue_bwd(", "dstd_model_rollout_tf_new"),
])
def test_an_altered_teacher_header_is_reported_by_name(header, what, marker, old, new, name):
    at = header.index(marker)
    assert old in header[at:]
    altered = header[:at] + header[at:].replace(old, new, 1)
    reports = compare({HEADER: altered}, native.ext.teacher)
    assert {r.split(":")[0] for r in reports} == {name}, reports


def test_library_exports_the_teacher_entry_points():
    from dstd_native import abi
    L = native.lib()
    for name, (restype, argtypes) in native.ext.TEACHER_ABI[HEADER].items():
        fn = getattr(L, name)  # the library exports it, and lib() declared it
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert not any(name in table for table in (*abi.ABI.values(), *native.ext.ABI.values())), name
    # no translation unit of its own: the entry points live beside the chain they extend,
    # which the Makefile lists and the source hash covers (with every include/ext/*.h)
    mk = open(os.path.join(ROOT, "dstd-gcn_amd", "Makefile")).read()
    src = open(os.path.join(ROOT, "dstd-gcn_amd", "csrc", "dstd_rollout.hip")).read()
    assert "csrc/dstd_rollout.hip" in mk and '#include "../../include/ext/dstd_gcn_teacher.h"' in src
    assert all(f"int {name}(" in src for name in EXPORTS)
    assert L.dstd_source_hash().decode() == native.source_hash()


# ---- refusals of the entry points --------------------------------------------------
def _ints(a, b):
    return (ctypes.c_int * 2)(a, b)


def _tf(truth=FAKE, truth_T=35, t0=(0, 34), step=(1, -1), mask=FAKE):
    return (truth, truth_T, None if t0 is None else _ints(*t0), None if step is None else _ints(*step), mask)


def _fwd(L, p, tf, B=2, Tin=10, H=25, nbytes=BIG, flags=0, saved=FAKE):
    ref = None if p is None else native.ext.model_params_ref(p)
    return L.dstd_model_rollout_tf_fwd(ref, FAKE, B, Tin, H, 0.1, 0.0, None, FAKE, saved, nbytes, *tf, None, flags)


def _bwd(L, p, tf, B=2, Tin=10, H=25, nbytes=BIG, flags=0, saved=FAKE, wbytes=BIG):
    ref = None if p is None else native.ext.model_params_ref(p)
    g = native.ext.model_grads_ref(_fake(native.ModelGrads()))
    return L.dstd_model_rollout_tf_bwd(ref, B, Tin, H, 0.0, None, saved, nbytes, FAKE, g, FAKE, FAKE, wbytes, *tf, None,
                                       flags)


def _bwd_window(L, p, tf, k=0, B=2, Tin=10, H=25, nbytes=BIG, flags=0, saved=FAKE, wbytes=BIG):
    ref = None if p is None else native.ext.model_params_ref(p)
    g = native.ext.model_grads_ref(_fake(native.ModelGrads()))
    return L.dstd_model_rollout_tf_bwd_window(ref, B, Tin, H, k, 0.0, None, saved, nbytes, FAKE, g, FAKE, FAKE, wbytes,
                                              *tf, None, flags)


def test_teacher_entry_points_refuse_bad_arguments_without_gpu():
    """The new DSTD_EINVAL cases, each before anything is dereferenced or
    launched (the pointers are fake), among the argument errors: before the
    window cap (DSTD_ELIMIT) and the sizes (DSTD_EWORKSPACE).  A call that
    passes everything shows as DSTD_EWORKSPACE on one-byte buffers."""
    L = native.lib()
    p = _model_params(35, 22, layers=5)
    PAIRED = native.TRAIN_PAIRED
    for call in (_fwd, _bwd, _bwd_window):
        ok = lambda tf, **kw: call(L, p, tf, nbytes=1, **kw)  # noqa: E731
        # the existing refusals, with a teacher and without
        for tf in (_tf(), _tf(truth=None, mask=None)):
            assert call(L, None, tf) == EINVAL
            assert call(L, p, tf, saved=None) == EINVAL
            assert call(L, p, tf, Tin=35) == EINVAL and call(L, p, tf, H=0) == EINVAL
            assert call(L, p, tf, B=3, flags=PAIRED) == EINVAL
            assert call(L, p, tf, flags=16) == EINVAL
            assert call(L, p, tf, Tin=1, H=64 * 34 + 1, nbytes=1) == (ELIMIT if tf[0] is None else EINVAL)  # frames
            assert ok(tf) == EWORKSPACE and ok(tf, flags=PAIRED) == EWORKSPACE
        assert ok(_tf(truth=None, mask=None, t0=None, step=None, truth_T=0)) == EWORKSPACE  # no teacher: nothing else read
        # truth and mask come together
        assert ok(_tf(truth=None)) == EINVAL and ok(_tf(mask=None)) == EINVAL
        assert ok(_tf(t0=None)) == EINVAL and ok(_tf(step=None)) == EINVAL
        assert ok(_tf(truth_T=0)) == EINVAL and ok(_tf(truth_T=-4)) == EINVAL
        # a step that is not +-1, of a half the call has
        for bad in (0, 2, -2):
            assert ok(_tf(truth_T=60, step=(bad, -1)), H=26) == EINVAL
            assert ok(_tf(truth_T=60, t0=(0, 59), step=(1, bad)), H=26, flags=PAIRED) == EINVAL
            assert ok(_tf(truth_T=60, step=(1, bad)), H=26) == EWORKSPACE  # unpaired: one half
        # frames: Tin = 10, Tout = 25.  One window reads no truth; two windows read window 1's
        # observed frames tau = 25 .. 34 (its padding repeats 34), whatever the horizon cuts off
        assert ok(_tf(truth_T=1, t0=(7, 0)), H=25) == EWORKSPACE
        assert ok(_tf(truth_T=35), H=50) == EWORKSPACE
        assert ok(_tf(truth_T=34), H=50) == EINVAL
        assert ok(_tf(truth_T=35), H=26) == EWORKSPACE
        assert ok(_tf(truth_T=34), H=26) == EINVAL
        assert ok(_tf(truth_T=60), H=51) == EWORKSPACE  # three windows: tau = 25 .. 59
        assert ok(_tf(truth_T=59), H=51) == EINVAL
        assert ok(_tf(truth_T=36, t0=(1, 0)), H=50) == EWORKSPACE
        assert ok(_tf(truth_T=36, t0=(2, 0)), H=50) == EINVAL
        assert ok(_tf(truth_T=60, t0=(-1, 0)), H=50) == EWORKSPACE  # tau = 0 is not read: frame 24 first
        assert ok(_tf(truth_T=60, t0=(-25, 0)), H=50) == EWORKSPACE
        assert ok(_tf(truth_T=60, t0=(-26, 0)), H=50) == EINVAL
        assert ok(_tf(truth_T=35, t0=(34, 0), step=(-1, 1)), H=50) == EWORKSPACE  # frames 9 .. 0
        assert ok(_tf(truth_T=35, t0=(33, 0), step=(-1, 1)), H=50) == EINVAL  # below frame 0
        assert ok(_tf(truth_T=35, t0=(59, 0), step=(-1, 1)), H=50) == EWORKSPACE  # frames 34 .. 25
        assert ok(_tf(truth_T=35, t0=(60, 0), step=(-1, 1)), H=50) == EINVAL
        assert ok(_tf(truth_T=2 ** 31 - 1, t0=(2 ** 31 - 36, 0)), H=50) == EWORKSPACE  # no int overflow in the check
        assert ok(_tf(truth_T=2 ** 31 - 1, t0=(2 ** 31 - 35, 0)), H=50) == EINVAL
        # the second half is checked under DSTD_TRAIN_PAIRED alone
        assert ok(_tf(truth_T=35, t0=(0, 34), step=(1, -1)), H=50, flags=PAIRED) == EWORKSPACE
        assert ok(_tf(truth_T=35, t0=(0, 33), step=(1, -1)), H=50, flags=PAIRED) == EINVAL
        assert ok(_tf(truth_T=35, t0=(0, 33), step=(1, -1)), H=50) == EWORKSPACE
        # an argument error wins over the window cap, the window cap over the sizes
        assert ok(_tf(truth_T=35), H=64 * 25 + 1) == EINVAL
        assert ok(_tf(truth_T=10 + 64 * 25), H=64 * 25 + 1) == ELIMIT
        assert ok(_tf(truth_T=10 + 63 * 25), H=64 * 25) == EWORKSPACE
        assert ok(_tf(truth_T=9 + 63 * 25), H=64 * 25) == EINVAL
        # the sizes are the rollout's
        need = L.dstd_model_rollout_saved_bytes(2, 35, 22, 64, 5, 2)
        assert call(L, p, _tf(truth_T=60), H=50, nbytes=need - 1) == EWORKSPACE
    assert _bwd(L, p, _tf(truth_T=60), H=50, wbytes=L.dstd_model_rollout_workspace_bytes(2, 35, 22, 64, 5) - 1) == EWORKSPACE
    assert _bwd_window(L, p, _tf(), k=-1) == EINVAL and _bwd_window(L, p, _tf(), k=1) == EINVAL
    assert _bwd_window(L, p, _tf(truth_T=60), k=1, H=50, nbytes=1) == EWORKSPACE


def test_teacher_glue_hook_refuses_bad_arguments_without_gpu():
    L = native.lib()

    def hook(step=0, dout=FAKE, Gn=FAKE, dst=FAKE, mrow=FAKE, B=3, T=6, Tin=4, V=22, H=5, k=0):
        return L.dstd_model_rollout_tf_glue_bwd(step, dout, Gn, dst, mrow, B, T, Tin, V, H, k, None)

    for mrow in (FAKE, None):
        assert hook(dst=None, mrow=mrow) == EINVAL
        assert hook(step=0, dout=None, mrow=mrow) == EINVAL
        assert hook(step=1, Gn=None, mrow=mrow) == EINVAL and hook(step=2, Gn=None, mrow=mrow) == EINVAL
        assert hook(step=3, mrow=mrow) == EINVAL and hook(step=-1, mrow=mrow) == EINVAL
        assert hook(B=0, mrow=mrow) == EINVAL and hook(V=0, mrow=mrow) == EINVAL
        assert hook(Tin=0, mrow=mrow) == EINVAL and hook(Tin=6, mrow=mrow) == EINVAL and hook(H=0, mrow=mrow) == EINVAL
        assert hook(k=-1, mrow=mrow) == EINVAL and hook(k=3, mrow=mrow) == EINVAL
        assert hook(step=1, Tin=3, mrow=mrow) == 0  # nothing carried over: no launch


# ---- refusals of the Python layer --------------------------------------------------
def test_teacher_arguments_are_checked_before_anything_runs():
    """On CPU tensors: every teacher refusal is a ValueError that comes before
    the device is looked at (a valid teacher then meets 'no CPU fallback')."""
    m = get_model("dstdgcn", dstdgcn=H36M)
    obs = torch.zeros(2, 10, 22, 3)
    teacher, mask = torch.zeros(2, 60, 22, 3), torch.zeros(2, 2, dtype=torch.bool)
    for mode in (m.train, m.eval):
        mode()
        for call, msk in ((lambda **kw: m.rollout(obs, 50, **kw), mask),
                          (lambda **kw: m.rollout_pair(obs, obs, 50, **kw), torch.zeros(2, 4, dtype=torch.uint8))):
            with pytest.raises(ValueError, match="come together"):
                call(teacher=teacher)
            with pytest.raises(ValueError, match="come together"):
                call(teacher_mask=msk)
            with pytest.raises(ValueError, match="frames"):
                call(teacher=teacher[:, :59], teacher_mask=msk)
            for bad in (teacher[:1], teacher[:, :, :21], teacher[..., :2], teacher[0]):
                with pytest.raises(ValueError, match="expected teacher"):
                    call(teacher=bad, teacher_mask=msk)
            with pytest.raises(ValueError, match="float32"):
                call(teacher=teacher.double(), teacher_mask=msk)
            with pytest.raises(ValueError, match="bool or uint8"):
                call(teacher=teacher, teacher_mask=msk.float())
            for bad in (msk[:1], msk[:, :1], msk[0], torch.cat([msk, msk])):
                with pytest.raises(ValueError, match="teacher_mask"):
                    call(teacher=teacher, teacher_mask=bad)
            with pytest.raises(ValueError, match="is on"):
                call(teacher=teacher.to("meta"), teacher_mask=msk)
            with pytest.raises(ValueError, match="must be a tensor"):
                call(teacher=teacher.numpy(), teacher_mask=msk)
        with pytest.raises(RuntimeError, match="no CPU fallback"):  # all valid: the call goes on to the device
            m.rollout(obs, 50, teacher=teacher, teacher_mask=mask)
    m.eval()
    for p in m.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match="predict has no teacher"):  # eval mode, nothing to differentiate
        m.rollout(obs, 50, teacher=teacher, teacher_mask=mask)
    with pytest.raises(RuntimeError, match="predict has no teacher"):
        m.rollout_pair(obs, obs, 50, teacher=teacher, teacher_mask=torch.zeros(2, 4, dtype=torch.bool))
    from model import dstdgcn_fast as F
    assert not hasattr(F.DSTDGCN, "rollout")  # the channels-last model has none


def test_engine_teacher_ratio_refusals():
    from engine import PredictionEngine

    class Log:
        def info(self, *a):
            pass

    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5),
               loss=dict(joint=["jl2", 1]), n_out=1, transform="tsc", use_weight=True, inverse=True)
    eng = PredictionEngine(cfg, get_model("dstdgcn", dstdgcn=dict(H36M, num_layers=1, num_feature=8)), Log())
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="teacher_ratio"):
            eng.train([], 0, horizon=50, teacher_ratio=bad)
    with pytest.raises(ValueError, match="needs horizon"):
        eng.train([], 0, teacher_ratio=0.5)


# ---- the restatements --------------------------------------------------------------
def _linear(T, feat, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T * feat, T * feat)) / np.sqrt(T * feat)


def _masks(K, N):
    return {"zero": np.zeros((K, N), np.uint8), "one": np.ones((K, N), np.uint8), "mixed": mixed_mask(K, N, N // 2)}


@pytest.mark.parametrize("Tin,Tout", SHAPES)
def test_closed_form_with_a_mask_is_autograd_of_the_forward_restatement(Tin, Tout):
    """K = 3 (and a truncated last window), a pair of 2 + 2 samples over one
    truth read forwards and backwards, a linear stand-in y = x M for every
    window: the numpy fp64 forward and backward against torch autograd of the
    forward written with indexing and torch.where, to 1e-12; the all-zero mask
    is rollout_helper's closed form."""
    T, N, tail = Tin + Tout, 4, (2, 3)
    M = _linear(T, 6, 10 * Tin + Tout)
    Mt = torch.from_numpy(M)
    rng = np.random.default_rng(11)
    for H in (3 * Tout, 3 * Tout - 1) if Tout > 1 else (3,):
        K = windows(T, Tin, H)
        assert K == 3
        truth = rng.standard_normal((N // 2, Tin + H) + tail)
        maps = [(0, 1), (Tin + H - 1, -1)]
        for name, mask in _masks(K, N).items():
            obs = torch.from_numpy(rng.standard_normal((N, Tin) + tail)).requires_grad_()
            dout = rng.standard_normal((N, H) + tail)
            out = teacher_reference(lambda x: (x.reshape(N, -1) @ Mt).reshape(x.shape), obs, torch.from_numpy(truth), maps,
                                    torch.from_numpy(mask), T, H)
            out.backward(torch.from_numpy(dout))
            fwd, xs = teacher_forward(obs.detach().numpy(), truth, maps, mask, T, H,
                                      lambda k, x: (x.reshape(N, -1) @ M).reshape(x.shape))
            assert float(np.abs(fwd - out.detach().numpy()).max()) <= 1e-12, (H, name)
            vjp = lambda k, dy: (dy.reshape(N, -1) @ M.T).reshape(dy.shape)  # noqa: E731
            got = teacher_backward(dout, mask, T, Tin, vjp)
            assert float(np.abs(got - obs.grad.numpy()).max()) <= 1e-12, (H, name)
            if name == "zero":
                assert np.array_equal(got, rollout_backward(dout, T, Tin, vjp))
            if name == "one":  # window 0 alone reaches obs
                assert np.array_equal(got, rollout_backward(dout[:, :Tout], T, Tin, vjp))
                for k in range(1, K):  # and every later window is the truth's
                    for h in range(2):
                        want = truth[:, truth_frames(T, Tin, k, maps[h])]
                        assert np.array_equal(xs[k][h * 2:(h + 1) * 2], want)


def test_masked_glue_steps_select_per_sample():
    """glue_dy_tf / glue_fold_tf: a forced sample's rows are the steps without
    G_{k+1}, a free sample's the steps with it; no mask row is the plain step."""
    from rollout_helper import glue_dy, glue_fold
    T, Tin, N, H = 6, 4, 3, 5
    rng = np.random.default_rng(5)
    dout, Gn, dx = (rng.standard_normal((N, t, 2, 3)).astype(np.float32) for t in (H, T, T))
    mrow = np.array([1, 0, 1], np.uint8)
    dy, G = glue_dy_tf(dout, Gn, mrow, T, Tin, 0), glue_fold_tf(dx, Gn, mrow, T, Tin)
    assert np.array_equal(dy[[0, 2]], glue_dy(dout, None, T, Tin, 0)[[0, 2]])
    assert np.array_equal(dy[1], glue_dy(dout, Gn, T, Tin, 0)[1]) and not np.array_equal(dy[0], glue_dy(dout, Gn, T, Tin, 0)[0])
    assert np.array_equal(G[[0, 2]], dx[[0, 2]]) and np.array_equal(G[1], glue_fold(dx, Gn, T, Tin)[1])
    assert np.array_equal(glue_dy_tf(dout, Gn, None, T, Tin, 0), glue_dy(dout, Gn, T, Tin, 0))
    assert np.array_equal(glue_dy_tf(dout, None, mrow, T, Tin, 2), glue_dy(dout, None, T, Tin, 2))
