"""Host-side checks of training through a strided rollout
(include/ext/dstd_gcn_stride_train.h, dstd_native.ext_stride_train,
DSTDGCN.rollout(stride=), PredictionEngine.train(stride=)) and of the loop the
GPU tests compare against (tests/rollout_stride_helper.py).  No GPU needed: the
entry points' refusals come before any HIP call, and the Python refusals before
anything touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dstd_native as native
from abi_reader import compare, parse
from conftest import ROOT
from dstd_native import abi
from guard_helper import rup
from model import dstdgcn_fast as F
from model import get_model
from rollout_stride_helper import StridedLoop, glue_acc, glue_dy, strided_reference, windows
from stride_helper import predict_strided_reference
from teacher_helper import mixed_mask
from test_taps_host import FAKE, H36M, _fake, _model_params

EINVAL, EWORKSPACE, ELIMIT = -1, -2, -3  # include/dstd_gcn.h
BIG = 1 << 40
PAIRED = 2  # DSTD_TRAIN_PAIRED
HEADER = "ext/dstd_gcn_stride_train.h"
NAMES = ("dstd_model_rollout_strided_workspace_bytes", "dstd_model_rollout_strided_fwd",
         "dstd_model_rollout_strided_bwd", "dstd_model_rollout_strided_bwd_window",
         "dstd_model_rollout_strided_glue_bwd")
CASES = [(4, 2, 1, 5), (3, 3, 2, 7), (1, 5, 2, 9), (2, 4, 3, 2)]  # (Tin, Tout, S, H)


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", *HEADER.split("/"))).read()


# ---- header and binding -------------------------------------------------------------
def test_binding_agrees_with_the_header(header):
    assert compare({HEADER: header}, native.ext_stride_train) == []
    defines, structs, callbacks, protos = parse(header)
    assert sorted(protos) == sorted(NAMES) and native.ext_stride_train.STRIDE_TRAIN_EXPORTS == NAMES
    assert (defines, structs, callbacks) == ({}, {}, {}) and native.ext_stride_train.C_TYPES == {}
    assert "typedef" not in header and "#define DSTD_GCN_STRIDE_TRAIN_H" in header
    assert set(native.ext_stride_train.ABI) == {HEADER}
    names = [p[2] for p in protos["dstd_model_rollout_strided_fwd"][1]]
    assert names == ["p", "obs", "B", "input_n", "horizon", "stride", "momentum", "dropout_p", "seeds", "out", "saved",
                     "saved_bytes", "truth", "truth_T", "t0", "step", "mask", "stream", "flags"]
    names = [p[2] for p in protos["dstd_model_rollout_strided_bwd_window"][1]]
    assert names == ["p", "B", "input_n", "horizon", "stride", "k", "dropout_p", "seeds", "saved", "saved_bytes", "dout",
                     "g", "dobs", "workspace", "workspace_bytes", "truth", "truth_T", "t0", "step", "mask", "stream",
                     "flags"]


@pytest.mark.parametrize("marker,old,new,name", [
    ("int dstd_model_rollout_strided_bwd(", "int horizon, int stride,", "int horizon,", "dstd_model_rollout_strided_bwd"),
    ("int dstd_model_rollout_strided_fwd(", "int truth_T", "size_t truth_T", "dstd_model_rollout_strided_fwd"),
    ("int dstd_model_rollout_strided_glue_bwd(", "int dstd_model_rollout_strided_glue_bwd(",
     "int dstd_model_rollout_strided_new(int B);\nint dstd_model_rollout_strided_glue_bwd(",
     "dstd_model_rollout_strided_new"),
])
def test_an_altered_header_is_reported_by_name(header, marker, old, new, name):
    at = header.index(marker)
    assert old in header[at:]
    reports = compare({HEADER: header[:at] + header[at:].replace(old, new, 1)}, native.ext_stride_train)
    assert {r.split(":")[0] for r in reports} == {name}, reports


def test_library_exports_the_symbols_and_the_pinned_tables_are_as_they_were():
    L = native.lib()
    for name, (restype, argtypes) in native.ext_stride_train.ABI[HEADER].items():
        fn = getattr(L, name)  # exported, and declared by lib()
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # a table of its own: the key counts of the pinned ones are unchanged
    assert set(native.ext.ALL) == {"ext/dstd_gcn_rollout.h", "ext/dstd_gcn_teacher.h"}
    assert sum(len(t) for t in native.ext.ALL.values()) == 10
    assert set(native.ext.ABI) == {"ext/dstd_gcn_rollout.h"} and len(native.ext.ABI["ext/dstd_gcn_rollout.h"]) == 6
    assert list(native.ext_eval.ABI) == ["ext/dstd_gcn_eval.h"] and len(native.ext_eval.ABI["ext/dstd_gcn_eval.h"]) == 1
    assert list(native.ext_augment.ABI) == ["ext/dstd_gcn_augment.h"]
    assert len(native.ext_augment.ABI["ext/dstd_gcn_augment.h"]) == 1
    assert list(native.ext_stride.ABI) == ["ext/dstd_gcn_stride.h"] and len(native.ext_stride.ABI["ext/dstd_gcn_stride.h"]) == 2
    assert sum(len(t) for t in abi.ABI.values()) == 61 and len(abi.C_TYPES) == 15 and len(abi.ABI) == 7
    others = (*abi.ABI.values(), *native.ext.ALL.values(), *native.ext_eval.ABI.values(),
              *native.ext_augment.ABI.values(), *native.ext_stride.ABI.values())
    assert not any(name in t for t in others for name in NAMES)
    assert not hasattr(native, "STRIDE_TRAIN_EXPORTS")
    assert native.ext_stride_train.model_params_ref is native.ext.model_params_ref
    assert native.ext_stride_train.model_grads_ref is native.ext.model_grads_ref
    mk = open(os.path.join(ROOT, "dstd-gcn_amd", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "csrc/dstd_rollout_stride.hip" in srcs and "csrc/dstd_rollout.hip" in srcs
    assert "csrc/dstd_chain.h" in re.search(r"^HDRS := (.*)$", mk, re.M).group(1).split()
    assert L.dstd_source_hash().decode() == native.source_hash()  # the new sources are hashed


def test_a_library_without_the_symbols_is_a_load_error():
    extra = {**native.ext.ALL, **native.ext_eval.ABI, **native.ext_augment.ABI, **native.ext_stride.ABI,
             **native.ext_stride_train.ABI}
    for missing in NAMES:
        class Lib:
            _name = "libold.so"

            def __getattr__(self, name, missing=missing):
                if name == missing:
                    raise AttributeError(name)
                return type("Fn", (), {})()

        with pytest.raises(RuntimeError, match=missing + r"\b"):
            native.declare(Lib(), extra=extra)
        native.declare(Lib(), allow_missing=True, extra=extra)


# ---- sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,V,C,layers", [(3, 35, 22, 64, 5), (2, 6, 5, 8, 1)])
def test_sizes_are_the_stated_closed_forms(B, T, V, C, layers):
    """workspace: the model backward's region, dy, dx and Gh, each rounded up to
    256 bytes; saved: dstd_gcn_rollout.h's layout with K = ceil(H / S) windows."""
    L = native.lib()
    W = rup(12 * B * T * V, 256)
    SV = rup(L.dstd_model_train_saved_bytes(B, T, V, C, layers), 256)
    M = rup(L.dstd_model_train_workspace_bytes(B, T, V, C, layers), 256)
    for Tin, H in ((T // 3, 100), (1, 1), (T - 1, 7)):
        got = L.dstd_model_rollout_strided_workspace_bytes(B, T, V, C, layers, Tin, H)
        assert got == M + 2 * W + rup(12 * B * (Tin + H) * V, 256), (Tin, H)
    assert L.dstd_model_rollout_strided_workspace_bytes(B, T, V, C, layers, 0, 0) == M + 2 * W
    assert L.dstd_model_rollout_strided_workspace_bytes(B, T, V, C, layers, 3, -9) == M + 2 * W
    if T == 35:
        assert (W, SV, M) == (27904, 56400128, 22648832)
        assert L.dstd_model_rollout_strided_workspace_bytes(B, T, V, C, layers, 10, 100) == 22791936
    for S, H in ((10, 100), (5, 100), (1, 3)):
        K = windows(H, S)
        assert L.dstd_model_rollout_saved_bytes(B, T, V, C, layers, K) == W + K * (W + SV)


# ---- refusals of the entry points -----------------------------------------------------
def _tf(truth=FAKE, truth_T=110, t0=(0, 109), step=(1, -1), mask=FAKE):
    arr = lambda v: None if v is None else (ctypes.c_int * 2)(*v)  # noqa: E731
    return truth, truth_T, arr(t0), arr(step), mask


NO_TF = (None, 0, None, None, None)


def _grads():
    return _fake(native.ModelGrads())


def _fwd(L, p, tf=NO_TF, obs=FAKE, B=2, Tin=10, H=25, S=10, drop=0.0, seeds=None, out=FAKE, saved=FAKE, nbytes=BIG,
         flags=0):
    ref = None if p is None else native.ext_stride_train.model_params_ref(p)
    return L.dstd_model_rollout_strided_fwd(ref, obs, B, Tin, H, S, 0.1, drop, seeds, out, saved, nbytes, *tf, None,
                                            flags)


def _bwd(L, p, tf=NO_TF, B=2, Tin=10, H=25, S=10, drop=0.0, seeds=None, saved=FAKE, nbytes=BIG, dout=FAKE, g="fake",
         dobs=FAKE, ws=FAKE, wbytes=BIG, flags=0, k=None):
    ref = None if p is None else native.ext_stride_train.model_params_ref(p)
    gref = None if g is None else native.ext_stride_train.model_grads_ref(_grads() if g == "fake" else g)
    tail = (drop, seeds, saved, nbytes, dout, gref, dobs, ws, wbytes, *tf, None, flags)
    if k is None:
        return L.dstd_model_rollout_strided_bwd(ref, B, Tin, H, S, *tail)
    return L.dstd_model_rollout_strided_bwd_window(ref, B, Tin, H, S, k, *tail)


def _bwd_window(L, p, tf=NO_TF, k=0, **kw):
    return _bwd(L, p, tf, k=k, **kw)


def test_entry_points_refuse_bad_arguments_without_gpu():
    """Every refusal returns before anything is dereferenced or launched (the
    pointers are fake), in the order of the header: arguments (DSTD_EINVAL), the
    window cap and the envelope (DSTD_ELIMIT), the sizes (DSTD_EWORKSPACE, saved
    first).  A call that passes the first two shows as DSTD_EWORKSPACE on
    one-byte buffers."""
    L = native.lib()
    p = _model_params(35, 22, layers=5)
    for call in (_fwd, _bwd, _bwd_window):
        assert call(L, None) == EINVAL
        assert call(L, p, saved=None) == EINVAL
        for Tin in (0, 35, 36):
            assert call(L, p, Tin=Tin, S=1) == EINVAL
        for H in (0, -3):
            assert call(L, p, H=H) == EINVAL
        for S in (0, -1, 26, 1 << 30):
            assert call(L, p, S=S) == EINVAL, S
        for S in (1, 10, 25):
            assert call(L, p, S=S, nbytes=1) == EWORKSPACE, S
        assert call(L, p, Tin=34, S=2) == EINVAL and call(L, p, Tin=34, S=1, H=3, nbytes=1) == EWORKSPACE
        assert call(L, p, drop=0.1, seeds=None) == EINVAL  # a mask needs its seeds
        assert call(L, p, drop=1.0, seeds=FAKE, flags=4) == EINVAL
        for bad in (16, 32, 1 << 31, 2 | 64):
            assert call(L, p, flags=bad) == EINVAL, bad
        for ok in (0, 1, 2, 8, 1 | 2, 2 | 8, 1 | 2 | 8):  # exactly the flags of dstd_model_train_fwd_ex ...
            assert call(L, p, flags=ok, nbytes=1) == EWORKSPACE, ok
        assert call(L, p, drop=0.1, seeds=FAKE, flags=4 | 2, nbytes=1) == EWORKSPACE  # ... DSTD_TRAIN_SEED_DEVICE too
        assert call(L, p, B=3, flags=2) == EINVAL and call(L, p, B=0) == EINVAL
        assert call(L, _model_params(35, 0, layers=5)) == EINVAL
        assert call(L, _model_params(35, 22, layers=17)) == EINVAL
        q = _model_params(35, 22, layers=5)
        q.enc[3].conv_t.wrm = None  # a parameter pointer: refused here, not by window 0
        assert call(L, q) == EINVAL
        # the window cap: 64 windows of S frames pass, one frame more does not; H = 100 needs S >= 2
        for S in (1, 2, 10, 25):
            assert call(L, p, S=S, H=64 * S + 1, nbytes=1) == ELIMIT
            assert call(L, p, S=S, H=64 * S, nbytes=1) == EWORKSPACE
        assert call(L, p, S=1, H=100) == ELIMIT and call(L, p, S=2, H=100, nbytes=1) == EWORKSPACE
        assert call(L, p, S=1, H=2 ** 31 - 1) == ELIMIT  # K is counted beyond an int
        # an argument error wins over the window cap, the window cap over the envelope and the sizes
        assert call(L, p, S=0, H=10 ** 6) == EINVAL
        assert call(L, p, S=1, H=100, flags=16) == EINVAL
        assert call(L, _model_params(129, 22), S=1, H=100) == ELIMIT
        assert call(L, _model_params(129, 22)) == ELIMIT and call(L, _model_params(35, 33)) == ELIMIT
        # saved, below the export for this horizon's windows (H = 25 at S = 10: 3)
        need = L.dstd_model_rollout_saved_bytes(2, 35, 22, 64, 5, 3)
        assert call(L, p, nbytes=need - 1) == EWORKSPACE
        assert call(L, p, H=31, nbytes=need) == EWORKSPACE
        # the teacher: dstd_gcn_teacher.h's refusals over tau = S .. (K-1) S + Tin - 1, argument errors all
        ok = lambda tf, **kw: call(L, p, tf, nbytes=1, **kw)  # noqa: E731
        assert ok(_tf()) == EWORKSPACE and ok(NO_TF) == EWORKSPACE
        assert ok(_tf(truth=None)) == EINVAL and ok(_tf(mask=None)) == EINVAL
        assert ok(_tf(t0=None)) == EINVAL and ok(_tf(step=None)) == EINVAL
        assert ok(_tf(truth_T=0)) == EINVAL
        for bad in (0, 2, -2):
            assert ok(_tf(step=(bad, -1))) == EINVAL
            assert ok(_tf(step=(1, bad)), flags=PAIRED) == EINVAL and ok(_tf(step=(1, bad))) == EWORKSPACE
        # H = 25 at S = 10: K = 3, tau = 10 .. 29 -- less than Tin + H = 35 frames suffice
        assert ok(_tf(truth_T=30)) == EWORKSPACE and ok(_tf(truth_T=29)) == EINVAL
        assert ok(_tf(truth_T=30, t0=(-10, 0))) == EWORKSPACE and ok(_tf(truth_T=30, t0=(-11, 0))) == EINVAL
        assert ok(_tf(truth_T=35, t0=(0, 34)), flags=PAIRED) == EWORKSPACE  # the reversal: frames 24 .. 5
        assert ok(_tf(truth_T=35, t0=(0, 28)), flags=PAIRED) == EINVAL  # ... 18 .. -1
        assert ok(_tf(truth_T=35, t0=(0, 28))) == EWORKSPACE  # unpaired: one half
        assert ok(_tf(truth_T=1, t0=(7, 0)), H=10) == EWORKSPACE  # one window reads nothing
        assert ok(_tf(truth_T=10 + 100), S=2, H=100) == EWORKSPACE  # Tin + H always suffices
        assert ok(_tf(truth_T=10 + 100, t0=(0, 109)), S=2, H=100, flags=PAIRED) == EWORKSPACE
        assert ok(_tf(truth_T=2 ** 31 - 1, t0=(2 ** 31 - 31, 0))) == EWORKSPACE  # no int overflow in the check
        assert ok(_tf(truth_T=2 ** 31 - 1, t0=(2 ** 31 - 30, 0))) == EINVAL
        assert ok(_tf(truth_T=29), S=1, H=100) == EINVAL  # a teacher's argument error wins over the window cap
        assert ok(_tf(truth_T=200), S=1, H=100) == ELIMIT
    # the window of a one-window backward: 0 .. K-1 (H = 25 at S = 10: 0 .. 2)
    assert _bwd_window(L, p, k=-1) == EINVAL and _bwd_window(L, p, k=3) == EINVAL
    assert _bwd_window(L, p, k=2, nbytes=1) == EWORKSPACE
    assert _bwd_window(L, p, k=100, S=1, H=100) == EINVAL  # an argument error wins over the window cap
    assert _bwd_window(L, p, k=99, S=1, H=100) == ELIMIT
    # each direction's own pointers
    assert _fwd(L, p, obs=None) == EINVAL and _fwd(L, p, out=None) == EINVAL
    assert _bwd(L, p, dout=None) == EINVAL and _bwd(L, p, g=None) == EINVAL and _bwd(L, p, ws=None) == EINVAL
    g = _grads()
    g.enc[2].conv_s[1].bm2 = None
    assert _bwd(L, p, g=g) == EINVAL
    # the backward's workspace comes after saved
    assert _bwd(L, p, nbytes=1, wbytes=1) == EWORKSPACE
    need = L.dstd_model_rollout_strided_workspace_bytes(2, 35, 22, 64, 5, 10, 25)
    assert _bwd(L, p, wbytes=need - 1) == EWORKSPACE
    assert _bwd(L, p, wbytes=L.dstd_model_train_workspace_bytes(2, 35, 22, 64, 5)) == EWORKSPACE
    # Gh grows with the horizon: the unstrided chain's three windows hold H = 25 and no frame more
    assert need == L.dstd_model_rollout_workspace_bytes(2, 35, 22, 64, 5)
    assert _bwd(L, p, H=26, wbytes=need) == EWORKSPACE


def test_glue_hook_refuses_bad_arguments_without_gpu():
    L = native.lib()

    def hook(step=0, dout=FAKE, dx=FAKE, Gh=FAKE, dst=FAKE, mrow=FAKE, B=3, T=6, Tin=4, V=22, H=5, S=1, k=0):
        return L.dstd_model_rollout_strided_glue_bwd(step, dout, dx, Gh, dst, mrow, B, T, Tin, V, H, S, k, None)

    assert hook(Gh=None) == EINVAL and hook(step=1, Gh=None) == EINVAL
    assert hook(step=0, dout=None) == EINVAL and hook(step=0, dst=None) == EINVAL
    assert hook(step=1, dx=None) == EINVAL
    assert hook(step=2) == EINVAL and hook(step=-1) == EINVAL
    assert hook(B=0) == EINVAL and hook(V=0) == EINVAL
    assert hook(Tin=0) == EINVAL and hook(Tin=6) == EINVAL and hook(H=0) == EINVAL
    assert hook(S=0) == EINVAL and hook(S=3) == EINVAL
    assert hook(k=-1) == EINVAL and hook(k=5) == EINVAL and hook(S=2, k=3) == EINVAL  # H = 5: windows 0 .. 4, 0 .. 2


# ---- refusals of the Python surface ---------------------------------------------------
def test_rollout_refuses_a_bad_stride_on_a_cpu_model():
    m = get_model("dstdgcn", dstdgcn=H36M)
    obs = torch.zeros(2, 10, 22, 3)
    for mode in (m.train, m.eval):
        mode()
        for bad in (0, 26, -1, 2.5, True, "10", 10.0):
            with pytest.raises(ValueError, match=r"DSTDGCN\.rollout: stride must be an integer in 1\.\.25"):
                m.rollout(obs, 53, stride=bad)
        with pytest.raises(ValueError, match=r"DSTDGCN\.rollout: .*stride >= 2\b"):
            m.rollout(obs, 100, stride=1)
        with pytest.raises(ValueError, match=r"stride >= 16\b"):
            m.rollout(obs, 1000, stride=10)
        with pytest.raises(ValueError, match="windows of 25 frames"):  # no stride of this model fits: said as before
            m.rollout(obs, 64 * 25 + 1, stride=5)
        with pytest.raises(ValueError, match="horizon"):
            m.rollout(obs, 0, stride=5)
        for ok in (1, 10, 25, None, np.int64(5)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                m.rollout(obs, 53, stride=ok)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.rollout(obs, 64, stride=1)  # 64 windows exactly
    m.train()
    with pytest.raises(ValueError, match=r"DSTDGCN\.rollout_pair: stride must be"):
        m.rollout_pair(obs, obs, 53, stride=0)
    with pytest.raises(ValueError, match=r"DSTDGCN\.rollout_pair: .*stride >= 2\b"):
        m.rollout_pair(obs, obs, 100, stride=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.rollout_pair(obs, obs, 53, stride=10)
    # the mask has ceil(H / S) rows
    teacher = torch.zeros(2, 63, 22, 3)
    with pytest.raises(ValueError, match=r"expected teacher_mask \[6, 2\]"):
        m.rollout(obs, 53, teacher=teacher, teacher_mask=torch.zeros(3, 2, dtype=torch.bool), stride=10)
    with pytest.raises(ValueError, match=r"expected teacher_mask \[6, 4\]"):
        m.rollout_pair(obs, obs, 53, teacher=teacher, teacher_mask=torch.zeros(6, 2, dtype=torch.bool), stride=10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.rollout(obs, 53, teacher=teacher, teacher_mask=torch.zeros(6, 2, dtype=torch.bool), stride=10)
    with pytest.raises(ValueError, match=r"expected teacher_mask \[3, 2\]"):  # a whole window's stride: today's rows
        m.rollout(obs, 53, teacher=teacher, teacher_mask=torch.zeros(6, 2, dtype=torch.bool), stride=25)

    class Sub(torch.Tensor):
        pass

    with pytest.raises(RuntimeError, match="eager only"):
        m.rollout(obs.as_subclass(Sub), 53, stride=10)
    m._dstd_bn_sync = object()  # what dstd_dist.convert_sync_batchnorm installs
    try:
        with pytest.raises(NotImplementedError, match="cross-rank BatchNorm"):
            m.rollout(obs, 53, stride=10)
        with pytest.raises(NotImplementedError, match="cross-rank BatchNorm"):
            m.rollout_pair(obs, obs, 53, stride=10)
    finally:
        del m._dstd_bn_sync
    assert not hasattr(F.DSTDGCN, "rollout")  # the channels-last model has none


def test_engine_refuses_a_stride_without_a_horizon():
    from test_stride_host import _engine
    eng = _engine()
    batch = (torch.zeros(2, 6, 66), torch.zeros(2, 6, 66), torch.zeros(2, 6, 66), torch.zeros(2, 6, 96))
    with pytest.raises(ValueError, match="stride.*horizon"):
        eng.train([batch], 0, stride=1)
    with pytest.raises(ValueError, match="stride must be an integer in 1..2"):
        eng.train([batch], 0, horizon=4, stride=3)
    assert eng.model.model._dstd_inplace_grads is False  # restored on the way out
    import inspect
    assert list(inspect.signature(eng.train).parameters)[-3:] == ["horizon", "teacher_ratio", "stride"]


# ---- the loop's backward --------------------------------------------------------------
def _mask(name, K, N):
    m = {"none": None, "zero": np.zeros((K, N), np.uint8), "one": np.ones((K, N), np.uint8),
         "mixed": mixed_mask(K, N) if K > 1 else np.array([[1, 0, 1, 0][:N]], np.uint8)}[name]
    return None if m is None else torch.from_numpy(m)


@pytest.mark.parametrize("mask_name", ["none", "zero", "one", "mixed"])
@pytest.mark.parametrize("Tin,Tout,S,H", CASES)
def test_loop_backward_is_autograd_of_the_forward_restatement(Tin, Tout, S, H, mask_name):
    """StridedLoop's hand-composed backward in float64 against torch autograd
    through strided_reference (indexing, concatenation and, for a mask, one
    torch.where per window; free running it is predict_strided_reference), with
    a random linear map per window as the forward: observed.grad and every map's gradient within 1e-12 relative (the
    two sum the same terms in other orders)."""
    T, N, tail = Tin + Tout, 4, (2, 3)
    K = windows(H, S)
    rng = np.random.default_rng(1000 * Tin + 100 * Tout + 10 * S + H)
    D = T * 6
    Ms = [torch.from_numpy(rng.standard_normal((D, D)) / np.sqrt(D)).requires_grad_() for _ in range(K)]
    Ls = [m.detach().clone().requires_grad_() for m in Ms]
    obs = torch.from_numpy(rng.standard_normal((N, Tin) + tail))
    truth = torch.from_numpy(rng.standard_normal((N, Tin + H) + tail))
    dout = torch.from_numpy(rng.standard_normal((N, H) + tail))
    mask = _mask(mask_name, K, N)
    maps = ((0, 1),)

    # the reference: autograd through the forward restatement
    o_ref = obs.clone().requires_grad_()
    tf = (truth, mask, maps) if mask is not None else ()
    want = strided_reference(lambda k, x: (x.reshape(N, -1) @ Ms[k]).reshape(x.shape), o_ref, T, H, S, *tf)
    if mask is None or mask_name == "zero":  # predict's chain, with the window counter riding in the forward
        count = [0]

        def counted(x):
            count[0] += 1
            return (x.reshape(N, -1) @ Ms[count[0] - 1].detach()).reshape(x.shape)

        assert torch.equal(want.detach(), predict_strided_reference(counted, obs, T, H, S)) and count[0] == K
    want.backward(dout)

    loop = StridedLoop(lambda k, x: (x.reshape(N, -1) @ Ls[k]).reshape(x.shape), obs, T, H, S,
                       truth if mask is not None else None, mask, maps)
    assert torch.equal(loop.out, want.detach())
    dobs = loop.backward(dout, Ls)

    def close(got, ref, what):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (what, Tin, Tout, S, H, mask_name)

    assert float(o_ref.grad.abs().max()) > 0
    close(dobs, o_ref.grad, "observed.grad")
    for k in range(K):
        close(Ls[k].grad, Ms[k].grad, f"map {k}")
    if mask_name == "one" and K > 1:  # observed.grad is window 0's alone
        o0 = obs.clone().requires_grad_()
        y0 = (o0[:, [min(s, Tin - 1) for s in range(T)]].reshape(N, -1) @ Ms[0].detach()).reshape(N, T, *tail)
        y0[:, Tin:Tin + S].backward(dout[:, :S])
        close(dobs, o0.grad, "window 0 alone")


@pytest.mark.parametrize("Tin,Tout,S,H", CASES)
def test_glue_restatement_is_the_loop_in_fp32(Tin, Tout, S, H):
    """glue_dy / glue_acc on float32 arrays against StridedLoop's backward with an
    identity forward per window (dx_k = dy_k): the same sums in the same order,
    equal bit for bit, under a mixed mask."""
    T, N, tail = Tin + Tout, 4, (5, 3)
    K = windows(H, S)
    rng = np.random.default_rng(7 + 10 * Tin + S)
    scale = [torch.tensor(float(1 + k)) for k in range(K)]
    obs = torch.from_numpy(rng.standard_normal((N, Tin) + tail).astype(np.float32))
    truth = torch.from_numpy(rng.standard_normal((N, Tin + H) + tail).astype(np.float32))
    dout = rng.standard_normal((N, H) + tail).astype(np.float32)
    mask = _mask("mixed", K, N)
    loop = StridedLoop(lambda k, x: x * scale[k], obs, T, H, S, truth, mask)
    dobs = loop.backward(torch.from_numpy(dout))
    Gh = np.zeros((N, Tin + H) + tail, np.float32)
    for k in range(K - 1, -1, -1):
        dy = glue_dy(Gh, dout, T, Tin, S, k)
        assert not dy[:, :Tin].any() and not dy[:, Tin + S:].any()
        Gh = glue_acc(Gh, dy * np.float32(1 + k), mask[k].numpy(), T, Tin, S, k)
    assert np.array_equal(Gh[:, :Tin], dobs.numpy())
