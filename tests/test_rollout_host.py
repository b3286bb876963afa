"""Host-side checks of training through the rollout (include/ext/dstd_gcn_rollout.h,
dstd_native.ext, DSTDGCN.rollout) and of the restatements the GPU tests compare
against (no GPU needed)."""
import os
import re

import numpy as np
import pytest
import torch

import dstd_native as native
from abi_reader import compare, parse
from conftest import ROOT
from guard_helper import rup
from model import dstdgcn_fast as F
from model import get_model
from predict_helper import predict_reference
from rollout_helper import _Pad, _Roll, glue_dy, glue_fold, glue_obs, rollout_backward, rollout_loop, windows
from test_taps_host import FAKE, H36M, _fake, _model_params

EINVAL, EWORKSPACE, ELIMIT = -1, -2, -3  # include/dstd_gcn.h
BIG = 1 << 40
HEADER = "ext/dstd_gcn_rollout.h"
SHAPES = [(5, 1), (1, 5), (3, 3), (4, 2)]  # (Tin, Tout): pad sums, no observed frame carried over, both, a fold


def horizons(Tout):
    return sorted({1, Tout, Tout + 1, 3 * Tout - 1})


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", *HEADER.split("/"))).read()


# ---- the binding -----------------------------------------------------------------
def test_binding_agrees_with_the_extension_header(header):
    assert compare({HEADER: header}, native.ext) == []
    protos = parse(header)[3]
    assert sorted(protos) == sorted(native.ext.ROLLOUT_EXPORTS) and len(protos) == 6
    assert parse(header)[:3] == ({}, {}, {})  # no define, no struct, no callback: the freeze of test_abi_host.py
    assert native.ext.C_TYPES == {} and set(native.ext.ABI) == {HEADER}


@pytest.mark.parametrize("what,marker,old,new,name", [
    ("parameter dropped", "int dstd_model_rollout_bwd(", "float* dobs, ", "", "dstd_model_rollout_bwd"),
    ("type changed", "int dstd_model_rollout_fwd(", "int horizon", "size_t horizon", "dstd_model_rollout_fwd"),
    ("prototype added", "size_t dstd_model_rollout_workspace_bytes(", "size_t dstd_model_rollout_workspace_bytes(",
     "int dstd_model_rollout_new(int B);\nsize_t dstd_model_rollout_workspace_bytes(", "dstd_model_rollout_new"),
])
def test_an_altered_extension_header_is_reported_by_name(header, what, marker, old, new, name):
    at = header.index(marker)
    assert old in header[at:]
    altered = header[:at] + header[at:].replace(old, new, 1)
    reports = compare({HEADER: altered}, native.ext)
    assert {r.split(":")[0] for r in reports} == {name}, reports


def test_extension_stays_out_of_the_frozen_tables():
    """dstd_native.ext is a name of the package, not star-imported into it, and
    adds nothing to abi.ABI / abi.C_TYPES; lib() declared its table all the same."""
    from dstd_native import abi
    for name in native.ext.ROLLOUT_EXPORTS:
        assert not any(name in table for table in abi.ABI.values()), name
    assert not hasattr(native, "ROLLOUT_EXPORTS") and HEADER not in native.ABI
    L = native.lib()
    for name, (restype, argtypes) in native.ext.ABI[HEADER].items():
        fn = getattr(L, name)  # the library exports it
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert native.ext.ROLLOUT_EXPORTS[:4] == ("dstd_model_rollout_saved_bytes", "dstd_model_rollout_workspace_bytes",
                                              "dstd_model_rollout_fwd", "dstd_model_rollout_bwd")


def test_a_missing_extension_symbol_is_an_error_unless_the_library_is_foreign_on_purpose():
    class Lib:  # every symbol of the frozen table, none of the extension's
        _name = "libold.so"

        def __getattr__(self, name):
            if name.startswith("dstd_model_rollout"):
                raise AttributeError(name)
            fn = type("Fn", (), {})()
            setattr(self, name, fn)
            return fn

    with pytest.raises(RuntimeError, match=r"libold\.so does not export dstd_model_rollout_saved_bytes \(ext/"):
        native.declare(Lib(), extra=native.ext.ABI)
    native.declare(Lib(), allow_missing=True, extra=native.ext.ABI)


def test_source_hash_covers_the_extension_header():
    mk = open(os.path.join(ROOT, "dstd-gcn_amd", "Makefile")).read()
    assert re.search(r"^HASHED := .*\.\./include/ext/\*\.h", mk, re.M) and "csrc/dstd_rollout.hip" in mk
    assert native.lib().dstd_source_hash().decode() == native.source_hash()


# ---- sizes -------------------------------------------------------------------------
def test_sizes_are_the_stated_closed_forms():
    """H36M, B = 3, K = 4.  saved: the forward's y scratch, then per window x_k and
    the model's saved region; workspace: the model backward's, then dy and the two
    G buffers -- every part rounded up to 256 bytes."""
    L = native.lib()
    B, T, V, C, layers, K = 3, 35, 22, 64, 5, 4
    W = rup(12 * B * T * V, 256)
    S = rup(L.dstd_model_train_saved_bytes(B, T, V, C, layers), 256)
    M = rup(L.dstd_model_train_workspace_bytes(B, T, V, C, layers), 256)
    assert (W, S, M) == (27904, 56400128, 22648832)
    assert L.dstd_model_rollout_saved_bytes(B, T, V, C, layers, K) == W + K * (W + S) == 225740032
    assert L.dstd_model_rollout_workspace_bytes(B, T, V, C, layers) == M + 3 * W == 22732544
    assert L.dstd_model_rollout_saved_bytes(B, T, V, C, layers, 0) == W
    assert L.dstd_model_rollout_saved_bytes(B, T, V, C, layers, -2) == W


# ---- refusals ----------------------------------------------------------------------
def _grads():
    return _fake(native.ModelGrads())


def _fwd(L, p, obs=FAKE, B=2, Tin=10, H=25, drop=0.0, seeds=None, out=FAKE, saved=FAKE, nbytes=BIG, flags=0):
    ref = None if p is None else native.ext.model_params_ref(p)
    return L.dstd_model_rollout_fwd(ref, obs, B, Tin, H, 0.1, drop, seeds, out, saved, nbytes, None, flags)


def _bwd(L, p, B=2, Tin=10, H=25, drop=0.0, seeds=None, saved=FAKE, nbytes=BIG, dout=FAKE, g="fake", dobs=FAKE,
         ws=FAKE, wbytes=BIG, flags=0):
    ref = None if p is None else native.ext.model_params_ref(p)
    gref = None if g is None else native.ext.model_grads_ref(_grads() if g == "fake" else g)
    return L.dstd_model_rollout_bwd(ref, B, Tin, H, drop, seeds, saved, nbytes, dout, gref, dobs, ws, wbytes, None,
                                    flags)


def _bwd_window(L, p, k=0, **kw):
    """_bwd through dstd_model_rollout_bwd_window at window k."""
    class OneWindow:
        def dstd_model_rollout_bwd(self, ref, B, Tin, H, *rest):
            return L.dstd_model_rollout_bwd_window(ref, B, Tin, H, k, *rest)

    return _bwd(OneWindow(), p, **kw)


def test_rollout_refuses_bad_arguments_without_gpu():
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
        assert call(L, p, Tin=0) == EINVAL
        assert call(L, p, Tin=35) == EINVAL  # input_n >= T
        assert call(L, p, Tin=36) == EINVAL
        assert call(L, p, H=0) == EINVAL
        assert call(L, p, H=-3) == EINVAL
        assert call(L, p, drop=0.1, seeds=None) == EINVAL  # a mask needs its seeds
        assert call(L, p, drop=1.0, seeds=FAKE, flags=4) == EINVAL
        assert call(L, p, drop=-0.5, flags=4) == EINVAL
        for bad in (16, 32, 1 << 31, 2 | 64):
            assert call(L, p, flags=bad) == EINVAL, bad
        for ok in (0, 1, 2, 8, 1 | 2, 2 | 8, 1 | 2 | 8):  # exactly the flags of dstd_model_train_fwd_ex ...
            assert call(L, p, flags=ok, nbytes=1) == EWORKSPACE, ok
        assert call(L, p, drop=0.1, seeds=FAKE, flags=4 | 2, nbytes=1) == EWORKSPACE  # ... DSTD_TRAIN_SEED_DEVICE too
        assert call(L, p, B=3, flags=2) == EINVAL  # an odd pair
        assert call(L, p, B=0) == EINVAL
        assert call(L, _model_params(35, 0, layers=5)) == EINVAL
        assert call(L, _model_params(35, 22, layers=17)) == EINVAL
        q = _model_params(35, 22, layers=5)
        q.enc[3].conv_t.wrm = None  # a parameter pointer: refused here, not by window 0
        assert call(L, q) == EINVAL
        # an argument error wins over the window cap, the window cap over the sizes
        assert call(L, p, H=64 * 25 + 1, flags=16) == EINVAL
        for Tin in (10, 34, 1):
            Tout = 35 - Tin
            assert call(L, p, Tin=Tin, H=64 * Tout + 1, nbytes=1) == ELIMIT
            assert call(L, p, Tin=Tin, H=64 * Tout, nbytes=1) == EWORKSPACE
        # the model's envelope, as dstd_model_train_fwd_ex judges it
        assert call(L, _model_params(129, 22), Tin=10) == ELIMIT
        assert call(L, _model_params(35, 33), Tin=10) == ELIMIT
        # saved, below the export for this horizon's windows (25 frames: 1, 26: 2)
        need = L.dstd_model_rollout_saved_bytes(2, 35, 22, 64, 5, 1)
        assert call(L, p, nbytes=need - 1) == EWORKSPACE
        assert call(L, p, H=26, nbytes=need) == EWORKSPACE
        assert call(L, p, H=26, nbytes=L.dstd_model_rollout_saved_bytes(2, 35, 22, 64, 5, 2) - 1) == EWORKSPACE
    # the window of a one-window backward: 0 .. K-1
    assert _bwd_window(L, p, k=-1) == EINVAL
    assert _bwd_window(L, p, k=1) == EINVAL  # 25 frames: one window
    assert _bwd_window(L, p, k=1, H=26, nbytes=1) == EWORKSPACE
    assert _bwd_window(L, p, k=2, H=26) == EINVAL
    assert _bwd_window(L, p, k=65, H=64 * 25 + 1) == EINVAL  # an argument error wins over the window cap
    assert _bwd_window(L, p, k=3, H=64 * 25 + 1) == ELIMIT
    # each direction's own pointers
    assert _fwd(L, p, obs=None) == EINVAL
    assert _fwd(L, p, out=None) == EINVAL
    assert _bwd(L, p, dout=None) == EINVAL
    assert _bwd(L, p, g=None) == EINVAL
    assert _bwd(L, p, ws=None) == EINVAL
    g = _grads()
    g.enc[2].conv_s[1].bm2 = None
    assert _bwd(L, p, g=g) == EINVAL
    # the backward's workspace comes after saved
    assert _bwd(L, p, nbytes=1, wbytes=1) == EWORKSPACE
    assert _bwd(L, p, wbytes=L.dstd_model_rollout_workspace_bytes(2, 35, 22, 64, 5) - 1) == EWORKSPACE
    assert _bwd(L, p, wbytes=L.dstd_model_train_workspace_bytes(2, 35, 22, 64, 5)) == EWORKSPACE
    with pytest.raises(TypeError, match="expected ModelParams"):
        native.ext.model_params_ref(_grads())


def test_glue_hook_refuses_bad_arguments_without_gpu():
    L = native.lib()

    def hook(step=0, dout=FAKE, Gn=FAKE, dst=FAKE, B=3, T=6, Tin=4, V=22, H=5, k=0):
        return L.dstd_model_rollout_glue_bwd(step, dout, Gn, dst, B, T, Tin, V, H, k, None)

    assert hook(dst=None) == EINVAL
    assert hook(step=0, dout=None) == EINVAL
    assert hook(step=1, Gn=None) == EINVAL
    assert hook(step=2, Gn=None) == EINVAL
    assert hook(step=3) == EINVAL and hook(step=-1) == EINVAL
    assert hook(B=0) == EINVAL and hook(V=0) == EINVAL
    assert hook(Tin=0) == EINVAL and hook(Tin=6) == EINVAL and hook(H=0) == EINVAL
    assert hook(k=-1) == EINVAL and hook(k=3) == EINVAL  # H = 5, Tout = 2: windows 0 .. 2
    assert hook(step=1, Tin=3) == 0  # nothing carried over: no launch


def test_rollout_method_refusals():
    m = get_model("dstdgcn", dstdgcn=H36M)
    obs = torch.zeros(2, 10, 22, 3)
    for mode in (m.train, m.eval):
        mode()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.rollout(obs)
        with pytest.raises(AssertionError):
            m.rollout(torch.zeros(2, 35, 22, 3))  # a window, not observations
        with pytest.raises(ValueError, match="expected"):
            m.rollout(torch.zeros(2, 10, 21, 3))
        with pytest.raises(ValueError, match="horizon"):
            m.rollout(obs, 0)
        with pytest.raises(ValueError, match="windows"):
            m.rollout(obs, 64 * 25 + 1)
    m.train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.rollout_pair(obs, obs)
    with pytest.raises(ValueError, match="windows"):
        m.rollout_pair(obs, obs, 64 * 25 + 1)

    class Sub(torch.Tensor):
        pass

    with pytest.raises(RuntimeError, match="eager only"):
        m.rollout(obs.as_subclass(Sub))
    m._dstd_bn_sync = object()  # what dstd_dist.convert_sync_batchnorm installs
    try:
        with pytest.raises(NotImplementedError, match="cross-rank BatchNorm"):
            m.rollout(obs)
        with pytest.raises(NotImplementedError, match="cross-rank BatchNorm"):
            m.rollout_pair(obs, obs)
    finally:
        del m._dstd_bn_sync
    assert not hasattr(F.DSTDGCN, "rollout")  # the channels-last model has none


# ---- the restatements --------------------------------------------------------------
def _linear(T, feat, seed):
    """A fixed random linear map over (frame, feature) as the window forward."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T * feat, T * feat)) / np.sqrt(T * feat)


@pytest.mark.parametrize("Tin,Tout", SHAPES)
def test_closed_form_is_autograd_of_the_forward_restatement(Tin, Tout):
    """The backward restated in numpy fp64 against torch autograd through
    predict_reference (indexing and concatenation only), with y = x M as every
    window's forward: the vector-Jacobian product is dy M^T."""
    T, N, tail = Tin + Tout, 3, (2, 3)
    M = _linear(T, 6, 10 * Tin + Tout)
    Mt = torch.from_numpy(M)
    rng = np.random.default_rng(7)
    for H in horizons(Tout):
        obs = torch.from_numpy(rng.standard_normal((N, Tin) + tail)).requires_grad_()
        dout = rng.standard_normal((N, H) + tail)
        out = predict_reference(lambda x: (x.reshape(N, -1) @ Mt).reshape(x.shape), obs, T, H)
        out.backward(torch.from_numpy(dout))
        got = rollout_backward(dout, T, Tin, lambda k, dy: (dy.reshape(N, -1) @ M.T).reshape(dy.shape))
        assert got.shape == obs.shape
        assert float(np.abs(got - obs.grad.numpy()).max()) <= 1e-12, (Tin, Tout, H)


@pytest.mark.parametrize("Tin,Tout", SHAPES)
def test_loop_glue_is_the_restatement_in_fp32(Tin, Tout):
    """rollout_loop's autograd Functions against the numpy steps on float32:
    the same sums in the same order, so equal bit for bit -- and the loop's
    forward is predict_reference's."""
    T, N, tail = Tin + Tout, 3, (5, 3)
    rng = np.random.default_rng(100 * Tin + Tout)
    M = torch.from_numpy(_linear(T, 15, 3).astype(np.float32))

    def forward(x):
        return (x.reshape(N, -1) @ M).reshape(x.shape)

    for H in horizons(Tout):
        K = windows(T, Tin, H)
        obs = torch.from_numpy(rng.standard_normal((N, Tin) + tail).astype(np.float32)).requires_grad_()
        out = rollout_loop(None, obs, H, forward=forward, T=T)
        with torch.no_grad():
            assert torch.equal(out, predict_reference(forward, obs, T, H))
        dout = rng.standard_normal((N, H) + tail).astype(np.float32)
        out.backward(torch.from_numpy(dout))
        vjp = lambda k, dy: (torch.from_numpy(dy).reshape(N, -1) @ M.T).reshape(dy.shape).numpy()  # noqa: E731
        assert np.array_equal(rollout_backward(dout, T, Tin, vjp), obs.grad.numpy()), (Tin, Tout, H)
        # the Functions one at a time, on random gradients
        Gn = rng.standard_normal((N, T) + tail).astype(np.float32)
        for k in range(K):
            last, take = k == K - 1, min(Tout, H - k * Tout)
            x = torch.zeros((N, T) + tail, requires_grad=True)
            y = torch.zeros((N, T) + tail, requires_grad=True)
            o, xn = _Roll.apply(x, y, Tin, take, last)
            d_o = torch.from_numpy(dout[:, k * Tout:k * Tout + take])
            if last:
                o.backward(d_o)
            else:
                torch.autograd.backward([o, xn], [d_o, torch.from_numpy(Gn)])
            assert np.array_equal(y.grad.numpy(), glue_dy(dout, None if last else Gn, T, Tin, k))
            want = glue_fold(np.zeros_like(Gn), None if last else Gn, T, Tin)
            assert np.array_equal(x.grad.numpy(), want)
        o = torch.zeros((N, Tin) + tail, requires_grad=True)
        _Pad.apply(o, T).backward(torch.from_numpy(Gn))
        assert np.array_equal(o.grad.numpy(), glue_obs(Gn, T, Tin))
