"""Host-side checks of predict with a stride (include/ext/dstd_gcn_stride.h,
dstd_native.ext_stride, DSTDGCN.predict(stride=), PredictionEngine.test /
test_groups(stride=)) and of the restatement the GPU tests compare against
(tests/stride_helper.py).  No GPU needed: the entry point's refusals come before
any HIP call, and the Python refusals before anything touches a device."""
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
from model import dstdgcn_fast as F
from model import get_model
from predict_helper import predict_reference
from stride_helper import predict_strided_reference
from test_taps_host import FAKE, H36M, _model_params

EINVAL, EWORKSPACE, ELIMIT = -1, -2, -3  # include/dstd_gcn.h
BIG = 1 << 40
HEADER = "ext/dstd_gcn_stride.h"
NAMES = ("dstd_model_predict_strided_workspace_bytes", "dstd_model_predict_strided")


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", *HEADER.split("/"))).read()


# ---- the restatement: equivalence ---------------------------------------------------
@pytest.mark.parametrize("Tin,Tout", [(2, 4), (3, 3), (4, 2), (5, 1), (1, 5)])
def test_stride_of_a_whole_window_is_predict_reference(Tin, Tout):
    """S = Tout: the chain of include/dstd_gcn_predict.h, frame for frame, under
    a forward that mixes every frame of its window (random fp64 data; the two
    loops hand the forward identical windows, so the results are equal in bits)."""
    T = Tin + Tout
    rng = np.random.default_rng(10 * Tin + Tout)
    W = rng.normal(size=(T, T))
    c = rng.normal(size=(T, 1, 1))
    obs = rng.normal(size=(3, Tin, 4, 3))

    def forward(x):
        return np.tanh(np.einsum("st,btvc->bsvc", W, x) + c)

    for H in (1, Tout, Tout + 1, 3 * Tout + 1):
        want = predict_reference(forward, obs, T, H)
        got = predict_strided_reference(forward, obs, T, H, Tout)
        assert got.shape == (3, H, 4, 3) and np.array_equal(got, want), (Tin, Tout, H)
        got_t = predict_strided_reference(lambda x: torch.from_numpy(forward(x.numpy())), torch.from_numpy(obs), T, H,
                                          Tout)
        assert np.array_equal(got_t.numpy(), want)


# ---- the restatement: bookkeeping ---------------------------------------------------
def _coef(T):
    """c[s][t] = 1 + s * T + t (every pair distinct) and d[s] = 7 * s + 3: output
    frame s depends on every frame of the window, each with a coefficient of
    its own, and on s."""
    s, t = np.arange(T).reshape(T, 1), np.arange(T).reshape(1, T)
    return 1 + s * T + t, 7 * np.arange(T) + 3


CASES = [(4, 2, 1, 5),   # S = 1 < Tin: windows read obs, older out and the newest frame together
         (2, 4, 3, 10),  # S > Tin, H no multiple of S
         (3, 3, 2, 7),   # S < Tin, H no multiple of S
         (1, 5, 2, 9),   # a single observed frame
         (5, 1, 1, 4),
         (2, 4, 4, 9),   # S = Tout
         (3, 3, 2, 1),   # H < S
         (3, 3, 3, 2),   # H < S = Tout
         (2, 4, 2, 8)]   # S = Tin, H a multiple of S


@pytest.mark.parametrize("Tin,Tout,S,H", CASES)
def test_restatement_against_a_per_frame_recursion(Tin, Tout, S, H):
    """Against a recursion that shares none of the loop's bookkeeping: with the
    known sequence h (obs, then out), output frame f = k * S + j is

        h[Tin + f] = d[Tin + j] + sum_t c[Tin + j][t] * h[k * S + min(t, Tin - 1)]

    computed one frame and one sample element at a time on Python integers.
    The fp64 loop works on integer-valued data below 2^53, so it is exact: an
    off-by-one in k * S + m(s), or emitting another slice of y_k, changes the
    result."""
    T = Tin + Tout
    c, d = _coef(T)
    rng = np.random.default_rng(1000 * Tin + 100 * Tout + 10 * S + H)
    obs = rng.integers(-5, 6, size=(2, Tin, 3, 3))

    def forward(x):
        return np.einsum("st,btvc->bsvc", c.astype(np.float64), x) + d.astype(np.float64).reshape(1, T, 1, 1)

    got = predict_strided_reference(forward, obs.astype(np.float64), T, H, S)
    assert got.shape == (2, H, 3, 3) and got.dtype == np.float64
    want = np.empty((2, H, 3, 3), dtype=object)
    for b, v, a in np.ndindex(2, 3, 3):
        h = [int(z) for z in obs[b, :, v, a]]
        for f in range(H):
            k, j = divmod(f, S)
            h.append(int(d[Tin + j]) + sum(int(c[Tin + j][t]) * h[k * S + min(t, Tin - 1)] for t in range(T)))
        want[b, :, v, a] = h[Tin:]
    assert max(abs(z) for z in want.flat) < 2 ** 53  # every sum of the fp64 forward is exact
    assert np.array_equal(got, want.astype(np.float64)), (Tin, Tout, S, H)
    got_t = predict_strided_reference(lambda x: torch.from_numpy(forward(x.numpy())),
                                      torch.from_numpy(obs.astype(np.float64)), T, H, S)
    assert np.array_equal(got_t.numpy(), got)


def test_restatement_refuses_a_stride_outside_the_window():
    obs = np.zeros((1, 2, 1, 3))
    for S in (0, 5, -1):
        with pytest.raises(AssertionError):
            predict_strided_reference(lambda x: x, obs, 6, 3, S)


# ---- header and binding -------------------------------------------------------------
def test_binding_agrees_with_the_stride_header(header):
    assert compare({HEADER: header}, native.ext_stride) == []
    defines, structs, callbacks, protos = parse(header)
    assert sorted(protos) == sorted(NAMES) and native.ext_stride.STRIDE_EXPORTS == NAMES
    ret, params = protos["dstd_model_predict_strided"]
    assert ret == ("int", 0)
    assert [p[2] for p in params] == ["p", "obs", "B", "input_n", "horizon", "stride", "out", "workspace",
                                      "workspace_bytes", "stream", "flags"]
    assert [(p[0], p[1]) for p in params] == [
        ("dstd_model_params", 1), ("float", 1), ("int", 0), ("int", 0), ("int", 0), ("int", 0), ("float", 1),
        ("void", 1), ("size_t", 0), ("void", 1), ("unsigned int", 0)]
    ret, params = protos["dstd_model_predict_strided_workspace_bytes"]
    assert ret == ("size_t", 0) and [(p[0], p[1]) for p in params] == [("int", 0)] * 5
    i, u, z, p = ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.c_void_p
    assert native.ext_stride.ABI == {HEADER: {NAMES[0]: (z, [i] * 5), NAMES[1]: (i, [p, p, i, i, i, i, p, p, z, p, u])}}
    # no typedef and no constant of its own: the window cap stays the predict header's, at 64
    assert (defines, structs, callbacks) == ({}, {}, {}) and native.ext_stride.C_TYPES == {}
    assert '#include "../dstd_gcn_predict.h"' in header and "typedef" not in header
    assert native.PREDICT_MAX_WINDOWS == 64


def test_an_altered_stride_header_is_reported_by_name(header):
    for old, new in (("int stride, ", ""), ("size_t workspace_bytes, void* stream", "int workspace_bytes, void* stream"),
                     ("int horizon,\n", "long long horizon,\n")):
        assert old in header
        reports = compare({HEADER: header.replace(old, new, 1)}, native.ext_stride)
        assert {r.split(":")[0] for r in reports} == {"dstd_model_predict_strided"}, reports


def test_library_exports_both_symbols_and_the_other_tables_are_as_they_were():
    L = native.lib()
    for name in NAMES:
        restype, argtypes = native.ext_stride.ABI[HEADER][name]
        fn = getattr(L, name)  # exported, and declared by lib()
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes)
    # a table of its own: nothing added to the pinned ones
    assert set(native.ext.ALL) == {"ext/dstd_gcn_rollout.h", "ext/dstd_gcn_teacher.h"}
    assert sum(len(t) for t in native.ext.ALL.values()) == 10
    assert set(native.ext.ABI) == {"ext/dstd_gcn_rollout.h"} and len(native.ext.ABI["ext/dstd_gcn_rollout.h"]) == 6
    assert list(native.ext_eval.ABI) == ["ext/dstd_gcn_eval.h"] and len(native.ext_eval.ABI["ext/dstd_gcn_eval.h"]) == 1
    assert list(native.ext_augment.ABI) == ["ext/dstd_gcn_augment.h"]
    assert len(native.ext_augment.ABI["ext/dstd_gcn_augment.h"]) == 1
    assert set(abi.ABI) == {"dstd_gcn.h", "dstd_gcn_train.h", "dstd_gcn_aux.h", "dstd_gcn_loss.h", "dstd_gcn_taps.h",
                            "dstd_gcn_data.h", "dstd_gcn_predict.h"}
    assert sum(len(t) for t in abi.ABI.values()) == 61 and len(abi.C_TYPES) == 15
    others = (*abi.ABI.values(), *native.ext.ALL.values(), *native.ext_eval.ABI.values(),
              *native.ext_augment.ABI.values())
    assert not any(name in t for t in others for name in NAMES)
    assert native.ext_stride.model_params_ref is native.ext.model_params_ref
    mk = open(os.path.join(ROOT, "dstd-gcn_amd", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "csrc/dstd_predict_stride.hip" in srcs and "csrc/dstd_predict.hip" in srcs
    assert L.dstd_source_hash().decode() == native.source_hash()  # the new sources are hashed


def test_a_library_without_the_symbols_is_a_load_error():
    extra = {**native.ext.ALL, **native.ext_eval.ABI, **native.ext_augment.ABI, **native.ext_stride.ABI}
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


# ---- refusals of the entry point ----------------------------------------------------
def _strided(L, p, obs=FAKE, B=2, Tin=10, H=25, S=10, out=FAKE, ws=FAKE, nbytes=BIG, flags=0):
    ref = native.ext_stride.model_params_ref(p) if p is not None else None
    return L.dstd_model_predict_strided(ref, obs, B, Tin, H, S, out, ws, nbytes, None, flags)


def test_workspace_is_the_forwards_plus_two_windows():
    L = native.lib()
    for B, T, V, C, layers in ((3, 35, 22, 64, 5), (2, 6, 5, 8, 1), (256, 75, 22, 64, 5)):
        model_bytes = L.dstd_model_workspace_bytes(B, T, V, C, layers)
        window = -(-12 * B * T * V // 256) * 256
        got = L.dstd_model_predict_strided_workspace_bytes(B, T, V, C, layers)
        assert got == -(-model_bytes // 256) * 256 + 2 * window
        assert got == L.dstd_model_predict_workspace_bytes(B, T, V, C, layers) - window


def test_strided_predict_refuses_bad_arguments_without_gpu():
    """Every refusal returns before anything is dereferenced or launched (the
    pointers are fake), in the order of dstd_model_predict.  A call that passes
    the argument and envelope checks shows as DSTD_EWORKSPACE on a one-byte
    workspace."""
    L = native.lib()
    p = _model_params(35, 22, layers=5)
    assert _strided(L, None) == EINVAL
    assert _strided(L, p, obs=None) == EINVAL
    assert _strided(L, p, out=None) == EINVAL
    assert _strided(L, p, ws=None) == EINVAL
    for Tin in (0, 35, 36):
        assert _strided(L, p, Tin=Tin, S=1) == EINVAL
    for H in (0, -3):
        assert _strided(L, p, H=H) == EINVAL
    for S in (0, -1, 26, 1 << 30):
        assert _strided(L, p, S=S) == EINVAL, S
    for S in (1, 10, 25):
        assert _strided(L, p, S=S, nbytes=1) == EWORKSPACE, S
    assert _strided(L, p, Tin=34, S=2) == EINVAL and _strided(L, p, Tin=34, S=1, H=3, nbytes=1) == EWORKSPACE
    for bad in (128, 256, 1 << 31, 2 | 512):
        assert _strided(L, p, flags=bad) == EINVAL, bad
    for ok in (0, 1, 2, 4, 8, 16, 32, 64, 127):  # exactly the flags of dstd_model_fwd_ex
        assert _strided(L, p, flags=ok, nbytes=1) == EWORKSPACE, ok
    # the window cap: 64 windows of S frames pass, one frame more does not; H = 100 needs S >= 2
    for S in (1, 2, 10, 25):
        assert _strided(L, p, S=S, H=64 * S + 1) == ELIMIT
        assert _strided(L, p, S=S, H=64 * S, nbytes=1) == EWORKSPACE
    assert _strided(L, p, S=1, H=100) == ELIMIT and _strided(L, p, S=2, H=100, nbytes=1) == EWORKSPACE
    assert _strided(L, p, S=1, H=2 ** 31 - 1) == ELIMIT  # K is counted beyond an int
    # a bad stride is an argument: EINVAL before the cap's ELIMIT and the shape's
    assert _strided(L, p, S=0, H=10 ** 6) == EINVAL
    assert _strided(L, _model_params(129, 22), S=200) == EINVAL
    # the model's shape, as dstd_model_fwd_ex judges it
    assert _strided(L, _model_params(129, 22)) == ELIMIT
    assert _strided(L, _model_params(35, 33)) == ELIMIT
    assert _strided(L, _model_params(35, 22, C=65)) == ELIMIT
    assert _strided(L, _model_params(35, 22, layers=17)) == EINVAL
    assert _strided(L, p, B=0) == EINVAL
    q = _model_params(35, 22, layers=5)
    q.enc[3].conv_t.wrm = None  # a parameter pointer: refused here, not by window 0's forward
    assert _strided(L, q) == EINVAL
    # the workspace, last
    need = L.dstd_model_predict_strided_workspace_bytes(2, 35, 22, 64, 5)
    assert _strided(L, p, nbytes=need - 1) == EWORKSPACE
    assert _strided(L, p, nbytes=L.dstd_model_workspace_bytes(2, 35, 22, 64, 5)) == EWORKSPACE
    with pytest.raises(TypeError, match="ModelParams"):
        native.ext_stride.model_params_ref(object())


# ---- refusals of the Python surface -------------------------------------------------
@pytest.mark.parametrize("cls", ["reference layout", "channels-last"])
def test_predict_refuses_a_bad_stride_on_a_cpu_model(cls):
    m = get_model("dstdgcn", dstdgcn=H36M) if cls == "reference layout" else F.DSTDGCN(**H36M)
    m.eval()
    obs = torch.zeros(2, 10, 22, 3)
    for bad in (0, 26, -1, 2.5, True, "10", 10.0, np.float32(3)):
        with pytest.raises(ValueError, match="stride"):
            m.predict(obs, 53, stride=bad)
    if cls == "reference layout":  # (the channels-last model asks for the device before its shadow sees the horizon)
        # too many windows, with the smallest stride that fits
        with pytest.raises(ValueError, match=r"stride >= 2\b"):
            m.predict(obs, 100, stride=1)
        with pytest.raises(ValueError, match=r"stride >= 16\b"):
            m.predict(obs, 1000, stride=10)
        with pytest.raises(ValueError, match="windows"):  # no stride of this model fits: said as before
            m.predict(obs, 64 * 25 + 1, stride=5)
        with pytest.raises(ValueError, match="horizon"):
            m.predict(obs, 0, stride=5)
    # a valid stride goes on to the device: there is no CPU path (numpy integers count as integers)
    for ok in (1, 10, 25, None, np.int64(5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.predict(obs, 53, stride=ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(obs, 64, stride=1)  # 64 windows exactly
    # the training-mode error is unchanged, and comes first
    for stride in (None, 10, 0):
        with pytest.raises(RuntimeError, match=r"^DSTDGCN\.predict rolls the eval forward out: call \.eval\(\) first$"):
            m.train().predict(obs, 53, stride=stride)


class _Log:
    def info(self, *a, **k):
        pass


def _engine():
    from engine.prediction import PredictionEngine
    opts = dict(input_channels=6, input_time_frame=2, output_time_frame=2, st_gcnn_dropout=0.1, joints_to_consider=22,
                num_feature=8, num_layers=1, layout="h36m")
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5), loss=dict(joint=["jl2", 1]),
               n_out=1, transform="tsc", use_weight=False, inverse=True)
    return PredictionEngine(cfg, get_model("dstdgcn", dstdgcn=opts), _Log())


def test_engine_refuses_a_stride_without_a_horizon():
    from dstd_data import DeviceLoader, DeviceSequences
    eng = _engine()
    batch = (torch.zeros(2, 4, 66), None, None, torch.zeros(2, 4, 96))
    with pytest.raises(ValueError, match="stride.*horizon"):
        eng.test([batch], input_n=2, eval_frame=[0, 1], stride=1)
    windows = np.random.default_rng(0).normal(size=(3, 4, 96))
    s = DeviceSequences.from_windows(windows, list(range(66)), 2, 2, device="cpu", groups=[0, 1, 1])
    with pytest.raises(ValueError, match="stride.*horizon"):
        eng.test_groups(DeviceLoader(s, 2), input_n=2, eval_frame=[0, 1], stride=1)
