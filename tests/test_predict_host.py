"""Host-side checks of the rollout entry point (include/dstd_gcn_predict.h,
DSTDGCN.predict) and of the restatement the GPU tests compare against (no GPU
needed)."""
import numpy as np
import pytest
import torch

import dstd_native as native
from conftest import group, load_npz
from guard_helper import rup
from model import dstdgcn_fast as F
from model import get_model
from oracle import dstdgcn_oracle as O
from predict_helper import predict_reference
from test_taps_host import FAKE, H36M, _model_params, header_symbols

EINVAL, EWORKSPACE, ELIMIT = -1, -2, -3  # include/dstd_gcn.h
BIG = 1 << 40


def test_library_exports_every_predict_header_symbol():
    L = native.lib()
    syms = header_symbols("dstd_gcn_predict.h")
    assert syms == ["dstd_model_predict", "dstd_model_predict_workspace_bytes"], syms
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(native.PREDICT_EXPORTS)


def test_predict_workspace_is_the_forwards_plus_three_windows():
    """H36M, B = 3: the model forward's region rounded up to 256 bytes, then two
    window buffers and one y buffer of 12 * B * T * V bytes, each rounded up."""
    L = native.lib()
    B, T, V = 3, 35, 22
    model_bytes = L.dstd_model_workspace_bytes(B, T, V, 64, 5)
    got = L.dstd_model_predict_workspace_bytes(B, T, V, 64, 5)
    assert got == rup(model_bytes, 256) + 3 * rup(12 * B * T * V, 256)
    assert rup(12 * B * T * V, 256) == 27904
    assert got == 3774976, got


def _predict(L, p, obs=FAKE, B=2, Tin=10, H=25, out=FAKE, ws=FAKE, nbytes=BIG, flags=0):
    return L.dstd_model_predict(p, obs, B, Tin, H, out, ws, nbytes, None, flags)


def test_predict_refuses_bad_arguments_without_gpu():
    """Every refusal returns before anything is dereferenced or launched (the
    pointers are fake).  A call that passes the argument and envelope checks
    shows as DSTD_EWORKSPACE on a one-byte workspace."""
    L = native.lib()
    p = _model_params(35, 22, layers=5)
    assert _predict(L, None) == EINVAL
    assert _predict(L, p, obs=None) == EINVAL
    assert _predict(L, p, out=None) == EINVAL
    assert _predict(L, p, ws=None) == EINVAL
    assert _predict(L, p, Tin=0) == EINVAL
    assert _predict(L, p, Tin=35) == EINVAL  # input_n >= T
    assert _predict(L, p, Tin=36) == EINVAL
    assert _predict(L, p, H=0) == EINVAL
    assert _predict(L, p, H=-3) == EINVAL
    for bad in (128, 256, 1 << 31, 2 | 512):
        assert _predict(L, p, flags=bad) == EINVAL, bad
    for ok in (0, 1, 2, 4, 8, 16, 32, 64, 127):  # exactly the flags of dstd_model_fwd_ex
        assert _predict(L, p, flags=ok, nbytes=1) == EWORKSPACE, ok
    # the window cap: 64 windows of Tout frames pass, one frame more does not
    for Tin in (10, 34, 1):
        Tout = 35 - Tin
        assert _predict(L, p, Tin=Tin, H=64 * Tout + 1) == ELIMIT
        assert _predict(L, p, Tin=Tin, H=64 * Tout, nbytes=1) == EWORKSPACE
    # the model's shape, as dstd_model_fwd_ex judges it
    assert _predict(L, _model_params(129, 22), Tin=10) == ELIMIT
    assert _predict(L, _model_params(35, 33), Tin=10) == ELIMIT
    assert _predict(L, _model_params(35, 22, C=65), Tin=10) == ELIMIT
    assert _predict(L, _model_params(35, 22, layers=17), Tin=10) == EINVAL
    assert _predict(L, p, B=0) == EINVAL
    q = _model_params(35, 22, layers=5)
    q.enc[3].conv_t.wrm = None  # a parameter pointer: refused here, not by window 0's forward
    assert _predict(L, q) == EINVAL
    # the workspace, last
    need = L.dstd_model_predict_workspace_bytes(2, 35, 22, 64, 5)
    assert _predict(L, p, nbytes=need - 1) == EWORKSPACE
    assert _predict(L, p, nbytes=L.dstd_model_workspace_bytes(2, 35, 22, 64, 5)) == EWORKSPACE


def test_predict_method_refusals():
    m = get_model("dstdgcn", dstdgcn=H36M)
    obs = torch.zeros(2, 10, 22, 3)
    with pytest.raises(RuntimeError, match="eval"):
        m.train().predict(obs)
    m.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(obs)
    with pytest.raises(AssertionError):
        m.predict(torch.zeros(2, 35, 22, 3))  # a window, not observations
    with pytest.raises(ValueError, match="expected"):
        m.predict(torch.zeros(2, 10, 21, 3))
    with pytest.raises(ValueError, match="horizon"):
        m.predict(obs, 0)
    with pytest.raises(ValueError, match="windows"):
        m.predict(obs, 64 * 25 + 1)
    fast = F.DSTDGCN(**H36M)
    with pytest.raises(RuntimeError, match="eval"):
        fast.train().predict(obs)


# ---- the restatement -----------------------------------------------------------
def _extrapolate(Tin, T):
    """f(x)[b][s] = x[b][Tin-1] + (s - Tin + 1) * v, v the last observed step
    (Tin = 1: the constant step 3): a straight line continued."""

    def f(x):
        last = x[:, Tin - 1]
        v = last - x[:, Tin - 2] if Tin >= 2 else np.full_like(last, 3.0)
        s = np.arange(T, dtype=np.float64).reshape(1, T, *([1] * (x.ndim - 2)))
        return last[:, None] + (s - Tin + 1) * v[:, None]

    return f


@pytest.mark.parametrize("Tin,Tout", [(2, 4), (3, 3), (4, 2), (5, 1), (1, 5)])
def test_restatement_continues_a_line_exactly(Tin, Tout):
    """Against a closed form that shares none of the loop's bookkeeping: under
    the extrapolating forward every output frame f is obs[Tin-1] + (f + 1) * v,
    whatever the window it falls in -- for Tin > Tout the next window's
    observed part mixes frames of x_k and y_k, for Tout = 1 its last step spans
    both.  Integer-valued float64: exact."""
    T = Tin + Tout
    rng = np.random.default_rng(100 * Tin + Tout)
    obs = rng.integers(-50, 50, size=(3, Tin, 4, 3)).astype(np.float64)
    last = obs[:, Tin - 1]
    v = last - obs[:, Tin - 2] if Tin >= 2 else np.full_like(last, 3.0)
    for H in (1, Tout, Tout + 1, 3 * Tout + 1):
        got = predict_reference(_extrapolate(Tin, T), obs, T, H)
        want = last[:, None] + np.arange(1, H + 1, dtype=np.float64).reshape(1, H, 1, 1) * v[:, None]
        assert got.shape == (3, H, 4, 3)
        assert np.array_equal(got, want), (Tin, Tout, H)
        # ... and on torch tensors, the form the GPU tests run it in
        got_t = predict_reference(lambda x: torch.from_numpy(_extrapolate(Tin, T)(x.numpy())), torch.from_numpy(obs),
                                  T, H)
        assert np.array_equal(got_t.numpy(), want)


def test_restatement_is_the_reference_forward_for_one_window():
    """The fixture inputs are windows padded with their last observed frame, so
    the restatement over the fp64 oracle on obs = x[:, :10] with the horizon
    25 is the fixture's y64[:, 10:]."""
    d = load_npz("model_h36m.npz")
    sd = group(d, "sd/")
    L_ = int(d["opt/num_layers"])
    x = torch.from_numpy(d["x"])
    assert torch.equal(x[:, 10:], x[:, 9:10].expand(-1, 25, -1, -1))
    got = predict_reference(lambda w: O.dstdgcn(w, sd, L_), x[:, :10], 35, 25)
    want = d["y64"][:, 10:]
    assert got.shape == want.shape
    assert float(np.abs(got.numpy() - want).max()) <= 1e-6 * float(np.abs(want).max())
