"""Host-side checks of the weighted / multi-term training loss
(include/dstd_gcn_loss.h, engine/loss.py): exports, argument checks before any
GPU work, the loss table, and the fp64 helper the GPU tests compare against
(tests/loss_helper.py) pinned to the reference fixture.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import dstd_native as native
from conftest import load_npz
from engine import (ModelWrapper, PredictionEngine, mae_error_3d, mpjpe_error_3d, mse_error_3d,
                    transition_error_3d)
from engine.loss import LOSSES, LossSpec, prepare_joint_weights
from loss_helper import TERMS, loss_terms_and_grads
from model import get_model
from test_capi_host import header_symbols

H36M = dict(input_channels=6, input_time_frame=10, output_time_frame=25, st_gcnn_dropout=0.1,
            joints_to_consider=22, num_feature=64, num_layers=5, layout="h36m")
CASES = ("small", "twoframe", "minmax", "positive")
EINVAL = -1


def test_library_exports_every_loss_header_symbol():
    L = native.lib()
    syms = header_symbols("dstd_gcn_loss.h")
    assert len(syms) == 3, syms
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(native.LOSS_EXPORTS)


def _problem(**kw):
    """A well-formed problem (B=2, T=25 of 35 target frames, V=22); the
    pointers are never dereferenced on the host."""
    f = dict(pred=0x1000, targ=0x2000, B=2, T=25, V=22, targ_T=35, targ_t0=10, targ_step=1)
    f.update(kw)
    return native.LossProblem(**f)


def _fwd(problems, n=None, terms=native.LOSS_JL2, values=0x3000, ws=0x4000, ws_bytes=None):
    L = native.lib()
    arr = (native.LossProblem * len(problems))(*problems) if problems is not None else None
    ws_bytes = L.dstd_losses_workspace_bytes() if ws_bytes is None else ws_bytes
    return L.dstd_losses_fwd(arr, len(problems) if n is None else n, terms, None, values, ws, ws_bytes, None)


def _bwd(problems, n=None, terms=native.LOSS_JL2, coef=0x3000, dpreds=(0x5000, 0x6000)):
    L = native.lib()
    arr = (native.LossProblem * len(problems))(*problems) if problems is not None else None
    ptrs = (ctypes.c_void_p * 2)(*dpreds) if dpreds is not None else None
    return L.dstd_losses_bwd(arr, len(problems) if n is None else n, terms, None, coef, 1.0, ptrs, None)


BAD_PROBLEMS = {
    "null pred": dict(pred=None), "null targ": dict(targ=None), "B = 0": dict(B=0), "T < 0": dict(T=-1),
    "V = 0": dict(V=0), "targ_T = 0": dict(targ_T=0), "step 0": dict(targ_step=0), "step 2": dict(targ_step=2),
    "frames past the end": dict(targ_t0=11), "negative start": dict(targ_t0=-1),
    "reversed below 0": dict(targ_t0=23, targ_step=-1), "reversed start past the end": dict(targ_t0=35, targ_step=-1),
}


@pytest.mark.parametrize("what", list(BAD_PROBLEMS))
def test_bad_problem_is_einval_before_any_gpu_work(what):
    bad = _problem(**BAD_PROBLEMS[what])
    assert _fwd([bad]) == EINVAL
    assert _bwd([bad]) == EINVAL
    assert _fwd([_problem(), bad]) == EINVAL  # and as the second problem
    assert _bwd([_problem(), bad]) == EINVAL


def test_bad_call_arguments_are_einval_before_any_gpu_work():
    L = native.lib()
    ok = _problem()
    assert L.dstd_losses_workspace_bytes() > 0
    assert _fwd(None, n=1) == EINVAL and _bwd(None, n=1) == EINVAL
    for n in (0, 3, -1):
        assert _fwd([ok, ok], n=n) == EINVAL and _bwd([ok, ok], n=n) == EINVAL
    for terms in (0, 16, native.LOSS_JL2 | 32):
        assert _fwd([ok], terms=terms) == EINVAL and _bwd([ok], terms=terms) == EINVAL
    assert _fwd([ok], values=None) == EINVAL
    assert _fwd([ok], ws=None) == EINVAL
    assert _fwd([ok], ws_bytes=L.dstd_losses_workspace_bytes() - 1) == EINVAL
    assert _bwd([ok], coef=None) == EINVAL
    assert _bwd([ok], dpreds=None) == EINVAL
    assert _bwd([ok, ok], dpreds=(0x5000, None)) == EINVAL
    # tl2 on a single frame: the reference takes the mean of an empty tensor
    one = _problem(T=1, targ_t0=34)
    assert _fwd([one], terms=native.LOSS_TL2) == EINVAL and _bwd([one], terms=native.LOSS_TL2 | 1) == EINVAL
    # the two problems share the joint weights, so they share V
    assert _fwd([ok, _problem(V=23)]) == EINVAL and _bwd([ok, _problem(V=23)]) == EINVAL
    # the reversed mapping of the engine's inverse pass is well-formed
    assert native.LossProblem(targ_t0=24, targ_step=-1).targ_step == -1


def test_model_wrapper_loss_table():
    m = get_model("dstdgcn", dstdgcn=H36M)
    w = ModelWrapper(m, {"joint": ["jl2", 1], "transition": ["tl2", 1], "coordinate": ["cl1", 1], "c2": ["cl2", 0.5]})
    assert list(w.loss_funcs) == ["joint", "transition", "coordinate", "c2"]
    assert [f for f, _ in w.loss_funcs.values()] == [mpjpe_error_3d, transition_error_3d, mae_error_3d, mse_error_3d]
    assert w.loss_spec.terms == 15 and not w.plain_mpjpe
    assert set(LOSSES) == {"jl2", "tl2", "cl1", "cl2"}
    for name in ("bl2", "gm2"):
        with pytest.raises(NotImplementedError):
            ModelWrapper(m, {"x": [name, 1]})
    # the shipped configuration keeps the plain mpjpe path unless weights are given
    plain = ModelWrapper(m, {"joint": ["jl2", 1]})
    assert plain.plain_mpjpe and not plain.fused_losses(None) and plain.fused_losses(np.ones(22))
    assert ModelWrapper(m, {"joint": ["jl2", 1], "again": ["jl2", 2]}).fused_losses(None)


def test_loss_spec_matrix_holds_each_line_in_its_term_column():
    spec = LossSpec([("cl1", 0.25), ("jl2", 1), ("tl2", 0.5), ("jl2", 2)])
    assert spec.terms == native.LOSS_JL2 | native.LOSS_TL2 | native.LOSS_CL1
    assert spec.matrix("cpu").tolist() == [[0, 0, 0.25, 0], [1, 0, 0, 0], [0, 0.5, 0, 0], [2, 0, 0, 0]]
    assert spec.matrix("cpu") is spec.matrix("cpu")


@pytest.mark.parametrize("fn", [mpjpe_error_3d, transition_error_3d, mae_error_3d, mse_error_3d])
def test_weights_are_checked_on_the_host_and_there_is_no_cpu_fallback(fn):
    o = torch.zeros(2, 3, 15)
    with pytest.raises(ValueError):
        fn(o, o, -np.ones(5))
    with pytest.raises(ValueError):
        fn(o, o, torch.tensor([1., 1., -0.5, 1., 1.]))
    with pytest.raises(ValueError):
        fn(o, o, np.ones(4))
    with pytest.raises(ValueError):
        fn(o, o, np.ones((5, 1)))
    with pytest.raises(ValueError):
        fn(o, torch.zeros(2, 4, 15), np.ones(5))
    for w in (None, np.ones(5), torch.ones(5, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(o, o, w)


def test_prepare_joint_weights_reuses_its_buffer():
    a = prepare_joint_weights(np.array([0., 0.5, 1.]), "cpu")
    assert a.dev.dtype == torch.float32 and a.dev.tolist() == [0., 0.5, 1.]
    b = prepare_joint_weights(torch.tensor([1., 2., 3.], dtype=torch.float64), "cpu", into=a)
    assert b is a and a.dev.tolist() == [1., 2., 3.]
    c = prepare_joint_weights(np.ones(4), "cpu", into=a)
    assert c is not a and len(c) == 4
    assert prepare_joint_weights(c, "cpu", 4) is c
    with pytest.raises(ValueError):
        prepare_joint_weights(c, "cpu", 5)


def test_engine_accepts_the_extra_loss_lines():
    class _Log:
        def info(self, *a, **k):
            pass

    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5),
               loss=dict(joint=["jl2", 1], transition=["tl2", 1], coordinate=["cl1", 1]), n_out=1, transform="tsc",
               use_weight=True, inverse=True)
    eng = PredictionEngine(cfg, get_model("dstdgcn", dstdgcn=H36M), _Log())
    assert eng.model.loss_spec.terms == native.LOSS_JL2 | native.LOSS_TL2 | native.LOSS_CL1
    with pytest.raises(NotImplementedError):
        PredictionEngine(dict(cfg, loss=dict(g=["gm2", 1])), get_model("dstdgcn", dstdgcn=H36M), _Log())


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("variant", ["u", "w"])
def test_helper_reproduces_the_reference_fixture(case, variant):
    """tests/loss_helper.py against the reference's fp64 values and autograd
    gradients, to 1e-12 -- which also pins the closed forms of the header."""
    d = load_npz("losses.npz")
    pred, targ = torch.from_numpy(d[f"{case}/pred"]), torch.from_numpy(d[f"{case}/targ"])
    w = d[f"{case}/w"] if variant == "w" else None
    values, grads = loss_terms_and_grads(pred, targ, w)
    for term in TERMS:
        ref = float(d[f"{case}/{variant}/{term}/value"])
        assert abs(values[term] - ref) <= 1e-12, (term, values[term], ref)
        key = f"{case}/{variant}/{term}/grad"
        if key in d.files:
            assert float((grads[term] - torch.from_numpy(d[key])).abs().max()) <= 1e-12, term
        else:  # the reference's NaN case: cl2 under a zero weight
            assert (case, variant, term) == ("minmax", "w", "cl2")
        assert bool(torch.isfinite(grads[term]).all())


def test_fixture_covers_the_edge_weights():
    d = load_npz("losses.npz")
    w = d["minmax/w"]
    assert w.min() == 0.0 and w.max() == 1.0 and d["positive/w"].min() > 0
    assert d["small/pred"].shape == (2, 3, 15) and d["twoframe/pred"].shape == (2, 2, 66)
    assert d["minmax/pred"].shape == d["positive/pred"].shape == (3, 25, 66)
    # cl2's value is cl1's (the reference takes sqrt((w d)^2))
    for case in CASES:
        for variant in "uw":
            assert abs(float(d[f"{case}/{variant}/cl2/value"]) - float(d[f"{case}/{variant}/cl1/value"])) < 1e-15
