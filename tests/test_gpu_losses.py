"""MI355X checks of the weighted / multi-term training loss
(include/dstd_gcn_loss.h, engine/loss.py, the engine's fused loss path).

References: the reference's own fp64 values and autograd gradients
(tests/golden/losses.npz, written by tests/golden/make_golden_losses.py) and,
for inputs the fixture does not hold, tests/loss_helper.py, which
tests/test_loss_host.py pins to that fixture at 1e-12.

Bars are those of test_mpjpe_forward_backward: value |delta| < 1e-5, gradient
max|delta| / max|ref| < 1e-5.  Bit-for-bit claims use torch.equal.

Time lengths are chosen around the kernels' 8-frame work items: 2, 3 (one
short item), 9 (an item of one frame after a full one), 25 (three full items
and a tail), 40 (a multiple of 8).
"""
import ctypes

import numpy as np
import pytest
import torch

import dstd_native as native
from conftest import group, load_npz
from engine import LossSpec, PredictionEngine, weighted_losses
from engine.loss import LOSSES, TERM_BITS, _problems
from loss_helper import TERMS, loss_terms
from model import DSTDGCB, get_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ("small", "twoframe", "minmax", "positive")
ALL = 15
VALUE_TOL = 1e-5
GRAD_TOL = 1e-5


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def raw_fwd(preds, targets, maps, terms, w=None):
    """dstd_losses_fwd as the C ABI gives it: values [n_problems][4]."""
    L = native.lib()
    values = torch.full((len(preds), native.LOSS_NTERMS), float("nan"), device=DEV)
    ws = torch.empty(L.dstd_losses_workspace_bytes(), dtype=torch.uint8, device=DEV)
    code = L.dstd_losses_fwd(_problems(preds, targets, maps), len(preds), terms,
                             w.data_ptr() if w is not None else None, values.data_ptr(), ws.data_ptr(), ws.numel(),
                             native.stream_handle(torch.device(DEV)))
    assert code == 0, code
    return values


def raw_bwd(preds, targets, maps, terms, coef, w=None, scale=1.0):
    """dstd_losses_bwd: one gradient per problem."""
    L = native.lib()
    dps = [torch.full_like(p, float("nan")) for p in preds]
    ptrs = (ctypes.c_void_p * len(preds))(*[d.data_ptr() for d in dps])
    code = L.dstd_losses_bwd(_problems(preds, targets, maps), len(preds), terms,
                             w.data_ptr() if w is not None else None, coef.data_ptr(), scale, ptrs,
                             native.stream_handle(torch.device(DEV)))
    assert code == 0, code
    return dps


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def check_against_helper(pred, targets, t0, step, targ_slice, w, cfg_w=(3.0, 0.5, 2.0, 0.25)):
    """All four terms of one problem through weighted_losses against the
    helper on ``targ_slice`` (the copy the frame mapping stands for)."""
    spec = LossSpec(list(zip(TERMS, cfg_w)))
    p = pred.to(DEV).requires_grad_(True)
    out = weighted_losses(spec, [p], targets.to(DEV), [(t0, step)], w)
    assert out.shape == (1, 4) and out.dtype == torch.float32 and out.is_cuda
    p64 = pred.double().requires_grad_(True)
    terms64 = loss_terms(p64, targ_slice, w)
    total = sum(c * terms64[t] for t, c in zip(TERMS, cfg_w))
    for i, (t, c) in enumerate(zip(TERMS, cfg_w)):
        got, ref = float(out[0, i].detach()) / c, float(terms64[t].detach())  # the term itself, config weight taken out
        print(t, got, ref)
        assert abs(got - ref) < VALUE_TOL, t
    (3.0 * out.sum()).backward()
    (3.0 * total).backward()
    print("grad rel", rel(p.grad, p64.grad))
    assert rel(p.grad, p64.grad) < GRAD_TOL
    return p.grad


# ---- every fixture case, every term, with and without weights -------------------
@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("variant", ["u", "w"])
@pytest.mark.parametrize("case", CASES)
def test_term_matches_reference_fixture(case, variant, term):
    d = load_npz("losses.npz")
    p = torch.from_numpy(d[f"{case}/pred"]).to(DEV).requires_grad_(True)
    q = torch.from_numpy(d[f"{case}/targ"]).to(DEV)
    w = d[f"{case}/w"].astype(np.float64) if variant == "w" else None  # float64 numpy, as the reference's datasets give
    v = LOSSES[term](p, q, w)
    assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
    ref = float(d[f"{case}/{variant}/{term}/value"])
    print(case, variant, term, float(v.detach()), ref)
    assert abs(float(v.detach()) - ref) < VALUE_TOL
    (3.0 * v).backward()
    key = f"{case}/{variant}/{term}/grad"
    if key not in d.files:
        # cl2 under a zero weight: the reference's gradient is NaN there; ours
        # is defined as cl1's (0 where w_j d_c == 0)
        assert (case, variant, term) == ("minmax", "w", "cl2")
        key = f"{case}/{variant}/cl1/grad"
    assert bool(torch.isfinite(p.grad).all())
    print("grad rel", rel(p.grad, 3.0 * torch.from_numpy(d[key])))
    assert rel(p.grad, 3.0 * torch.from_numpy(d[key])) < GRAD_TOL


# ---- one call for everything equals the separate calls, bit for bit -------------
def _two_problems():
    d = load_npz("losses.npz")
    targets = randn(3, 35, 66, seed=11).to(DEV)
    preds = [torch.from_numpy(d["positive/pred"]).to(DEV), torch.from_numpy(d["minmax/pred"]).to(DEV)]
    maps = [(10, 1), (24, -1)]
    w = torch.from_numpy(d["minmax/w"]).to(DEV)
    return preds, targets, maps, w


def test_all_terms_in_one_call_equal_single_term_calls():
    preds, targets, maps, w = _two_problems()
    both = raw_fwd(preds, targets, maps, ALL, w)
    assert bool(torch.isfinite(both).all())
    coef = torch.tensor([[3.0, 0.5, 2.0, 0.25], [1.5, 2.5, 0.75, 4.0]], device=DEV)
    for k, term in enumerate(TERMS):
        bit = TERM_BITS[term]
        one = raw_fwd(preds, targets, maps, bit, w)
        assert torch.equal(one[:, k], both[:, k]), term
        other = [j for j in range(4) if j != k]
        assert torch.equal(one[:, other], torch.zeros(2, 3, device=DEV)), term  # unrequested slots: 0
        # backward: all four terms requested with only this term's coefficient
        # set == this term alone (its other coefficient slots are not read)
        only = torch.zeros_like(coef)
        only[:, k] = coef[:, k]
        poisoned = torch.full_like(coef, float("nan"))
        poisoned[:, k] = coef[:, k]
        for a, b in zip(raw_bwd(preds, targets, maps, ALL, only, w), raw_bwd(preds, targets, maps, bit, poisoned, w)):
            assert bool(torch.isfinite(b).all()) and torch.equal(a, b), term


def test_two_problem_call_equals_two_one_problem_calls():
    preds, targets, maps, w = _two_problems()
    coef = torch.tensor([[3.0, 0.5, 2.0, 0.25], [1.5, 2.5, 0.75, 4.0]], device=DEV)
    both = raw_fwd(preds, targets, maps, ALL, w)
    g_both = raw_bwd(preds, targets, maps, ALL, coef, w, scale=0.5)
    assert not torch.equal(both[0], both[1])
    for i in range(2):
        one = raw_fwd(preds[i:i + 1], targets, maps[i:i + 1], ALL, w)
        assert torch.equal(one[0], both[i]), i
        g_one = raw_bwd(preds[i:i + 1], targets, maps[i:i + 1], ALL, coef[i:i + 1].contiguous(), w, scale=0.5)
        assert torch.equal(g_one[0], g_both[i]), i


def test_two_runs_are_bit_identical():
    preds, targets, maps, w = _two_problems()
    coef = torch.tensor([[3.0, 0.5, 2.0, 0.25], [1.5, 2.5, 0.75, 4.0]], device=DEV)
    runs = [(raw_fwd(preds, targets, maps, ALL, w), raw_bwd(preds, targets, maps, ALL, coef, w)) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


# ---- frame mapping: the targets are read in place ---------------------------------
@pytest.mark.parametrize("t0,step", [(10, 1), (24, -1)])
def test_frame_mapping_reads_the_slice_it_stands_for(t0, step):
    pred, targets = randn(3, 25, 66, seed=3), randn(3, 35, 66, seed=4)
    w = np.random.default_rng(5).uniform(0.1, 1.5, 22).astype(np.float32)
    sliced = targets[:, -25:] if step == 1 else targets.flip(1)[:, -25:]
    check_against_helper(pred, targets, t0, step, sliced.contiguous(), w)


def test_default_mapping_is_the_last_frames():
    pred, targets = randn(2, 9, 15, seed=6), randn(2, 12, 15, seed=7)
    spec = LossSpec([("jl2", 1.0), ("tl2", 1.0)])
    a = weighted_losses(spec, [pred.to(DEV)], targets.to(DEV))
    b = weighted_losses(spec, [pred.to(DEV)], targets[:, -9:].contiguous().to(DEV))
    assert torch.equal(a, b)


# ---- more work items than one pass of the 128 x 256 grid --------------------------
def test_grid_stride_covers_more_than_one_pass():
    B, T, V = 288, 40, 23  # 288 x 5 eight-frame items x 23 joints = 33,120 > 32,768 threads
    assert B * -(-T // 8) * V > 128 * 256
    pred = randn(B, T, V * 3, seed=8)
    targ = pred + 0.5 * randn(B, T, V * 3, seed=9)
    w = np.random.default_rng(10).uniform(0.0, 1.5, V).astype(np.float32)
    check_against_helper(pred, targ, 0, 1, targ, w)


# ---- ties and zero weights ---------------------------------------------------------
def test_ties_and_zero_weights_give_exact_zeros():
    B, T, V = 2, 9, 5
    pred = randn(B, T, V * 3, seed=12)
    targ = pred + 0.5 * randn(B, T, V * 3, seed=13)
    targ.view(B, T, V, 3)[:, :, 1] = pred.view(B, T, V, 3)[:, :, 1]  # joint 1: pred == targ exactly
    w = np.array([0.7, 1.3, 1.0, 0.0, 0.4], dtype=np.float32)  # joint 3: weight 0
    g = check_against_helper(pred, targ, 0, 1, targ, w).view(B, T, V, 3)
    assert bool(torch.isfinite(g).all())
    assert float(g[:, :, 1].abs().max()) == 0.0
    assert float(g[:, :, 3].abs().max()) == 0.0
    assert float(g[:, :, 0].abs().min()) > 0.0
    # and term by term (cl2 where the reference's autograd gives NaN)
    for term in TERMS:
        p = pred.to(DEV).requires_grad_(True)
        LOSSES[term](p, targ.to(DEV), w).backward()
        gt = p.grad.view(B, T, V, 3)
        assert bool(torch.isfinite(gt).all()), term
        assert float(gt[:, :, 1].abs().max()) == 0.0 and float(gt[:, :, 3].abs().max()) == 0.0, term


# ---- engine -------------------------------------------------------------------------
class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg, *a, **k):
        self.lines.append(msg)


LOSS_CFG = dict(joint=["jl2", 1], transition=["tl2", 0.5], coordinate=["cl1", 0.1])
N = 4  # samples per batch


def _model_3dpw():
    d = load_npz("engine.npz")
    opts = dict(input_channels=6, input_time_frame=10, output_time_frame=30, st_gcnn_dropout=0.0,
                joints_to_consider=23, num_feature=64, num_layers=5, layout="3dpw")
    m = get_model("dstdgcn", dstdgcn=opts)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in group(d, "train/sd0/").items()})
    m = m.to(DEV)
    for blk in m.modules():  # Module.to() splits the A_s / R_s storage alias
        if isinstance(blk, DSTDGCB):
            blk.A_s.data = blk.R_s.data
    return m.train(), d


def _weights_3dpw():
    w = np.random.default_rng(14).uniform(0.2, 1.5, 23)
    w[7] = 0.0
    return w  # float64, one joint switched off


def test_engine_reports_weighted_terms_in_config_order():
    m, d = _model_3dpw()
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5), loss=LOSS_CFG, n_out=1,
               transform="tsc", use_weight=True, inverse=False)
    log = _Log()
    eng = PredictionEngine(cfg, m, log)
    batch = tuple(torch.from_numpy(d[f"train/{n}0"])[:N] for n in ("inp", "inv", "seq", "seq"))
    captured, reported = [], []
    hook = m.register_forward_hook(lambda mod, args, out: captured.append(out.detach().clone()))
    step = eng._step
    eng._step = lambda *a: reported.append(step(*a)) or reported[-1]
    w = _weights_3dpw()
    total = eng.train([batch], 0, weights=w, max_iter=1)
    hook.remove()
    assert len(captured) == 1 and len(reported) == 1 and len(reported[0]) == 3
    out = captured[0].cpu().reshape(N, 40, 69)
    ref = loss_terms(out, batch[2], w)
    want = [cw * float(ref[name]) for name, cw in LOSS_CFG.values()]
    got = [float(v) for v in reported[0]]
    print(got, want)
    for g, r in zip(got, want):
        assert abs(g - r) <= 1e-5 * abs(r), (got, want)
    assert abs(total - sum(want)) <= 1e-5 * sum(want)
    line = log.lines[-1]
    assert line.index("joint:") < line.index("transition:") < line.index("coordinate:")
    grads = [p.grad for p in m.parameters() if p.requires_grad]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)


def test_graphed_weighted_step_equals_eager():
    """The three-term weighted step with the inverse pass, captured as a HIP
    graph and replayed: equal to the eager steps bit for bit (losses,
    parameters, buffers), across epochs -- each train() call rewrites the
    joint weights in the buffer the graph reads -- and a ragged last batch."""
    d = load_npz("engine.npz")
    batches = [tuple(torch.from_numpy(d[f"train/{n}{i}"])[:N] for n in ("inp", "inv", "seq", "seq")) for i in range(3)]
    ragged = tuple(t[:3] for t in batches[2])
    w = _weights_3dpw()
    engines = []
    for graphed in (True, False):
        m, _ = _model_3dpw()
        cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.5, step_size=2, graph=True),
                   loss=LOSS_CFG, n_out=1, transform="tsc", use_weight=True, inverse=True)
        eng = PredictionEngine(cfg, m, _Log())
        if not graphed:
            eng._graphed = lambda: False  # same capturable Adam, eager steps
        losses = [eng.train(batches[:2] + [ragged], e, weights=w) for e in range(3)]
        engines.append((eng, m, losses))
    (eg, mg, lg), (ee, me, le) = engines
    assert eg._graph_step is not None and ee._graph_step is None
    assert lg == le, (lg, le)
    for (n, a), b in zip(mg.named_parameters(), me.parameters()):
        assert torch.equal(a, b), n
    for (n, a), b in zip(mg.named_buffers(), me.buffers()):
        assert torch.equal(a, b), n
    assert lg[-1] < lg[0]
