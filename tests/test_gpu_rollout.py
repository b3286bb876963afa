"""Training through the rollout on the GPU (include/ext/dstd_gcn_rollout.h,
DSTDGCN.rollout / rollout_pair, PredictionEngine.train(horizon=...)).

The reference of every comparison is the loop a caller writes without the
feature (tests/rollout_helper.py rollout_loop: ``model(x_k)`` per window under
autograd, the frame shuffling as a small autograd Function with the header's
summation order).  Both sides issue the same native forward and backward calls
on the same bits in the same order -- window K-1's backward first -- so outputs,
BatchNorm buffers and gradients are compared with torch.equal.

Shapes: T = 6 models on the first five h36m joints (the generic kernels) at
(Tin, Tout) = (5, 1), (1, 5), (3, 3), (4, 2) with horizon 3 Tout - 1 -- the
smallest with the Tout + 1 term sums of the padding, observed frames carried
from x_k into x_{k+1} (Tin > Tout), and a truncated last window -- and the
two-encoder h36m fixture model of the guard tests at T = 35, B = 2, horizon 30
(two windows, the second cut to five frames).
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import dstd_native as native
from rollout_helper import glue_dy, glue_fold, glue_obs, rollout_loop, rollout_loop_pair, windows
from test_gpu_guards import (NAN_OUT, Bufs, _clones, _guard_model_stats, _keep, _on_gpu, _same, _unchanged, run_fills,
                             synth_model)
from test_gpu_predict import small_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EWORKSPACE = -2  # include/dstd_gcn.h
SMALL = [(5, 1), (1, 5), (3, 3), (4, 2)]
CASES = [f"T6-{a}-{b}" for a, b in SMALL] + ["h36m"]


def case_model(case):
    """(model on the GPU in eval mode, B, Tin, V, horizon)"""
    if case == "h36m":
        return _on_gpu(synth_model(35, 22, 2)), 2, 10, 22, 30
    Tin, Tout = (int(s) for s in case.split("-")[1:])
    return small_model(Tin, Tout), 2, Tin, 5, 3 * Tout - 1


def observations(B, Tin, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Tin, V, 3, generator=g).to(DEV)


def twins(case, mode, inplace=False, one_stream=False):
    m, B, Tin, V, H = case_model(case)
    a, b = m, copy.deepcopy(m)
    for x in (a, b):
        x.train(mode != "eval")
        x.do_in.p = 0.0  # (the fixture's 0.1: the chain and the loop draw their own seeds; the seeded test covers masks)
        x._dstd_inplace_grads = inplace
        x._dstd_one_stream = one_stream
    return a, b, B, Tin, V, H


def _equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(want).all()), what
    if not torch.equal(got, want):
        d = (got.detach().double() - want.detach().double()).abs()
        raise AssertionError(f"{what}: {int((got != want).sum())} of {got.numel()} elements differ, max |d| "
                             f"{float(d.max()):.3e} at max |want| {float(want.detach().abs().max()):.3e}")


def _state_equal(a, b, what):
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), f"{what}: {k}"


def _grads_equal(a, b, what):
    bad = []
    for (name, p), q in zip(a.named_parameters(), b.parameters()):
        assert (p.grad is None) == (q.grad is None), (what, name)
        if p.grad is not None and not torch.equal(p.grad, q.grad):
            d = float((p.grad.double() - q.grad.double()).abs().max())
            bad.append(f"{name}: max |d| {d:.3e} at max |grad| {float(q.grad.abs().max()):.3e}")
    assert not bad, (what, bad)


def _run(case, mode, inplace, one_stream=False):
    """One forward and backward of the chain and of the loop on twin models."""
    a, b, B, Tin, V, H = twins(case, mode, inplace, one_stream)
    what = f"{case} {mode} inplace={inplace} one_stream={one_stream}"
    n0 = int(a.bn_in.bn.num_batches_tracked)
    if mode == "pair":
        obs_a = [observations(B, Tin, V, 60 + i).requires_grad_() for i in range(2)]
        obs_b = [o.detach().clone().requires_grad_() for o in obs_a]
        out_a, out_b = a.rollout_pair(*obs_a, H), rollout_loop_pair(b, *obs_b, H)
    else:
        obs_a = [observations(B, Tin, V, 60).requires_grad_()]
        obs_b = [obs_a[0].detach().clone().requires_grad_()]
        out_a, out_b = (a.rollout(obs_a[0], H),), (rollout_loop(b, obs_b[0], H),)
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert x.shape == (B, H, V, 3)
        _equal(x, y, f"{what}: out {i}")
    _state_equal(a, b, what + ": buffers after the forward")
    K = windows(Tin + a.output_time_frame, Tin, H)
    calls = 0 if mode == "eval" else K * (2 if mode == "pair" else 1)
    assert int(a.bn_in.bn.num_batches_tracked) == n0 + calls
    scale = 1.0 / (B * H * V * 3)  # a loss of O(1): the models' outputs are O(1)
    (sum(o.square().sum() for o in out_a) * scale).backward()
    (sum(o.square().sum() for o in out_b) * scale).backward()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(obs_a, obs_b)):
        assert float(y.grad.abs().max()) > 0
        _equal(x.grad, y.grad, f"{what}: observed.grad {i}")
    _grads_equal(a, b, what)
    _state_equal(a, b, what + ": after the backward")


# ---- 1. the chain is the loop ---------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["autograd", "inplace"])
@pytest.mark.parametrize("mode", ["train", "pair", "eval"])
@pytest.mark.parametrize("case", CASES)
def test_rollout_is_the_loop(case, mode, inplace):
    """Outputs, running statistics, num_batches_tracked, observed.grad and every
    parameter's .grad of DSTDGCN.rollout / rollout_pair against the loop: in
    train mode, as a pair, and in eval mode under autograd (running-statistics
    BatchNorm); with the gradients handed to autograd from a fresh arena and
    accumulated in place (_dstd_inplace_grads)."""
    _run(case, mode, inplace)


@pytest.mark.parametrize("inplace", [False, True], ids=["autograd", "inplace"])
@pytest.mark.parametrize("case", ["T6-4-2", "h36m"])
def test_rollout_is_the_loop_on_one_stream(case, inplace):
    _run(case, "train", inplace, one_stream=True)


def test_rollout_without_grad_and_edges():
    m, B, Tin, V, H = case_model("T6-4-2")
    obs = observations(B, Tin, V, 61)
    with torch.no_grad():
        assert torch.equal(m.rollout(obs, H), m.predict(obs, H))  # eval, nothing to differentiate
        assert torch.equal(m.rollout(obs), m.predict(obs))
    for p in m.parameters():
        p.requires_grad_(False)
    assert torch.equal(m.rollout(obs, H), m.predict(obs, H)) and not m.rollout(obs, H).requires_grad
    o = obs.clone().requires_grad_()
    out = m.rollout(o, H)  # input gradients alone: frozen parameters, eval mode
    out.square().sum().backward()
    assert out.requires_grad and float(o.grad.abs().max()) > 0
    assert all(p.grad is None for p in m.parameters())
    with pytest.raises(RuntimeError, match="second time"):
        out.square().sum().backward()
    m.train()
    with torch.no_grad():  # train mode without autograd: the chain all the same, buffers updated
        n0 = int(m.bn_in.bn.num_batches_tracked)
        got = m.rollout(obs, H)
        assert got.shape == (B, H, V, 3) and not got.requires_grad
        assert int(m.bn_in.bn.num_batches_tracked) == n0 + windows(6, Tin, H)
    assert m.rollout(obs[:0], H).shape == (0, H, V, 3)
    with pytest.raises(ValueError, match="windows"):
        m.rollout(obs, 64 * 2 + 1)


# ---- 2. the entry points: dropout seeds, memory contract -------------------------------
def _c_params(m, b):
    p = native.ModelParams.from_buffer_copy(m._native_params())
    return p, _guard_model_stats(b, p, m)  # the running statistics on guarded copies


def _seeds(values):
    return (ctypes.c_uint64 * len(values))(*values)


def rollout_call(m, obs, dout, H, flags, drop, seeds, need_dobs, fill, short=None, stepwise=False):
    """dstd_model_rollout_fwd and _bwd on exact-size guarded buffers.  ``short``
    names a size to pass one byte short first: that call must be refused with
    nothing written, and the valid call follows on the same buffers.
    ``stepwise``: the backward as K calls of dstd_model_rollout_bwd_window."""
    L, st = native.lib(), native.stream_handle(obs.device)
    B, Tin, V, _ = obs.shape
    T, C, layers = Tin + m.output_time_frame, m.num_feature, m.num_layers
    K = windows(T, Tin, H)
    b = Bufs()
    p, stats = _c_params(m, b)
    pref = native.ext.model_params_ref(p)
    ns = L.dstd_model_rollout_saved_bytes(B, T, V, C, layers, K)
    nw = L.dstd_model_rollout_workspace_bytes(B, T, V, C, layers)
    saved = b.new("saved", ns, fill)
    out = b.f32("out", (B, H, V, 3), NAN_OUT)
    sd = _seeds(seeds) if seeds is not None else None

    def refused(code, what):
        assert code == EWORKSPACE, (what, code)
        b.check_frozen(snap, what)

    if short == "saved fwd":
        snap = b.freeze()
        refused(L.dstd_model_rollout_fwd(pref, obs.data_ptr(), B, Tin, H, 0.1, drop, sd, out.data_ptr(), saved.ptr,
                                         ns - 1, st, flags), short)
    native.check(L.dstd_model_rollout_fwd(pref, obs.data_ptr(), B, Tin, H, 0.1, drop, sd, out.data_ptr(), saved.ptr,
                                          ns, st, flags), "dstd_model_rollout_fwd")
    torch.cuda.synchronize()
    saved0, stats0 = saved.tensor.clone(), _clones(stats)
    ws = b.new("workspace", nw, fill)
    dobs = b.f32("dobs", obs.shape, NAN_OUT) if need_dobs else None
    params = list(m.parameters())
    arena = native.GradArena(params, obs.device, buf=b.f32("gradient arena", (native.arena_numel(params),), 0))
    gref = native.ext.model_grads_ref(m._native_grads(arena))
    args = lambda a, c: (pref, B, Tin, H, drop, sd, saved.ptr, a, dout.data_ptr(), gref,  # noqa: E731
                         dobs.data_ptr() if need_dobs else None, ws.ptr, c, st, flags)
    if short in ("saved bwd", "workspace"):
        snap = b.freeze()
        refused(L.dstd_model_rollout_bwd(*(args(ns - 1, nw) if short == "saved bwd" else args(ns, nw - 1))), short)
    if stepwise:
        a = args(ns, nw)
        for k in range(K - 1, -1, -1):
            native.check(L.dstd_model_rollout_bwd_window(*a[:4], k, *a[4:]), "dstd_model_rollout_bwd_window")
    else:
        native.check(L.dstd_model_rollout_bwd(*args(ns, nw)), "dstd_model_rollout_bwd")
    b.check()  # (synchronises) no write outside out, saved, dobs, the workspace or the arena
    assert torch.equal(saved.tensor, saved0), "the backward wrote to saved"
    _unchanged(stats, stats0, "running statistics across the backward")
    res = {"out": out}
    if need_dobs:
        res["dobs"] = dobs
    res.update({f"stat{i}": s for i, s in enumerate(stats)})
    res.update({"grad " + n: g for (n, _), g in zip(m.named_parameters(), arena.views()) if g is not None})
    return _keep(res)


@pytest.mark.parametrize("case,flags,drop,need_dobs", [
    ("T6-4-2", 0, 0.1, True), ("T6-5-1", native.TRAIN_PAIRED, 0.0, True), ("T6-1-5", native.TRAIN_ONE_STREAM, 0.1, False),
    ("T6-3-3", native.TRAIN_RUNNING_STATS, 0.0, True), ("h36m", 0, 0.0, True),
], ids=["T6-4-2-drop", "T6-5-1-paired", "T6-1-5-one-stream-drop-no-dobs", "T6-3-3-running", "h36m"])
def test_rollout_memory_contract(case, flags, drop, need_dobs):
    """Exact-size saved / out / dobs / workspace / arena between sentinel guards:
    nothing is written outside them, the results do not depend on what saved and
    the workspace held before (0x00, 0xFF, 0x4B), the backward leaves saved and
    the running statistics alone, the inputs are not written."""
    m, B, Tin, V, H = case_model(case)
    m.train(not flags & native.TRAIN_RUNNING_STATS)
    obs = observations(B, Tin, V, 71)
    dout = observations(B, H, V, 72)
    seeds = [0x5DEECE66D + 977 * k for k in range(windows(Tin + m.output_time_frame, Tin, H))] if drop else None
    inputs = [obs, dout] + list(m.parameters()) + list(m.buffers())
    before = _clones(inputs)
    what = f"rollout {case} flags {flags} p{drop}"
    got = run_fills(lambda fill: rollout_call(m, obs, dout, H, flags, drop, seeds, need_dobs, fill), what)
    _unchanged(inputs, before, what)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (what, k)
    # one window per call into the same arena: the same launches, the same bits
    _same(got, rollout_call(m, obs, dout, H, flags, drop, seeds, need_dobs, 0xFF, stepwise=True), what + ": stepwise")
    assert ("dobs" in got) == need_dobs
    if need_dobs:
        assert float(got["dobs"].abs().max()) > 0


def test_rollout_size_checks():
    """Each size one byte short is DSTD_EWORKSPACE with nothing written --
    saved in the forward, saved and the workspace in the backward -- and the
    valid call on the same buffers still gives the reference result."""
    m, B, Tin, V, H = case_model("T6-4-2")
    m.train()
    obs, dout = observations(B, Tin, V, 73), observations(B, H, V, 74)
    base = rollout_call(m, obs, dout, H, 0, 0.0, None, True, 0x4B)
    for short in ("saved fwd", "saved bwd", "workspace"):
        _same(base, rollout_call(m, obs, dout, H, 0, 0.0, None, True, 0x4B, short=short), short)


def test_rollout_windows_are_the_seeded_train_forwards():
    """Dropout 0.1 with explicit host seeds: window k's slice of out is
    dstd_model_train_fwd_ex(x_k, seed_k) of a chain built by hand with torch
    indexing, bit for bit; the same seeds give the same out, other seeds
    another."""
    L, st = native.lib(), native.stream_handle(torch.device(DEV))
    m, B, Tin, V, H = case_model("T6-4-2")
    m.train()
    T, Tout, C, layers = 6, 2, m.num_feature, m.num_layers
    K = windows(T, Tin, H)
    obs, dout = observations(B, Tin, V, 75), observations(B, H, V, 76)
    seeds = [11, 0xFFFFFFFF12345678, 3]
    got = rollout_call(m, obs, dout, H, 0, 0.1, seeds, True, 0x00)
    _same(got, rollout_call(m, obs, dout, H, 0, 0.1, seeds, True, 0x00), "the same seeds")
    other = rollout_call(m, obs, dout, H, 0, 0.1, [11, 0xFFFFFFFF12345678, 4], True, 0x00)
    assert torch.equal(other["out"][:, :2 * Tout], got["out"][:, :2 * Tout])  # windows 0 and 1: their seeds
    assert not torch.equal(other["out"][:, 2 * Tout:], got["out"][:, 2 * Tout:])
    assert not torch.equal(rollout_call(m, obs, dout, H, 0, 0.1, [12, 5, 3], True, 0x00)["out"], got["out"])
    b = Bufs()
    p, _ = _c_params(m, b)
    ns = L.dstd_model_train_saved_bytes(B, T, V, C, layers)
    saved = b.new("saved", ns, 0x00)
    mfr = [min(s, Tin - 1) for s in range(T)]
    x = obs[:, mfr].contiguous()
    for k in range(K):
        y = torch.empty_like(x)
        native.check(L.dstd_model_train_fwd_ex(p, x.data_ptr(), B, 0.1, 0.1, seeds[k], y.data_ptr(), saved.ptr, ns, st, 0),
                     "dstd_model_train_fwd_ex")
        take = min(Tout, H - k * Tout)
        assert torch.equal(got["out"][:, k * Tout:k * Tout + take], y[:, Tin:Tin + take]), f"window {k}"
        seq = torch.cat([x[:, :Tin], y[:, Tin:]], 1)
        x = seq[:, [Tout + i for i in mfr]].contiguous()
    b.check()


# ---- 3. the backward glue alone ------------------------------------------------------
@pytest.mark.parametrize("Tin,Tout", SMALL)
def test_backward_glue_is_the_restatement(Tin, Tout):
    """The three glue kernels through the test hook on random dout / G, B = 3,
    V = 1, 22, 25 (rows of 3, 66 and 75 floats: below, just above and above one
    pass of a wave's lanes): equal to the fp32 restatement exactly, and within
    (Tout + 2) * 2^-24 * sum |terms| of the fp64 closed form elementwise -- the
    bound of a sequential sum of at most Tout + 2 terms (Tout + 1 padding copies
    and the dout or dx term) in fp32, rounding unit 2^-24."""
    L, st = native.lib(), native.stream_handle(torch.device(DEV))
    T, B, H = Tin + Tout, 3, 3 * Tout - 1
    K = windows(T, Tin, H)
    u = (Tout + 2) * 2.0 ** -24

    def check(got, f, args, what):
        got = got.cpu().numpy()
        assert np.array_equal(got, f(*args)), what
        a64 = [a.astype(np.float64) if isinstance(a, np.ndarray) else a for a in args]
        mag = [np.abs(a) if isinstance(a, np.ndarray) else a for a in a64]
        assert (np.abs(got.astype(np.float64) - f(*a64)) <= u * f(*mag)).all(), what

    for V in (1, 22, 25):
        rng = np.random.default_rng(1000 * Tin + 10 * Tout + V)
        dout = rng.standard_normal((B, H, V, 3)).astype(np.float32)
        Gn = rng.standard_normal((B, T, V, 3)).astype(np.float32)
        dx = rng.standard_normal((B, T, V, 3)).astype(np.float32)
        d_dout, d_Gn = torch.from_numpy(dout).to(DEV), torch.from_numpy(Gn).to(DEV)
        for k in range(K):
            gn, d_gn = (None, None) if k == K - 1 else (Gn, d_Gn.data_ptr())
            dy = torch.full((B, T, V, 3), float("nan"), device=DEV)
            assert L.dstd_model_rollout_glue_bwd(0, d_dout.data_ptr(), d_gn, dy.data_ptr(), B, T, Tin, V, H, k, st) == 0
            check(dy, glue_dy, (dout, gn, T, Tin, k), f"dy V{V} k{k}")
        G = torch.from_numpy(dx).to(DEV)
        assert L.dstd_model_rollout_glue_bwd(1, None, d_Gn.data_ptr(), G.data_ptr(), B, T, Tin, V, H, 0, st) == 0
        check(G, glue_fold, (dx, Gn, T, Tin), f"fold V{V}")
        dobs = torch.full((B, Tin, V, 3), float("nan"), device=DEV)
        assert L.dstd_model_rollout_glue_bwd(2, None, d_Gn.data_ptr(), dobs.data_ptr(), B, T, Tin, V, H, 0, st) == 0
        check(dobs, glue_obs, (Gn, T, Tin), f"dobs V{V}")
        assert torch.equal(d_Gn.cpu(), torch.from_numpy(Gn)) and torch.equal(d_dout.cpu(), torch.from_numpy(dout))


# ---- 4. the engine ------------------------------------------------------------------
class _Log:
    def info(self, *a):
        pass


def _engine_setup(frames, seed):
    """A T = 6 (Tin 3) h36m model in a PredictionEngine (inverse pass, jl2 + tl2)
    and one batch of two windows of ``frames`` frames from the device loader."""
    from dstd_data import DeviceLoader, DeviceSequences
    from engine import PredictionEngine
    opts = dict(input_channels=6, input_time_frame=3, output_time_frame=3, st_gcnn_dropout=0.0,
                joints_to_consider=22, num_feature=16, num_layers=1, layout="h36m")
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5),
               loss=dict(joint=["jl2", 1], transition=["tl2", 0.5]), n_out=1, transform="tsc", use_weight=True,
               inverse=True)
    from model import get_model
    torch.manual_seed(seed)
    m = get_model("dstdgcn", dstdgcn=opts).to(DEV).train()
    rng = np.random.default_rng(seed)
    dim_used = np.sort(rng.choice(96, 66, replace=False))
    seqs = DeviceSequences.from_windows(rng.normal(size=(2, frames, 96)), dim_used, 3, frames - 3, padding=True,
                                        device=DEV)
    weights = rng.uniform(0.5, 1.5, 22).astype(np.float32)
    twin = copy.deepcopy(m)
    return PredictionEngine(cfg, m, _Log()), PredictionEngine(cfg, twin, _Log()), DeviceLoader(seqs, 2), weights


def _hand_step(eng, batch, weights, horizon):
    """The engine's step composed by hand from the model's pair forward /
    rollout, weighted_losses and the optimizer."""
    from engine.loss import prepare_joint_weights, weighted_losses
    inputs, inputs_inv, targets, _ = batch
    net = eng.model.model
    net._dstd_inplace_grads = True
    try:
        x, xi = eng.transform(inputs.float()), eng.transform(inputs_inv.float())
        if horizon is None:
            o1, o2 = net.forward_pair(x, xi)
            t = o1.shape[1]
            maps = [(targets.shape[1] - t, 1), (t - 1, -1)]
        else:
            o1, o2 = net.rollout_pair(x[:, :3].contiguous(), xi[:, :3].contiguous(), horizon)
            maps = [(3, 1), (horizon - 1, -1)]
        out = weighted_losses(eng.model.loss_spec, [eng.inverse(o1), eng.inverse(o2)], targets.float(), maps,
                              prepare_joint_weights(weights, DEV))
        eng.optimizer.zero_grad()
        (out.sum() / 2).backward()
        eng.optimizer.step()
    finally:
        net._dstd_inplace_grads = False
    return out[0].detach().clone()


@pytest.mark.parametrize("horizon", [12, None])
def test_engine_step_is_the_hand_composed_step(horizon):
    """One train() step -- through the rollout with horizon = 12 (four windows),
    and the plain path with horizon = None on a batch of one window -- against
    the same step composed by hand on a twin: the step's losses and every
    parameter and buffer afterwards, bit for bit."""
    eng, hand, loader, weights = _engine_setup(15 if horizon else 6, 31)
    steps = []
    name = "_step_rollout" if horizon else "_step"
    step = getattr(eng, name)
    setattr(eng, name, lambda *a: steps.append(step(*a)) or steps[-1])
    total = eng.train(loader, 0, weights=weights, horizon=horizon)
    want = _hand_step(hand, next(iter(loader)), weights, horizon)
    assert len(steps) == 1 and np.isfinite(total)
    got = torch.stack([v.reshape(()) for v in steps[0]])
    assert got.shape == (2,) and bool((got > 0).all())
    assert torch.equal(got, want), (got, want)
    _state_equal(eng.model.model, hand.model.model, f"engine step, horizon {horizon}")
    assert not getattr(eng.model.model, "_dstd_inplace_grads", False)


def test_engine_horizon_refusals():
    eng, _, loader, weights = _engine_setup(15, 32)
    batch = next(iter(loader))
    with pytest.raises(ValueError, match="frames"):  # 15 frames are 3 + 12, not 3 + 9
        eng.train(loader, 0, horizon=9)
    with pytest.raises(ValueError, match="list"):
        eng.train([([batch[0]], batch[1], batch[2], batch[3])], 0, horizon=12)

    class _Time:
        def transform(self, x):
            return x

        inverse = transform

    with pytest.raises(ValueError, match="time"):
        eng.train(loader, 0, horizon=12, time_tsfm=_Time())
