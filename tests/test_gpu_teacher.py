"""Scheduled sampling over the rollout on the GPU (include/ext/dstd_gcn_teacher.h,
the teacher arguments of DSTDGCN.rollout / rollout_pair,
PredictionEngine.train(horizon=..., teacher_ratio=...)).

The reference of every comparison is the loop a caller writes without the
feature (tests/teacher_helper.py teacher_loop: ``model(x_k)`` per window under
autograd, rollout_helper's glue Functions and a torch.where on the mask between
two windows).  Both sides issue the same native forward and backward calls on
the same bits in the same order, so outputs, BatchNorm buffers and gradients
are compared with torch.equal, as tests/test_gpu_rollout.py does for the
free-running chain.

Shapes: the T = 6 models of that file at (Tin, Tout) = (5, 1), (1, 5), (3, 3),
(4, 2) with B = 4 (a pair: 2 + 2) and horizons of three or four windows, the
last one truncated wherever Tout > 1; masks all-zero, all-one and a fixed
mixed pattern (every boundary has forced and free samples, the halves of a
pair differ); and the two-encoder h36m model at T = 35, B = 2, horizon 30.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import dstd_native as native
from rollout_helper import glue_obs, windows
from teacher_helper import glue_dy_tf, glue_fold_tf, mixed_mask, teacher_loop, teacher_loop_pair
from test_gpu_guards import NAN_OUT, Bufs, _clones, _guard_model_stats, _keep, _on_gpu, _same, _unchanged, run_fills, synth_model
from test_gpu_predict import small_model
from test_gpu_rollout import _equal, _grads_equal, _state_equal, observations

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, EWORKSPACE = -1, -2  # include/dstd_gcn.h
HORIZON = {(5, 1): 4, (1, 5): 14, (3, 3): 8, (4, 2): 7}  # K = 4, 3, 3, 4
SMALL = list(HORIZON)
CASES = [f"T6-{a}-{b}" for a, b in SMALL]
MASKS = ("zero", "one", "mixed")


def case_model(case):
    """(model on the GPU in eval mode, Tin, V, horizon)"""
    if case == "h36m":
        return _on_gpu(synth_model(35, 22, 2)), 10, 22, 30
    Tin, Tout = (int(s) for s in case.split("-")[1:])
    return small_model(Tin, Tout), Tin, 5, HORIZON[Tin, Tout]


def mask_of(name, K, N, pair):
    m = {"zero": np.zeros((K, N), np.uint8), "one": np.ones((K, N), np.uint8),
         "mixed": mixed_mask(K, N, N // 2 if pair else None)}[name]
    return torch.from_numpy(m).to(DEV)


def twins(m, mode, inplace=False, count=2):
    out = [m] + [copy.deepcopy(m) for _ in range(count - 1)]
    for x in out:
        x.train(mode != "eval")
        x.do_in.p = 0.0  # gradient comparisons: no dropout (the chain and the loop draw their own seeds)
        x._dstd_inplace_grads = inplace
    return out


def _loss(outs):
    return sum(o.square().sum() for o in outs) / sum(o.numel() for o in outs) * len(outs)


def _run(case, mode, inplace, mask_name, B):
    """One forward and backward of the teacher-forced chain and of the loop on twin models."""
    m, Tin, V, H = case_model(case)
    a, b = twins(m, mode, inplace)
    K = windows(Tin + a.output_time_frame, Tin, H)
    what = f"{case} {mode} inplace={inplace} mask={mask_name}"
    n0 = int(a.bn_in.bn.num_batches_tracked)
    pair = mode == "pair"
    n = B // 2 if pair else B
    truth = observations(n, Tin + H, V, 81)
    mask = mask_of(mask_name, K, B, pair)
    mask_a = mask.bool() if inplace else mask  # both dtypes the method takes
    before = _clones([truth, mask])
    if pair:
        obs_a = [observations(n, Tin, V, 82 + i).requires_grad_() for i in range(2)]
        obs_b = [o.detach().clone().requires_grad_() for o in obs_a]
        out_a = a.rollout_pair(*obs_a, H, teacher=truth, teacher_mask=mask_a)
        out_b = teacher_loop_pair(b, *obs_b, H, truth, mask)
    else:
        obs_a = [observations(n, Tin, V, 82).requires_grad_()]
        obs_b = [obs_a[0].detach().clone().requires_grad_()]
        out_a = (a.rollout(obs_a[0], H, teacher=truth, teacher_mask=mask_a),)
        out_b = (teacher_loop(b, obs_b[0], H, truth, mask),)
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert x.shape == (n, H, V, 3)
        _equal(x, y, f"{what}: out {i}")
    _state_equal(a, b, what + ": buffers after the forward")
    calls = 0 if mode == "eval" else K * (2 if pair else 1)
    assert int(a.bn_in.bn.num_batches_tracked) == n0 + calls
    _loss(out_a).backward()
    _loss(out_b).backward()
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(obs_a, obs_b)):
        assert float(y.grad.abs().max()) > 0
        _equal(x.grad, y.grad, f"{what}: observed.grad {i}")
    _grads_equal(a, b, what)
    _state_equal(a, b, what + ": after the backward")
    _unchanged([truth, mask], before, what + ": teacher and mask")
    assert truth.grad is None


# ---- 1. the chain is the loop ---------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["autograd", "inplace"])
@pytest.mark.parametrize("mode", ["train", "pair", "eval"])
@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("case", CASES)
def test_teacher_rollout_is_the_loop(case, mask_name, mode, inplace):
    """Outputs, running statistics, num_batches_tracked, observed.grad and every
    parameter's .grad of rollout / rollout_pair with a teacher against the loop
    with torch.where, for each of the three masks: in train mode, as a pair, and in eval
    mode under autograd; gradients through autograd's arenas (uint8 mask) and
    accumulated in place (bool mask)."""
    _run(case, mode, inplace, mask_name, 4)


@pytest.mark.parametrize("mode,inplace", [("train", True), ("pair", False)])
def test_teacher_rollout_is_the_loop_at_h36m(mode, inplace):
    """The two-encoder H36M model (the split-f16 kernels), horizon 30: two
    windows, the second cut to five frames, a mixed mask."""
    _run("h36m", mode, inplace, "mixed", 4 if mode == "pair" else 2)


# ---- 2. degenerate masks ----------------------------------------------------------------
@pytest.mark.parametrize("mode", ["train", "pair"])
def test_an_all_zero_mask_is_the_free_running_rollout(mode):
    m, Tin, V, H = case_model("T6-4-2")
    a, b = twins(m, "train")
    K, n = windows(6, Tin, H), 2
    truth = torch.full((n, Tin + H, V, 3), float("nan"), device=DEV)  # never read
    obs_a = [observations(n, Tin, V, 90 + i).requires_grad_() for i in range(2 if mode == "pair" else 1)]
    obs_b = [o.detach().clone().requires_grad_() for o in obs_a]
    mask = mask_of("zero", K, n * len(obs_a), False)
    if mode == "pair":
        out_a, out_b = a.rollout_pair(*obs_a, H, teacher=truth, teacher_mask=mask), b.rollout_pair(*obs_b, H)
    else:
        out_a, out_b = (a.rollout(obs_a[0], H, truth, mask),), (b.rollout(obs_b[0], H),)
    for x, y in zip(out_a, out_b):
        _equal(x, y, f"all-zero {mode}: out")
    _loss(out_a).backward()
    _loss(out_b).backward()
    for x, y in zip(obs_a, obs_b):
        _equal(x.grad, y.grad, f"all-zero {mode}: observed.grad")
    _grads_equal(a, b, f"all-zero {mode}")
    _state_equal(a, b, f"all-zero {mode}")


def test_dropout_seeds_are_drawn_as_in_the_free_running_chain():
    """Dropout 0.1: under one torch seed the teacher's chain with an all-zero
    mask draws the free-running chain's per-window seeds -- the same outputs and
    gradients -- and the backward regenerates the masks of a mixed run (its
    gradients are finite and repeat under the same seed)."""
    m, Tin, V, H = case_model("T6-4-2")
    a, b = twins(m, "train")
    for x in (a, b):
        x.do_in.p = 0.1
    K, n = windows(6, Tin, H), 4
    truth, obs = observations(n, Tin + H, V, 97), observations(n, Tin, V, 98)
    runs = []
    for net, kw in ((a, dict(teacher=truth, teacher_mask=mask_of("zero", K, n, False))), (b, {}),
                    (a, dict(teacher=truth, teacher_mask=mask_of("mixed", K, n, False))),
                    (b, dict(teacher=truth, teacher_mask=mask_of("mixed", K, n, False)))):
        o = obs.clone().requires_grad_()
        net.zero_grad()
        torch.manual_seed(5)
        out = net.rollout(o, H, **kw)
        _loss([out]).backward()
        runs.append((out.detach(), o.grad, [p.grad.clone() for p in net.parameters() if p.grad is not None]))
    for i, j in ((0, 1), (2, 3)):
        _equal(runs[i][0], runs[j][0], f"dropout: out {i} {j}")
        _equal(runs[i][1], runs[j][1], f"dropout: observed.grad {i} {j}")
        assert all(torch.equal(x, y) and bool(torch.isfinite(x).all()) for x, y in zip(runs[i][2], runs[j][2]))
    assert not torch.equal(runs[0][0], runs[2][0])


@pytest.mark.parametrize("case", ["T6-4-2", "T6-1-5"])
def test_an_all_one_mask_is_one_window_rollouts_of_the_truth(case):
    """Window k's slice of out is a one-window rollout from
    teacher[:, k Tout : k Tout + Tin], run in window order on a twin (the
    running statistics too); observed.grad is window 0's gradient alone; and
    nothing after window 0 depends on the observations."""
    m, Tin, V, H = case_model(case)
    a, b, c = twins(m, "train", count=3)
    Tout, n = a.output_time_frame, 4
    K = windows(Tin + Tout, Tin, H)
    truth = observations(n, Tin + H, V, 91)
    mask = mask_of("one", K, n, False)
    obs = observations(n, Tin, V, 92).requires_grad_()
    out = a.rollout(obs, H, teacher=truth, teacher_mask=mask)
    assert bool(torch.isfinite(out).all())
    with torch.no_grad():
        for k in range(K):
            take = min(Tout, H - k * Tout)
            src = obs.detach() if k == 0 else truth[:, k * Tout:k * Tout + Tin].contiguous()
            _equal(out[:, k * Tout:k * Tout + take], b.rollout(src, take), f"{case}: window {k}")
    _state_equal(a, b, f"{case}: all-one buffers")
    _loss([out]).backward()
    obs_c = obs.detach().clone().requires_grad_()
    (c.rollout(obs_c, Tout).square().sum() / out.numel()).backward()
    _equal(obs.grad, obs_c.grad, f"{case}: observed.grad is window 0's")
    assert all(bool(torch.isfinite(p.grad).all()) for p in a.parameters() if p.grad is not None)
    with torch.no_grad():  # other observations: windows 1 .. K-1 see the truth alone, batch statistics included
        other = a.rollout(observations(n, Tin, V, 93), H, teacher=truth, teacher_mask=mask)
    assert torch.equal(other[:, Tout:], out[:, Tout:]) and not torch.equal(other[:, :Tout], out[:, :Tout])


def test_a_forced_sample_does_not_see_its_prediction():
    """Eval mode under autograd (no batch statistics couple the samples): sample
    1 is forced at every boundary onto a constant truth.  Changing its
    observations changes its window 0 and nothing else -- its later windows are
    the truth's, the free samples' outputs are untouched -- and no gradient
    reaches its observations from beyond window 0."""
    m, Tin, V, H = case_model("T6-4-2")
    (a,) = twins(m, "eval", count=1)
    Tout, n = a.output_time_frame, 3
    K = windows(Tin + Tout, Tin, H)
    truth = observations(n, Tin + H, V, 94)
    truth[1] = 0.25
    mask = torch.zeros(K, n, dtype=torch.uint8, device=DEV)
    mask[:, 1] = 1
    obs = observations(n, Tin, V, 95)
    obs2 = obs.clone()
    obs2[1] = observations(1, Tin, V, 96)[0]
    o1 = obs.clone().requires_grad_()
    out1 = a.rollout(o1, H, teacher=truth, teacher_mask=mask)
    out2 = a.rollout(obs2.requires_grad_(), H, teacher=truth, teacher_mask=mask)
    assert torch.equal(out1[[0, 2]], out2[[0, 2]]) and torch.equal(out1[1, Tout:], out2[1, Tout:])
    assert not torch.equal(out1[1, :Tout], out2[1, :Tout])
    free = a.rollout(obs, H, teacher=truth, teacher_mask=torch.zeros_like(mask))
    assert torch.equal(free[[0, 2]], out1[[0, 2]]) and not torch.equal(free[1, Tout:], out1[1, Tout:])
    out1[:, Tout:].square().sum().backward()  # a loss on windows 1 .. K-1 alone
    assert float(o1.grad[1].abs().max()) == 0 and float(o1.grad[0].abs().max()) > 0


# ---- 3. the backward glue alone ------------------------------------------------------
@pytest.mark.parametrize("Tin,Tout", SMALL)
def test_masked_backward_glue_is_the_restatement(Tin, Tout):
    """Steps 0 and 1 through the test hook with a mask row, step 2 as it is, on
    random dout / G, B = 3, V = 1, 22, 25 (rows of 3, 66 and 75 floats: below,
    just above and above one pass of a wave's lanes): equal to the fp32
    restatement exactly, and within (Tout + 2) * 2^-24 * sum |terms| of the fp64
    closed form elementwise -- the bound of tests/test_gpu_rollout.py for a
    sequential sum of at most Tout + 2 terms."""
    L, st = native.lib(), native.stream_handle(torch.device(DEV))
    T, B, H = Tin + Tout, 3, 3 * Tout - 1 if Tout > 1 else 3
    K = windows(T, Tin, H)
    u = (Tout + 2) * 2.0 ** -24

    def check(got, f, args, what):
        got = got.cpu().numpy()
        assert np.array_equal(got, f(*args)), what
        a64 = [a.astype(np.float64) if isinstance(a, np.ndarray) and a.dtype == np.float32 else a for a in args]
        mag = [np.abs(a) if isinstance(a, np.ndarray) and a.dtype == np.float64 else a for a in a64]
        assert (np.abs(got.astype(np.float64) - f(*a64)) <= u * f(*mag)).all(), what

    for V in (1, 22, 25):
        rng = np.random.default_rng(2000 * Tin + 10 * Tout + V)
        dout = rng.standard_normal((B, H, V, 3)).astype(np.float32)
        Gn = rng.standard_normal((B, T, V, 3)).astype(np.float32)
        dx = rng.standard_normal((B, T, V, 3)).astype(np.float32)
        d_dout, d_Gn = torch.from_numpy(dout).to(DEV), torch.from_numpy(Gn).to(DEV)
        for row in ([1, 0, 1], [0, 1, 0]):
            mrow = np.array(row, np.uint8)
            d_mrow = torch.from_numpy(mrow).to(DEV)
            for k in range(K):
                gn, d_gn = (None, None) if k == K - 1 else (Gn, d_Gn.data_ptr())
                dy = torch.full((B, T, V, 3), float("nan"), device=DEV)
                assert L.dstd_model_rollout_tf_glue_bwd(0, d_dout.data_ptr(), d_gn, dy.data_ptr(), d_mrow.data_ptr(), B, T,
                                                        Tin, V, H, k, st) == 0
                check(dy, glue_dy_tf, (dout, gn, mrow, T, Tin, k), f"dy V{V} k{k} {row}")
            G = torch.from_numpy(dx).to(DEV)
            assert L.dstd_model_rollout_tf_glue_bwd(1, None, d_Gn.data_ptr(), G.data_ptr(), d_mrow.data_ptr(), B, T, Tin, V,
                                                    H, 0, st) == 0
            check(G, glue_fold_tf, (dx, Gn, mrow, T, Tin), f"fold V{V} {row}")
            dobs = torch.full((B, Tin, V, 3), float("nan"), device=DEV)
            assert L.dstd_model_rollout_tf_glue_bwd(2, None, d_Gn.data_ptr(), dobs.data_ptr(), d_mrow.data_ptr(), B, T, Tin,
                                                    V, H, 0, st) == 0
            check(dobs, glue_obs, (Gn, T, Tin), f"dobs V{V}")
            assert torch.equal(d_mrow.cpu(), torch.from_numpy(mrow))
        # no mask row: the free-running hook
        dy = torch.full((B, T, V, 3), float("nan"), device=DEV)
        assert L.dstd_model_rollout_tf_glue_bwd(0, d_dout.data_ptr(), d_Gn.data_ptr(), dy.data_ptr(), None, B, T, Tin, V, H,
                                                0, st) == 0
        check(dy, glue_dy_tf, (dout, Gn, None, T, Tin, 0), f"dy V{V} no row")
        assert torch.equal(d_Gn.cpu(), torch.from_numpy(Gn)) and torch.equal(d_dout.cpu(), torch.from_numpy(dout))


# ---- 4. the entry points: memory contract, refusals ------------------------------------
def _ints(a, b):
    return (ctypes.c_int * 2)(a, b)


def teacher_call(m, obs, dout, H, flags, truth, maps, mask, fill, short=None, stepwise=False, bad=None):
    """dstd_model_rollout_tf_fwd and _tf_bwd on exact-size guarded buffers, truth
    and mask guarded too.  ``short`` names a size to pass one byte short first,
    ``bad`` is {name: teacher arguments that must be DSTD_EINVAL}, tried in both
    directions: those calls must be refused with nothing written and nothing
    left pending, and the valid call follows on the same buffers.  ``stepwise``: the backward as K
    calls of dstd_model_rollout_tf_bwd_window."""
    L, st = native.lib(), native.stream_handle(obs.device)
    B, Tin, V, _ = obs.shape
    T, C, layers = Tin + m.output_time_frame, m.num_feature, m.num_layers
    K = windows(T, Tin, H)
    b = Bufs()
    p = native.ModelParams.from_buffer_copy(m._native_params())
    stats = _guard_model_stats(b, p, m)
    pref = native.ext.model_params_ref(p)
    ns = L.dstd_model_rollout_saved_bytes(B, T, V, C, layers, K)
    nw = L.dstd_model_rollout_workspace_bytes(B, T, V, C, layers)
    saved = b.new("saved", ns, fill)
    out = b.f32("out", (B, H, V, 3), NAN_OUT)
    d_truth = b.f32("truth", truth.shape, 0, like=truth)
    g_mask = b.new("mask", mask.numel(), 0)
    g_mask.tensor.copy_(mask.reshape(-1))
    tf = (d_truth.data_ptr(), truth.shape[1], _ints(*[x[0] for x in maps]), _ints(*[x[1] for x in maps]), g_mask.ptr)

    def refused(code, want, what):
        torch.cuda.synchronize()  # nothing pending either
        assert code == want, (what, code)
        b.check_frozen(snap, what)

    fwd = lambda n, t: L.dstd_model_rollout_tf_fwd(pref, obs.data_ptr(), B, Tin, H, 0.1, 0.0, None, out.data_ptr(),  # noqa: E731
                                                   saved.ptr, n, *t, st, flags)
    if short == "saved fwd":
        snap = b.freeze()
        refused(fwd(ns - 1, tf), EWORKSPACE, short)
    for name, alter in (bad or {}).items():
        snap = b.freeze()
        refused(fwd(ns, alter(tf)), EINVAL, "fwd: " + name)
    native.check(fwd(ns, tf), "dstd_model_rollout_tf_fwd")
    torch.cuda.synchronize()
    saved0, stats0, truth0, mask0 = saved.tensor.clone(), _clones(stats), d_truth.clone(), g_mask.tensor.clone()
    ws = b.new("workspace", nw, fill)
    dobs = b.f32("dobs", obs.shape, NAN_OUT)
    params = list(m.parameters())
    arena = native.GradArena(params, obs.device, buf=b.f32("gradient arena", (native.arena_numel(params),), 0))
    gref = native.ext.model_grads_ref(m._native_grads(arena))
    args = lambda a, c, t: (pref, B, Tin, H, 0.0, None, saved.ptr, a, dout.data_ptr(), gref, dobs.data_ptr(), ws.ptr, c,  # noqa: E731
                            *t, st, flags)
    if short in ("saved bwd", "workspace"):
        snap = b.freeze()
        refused(L.dstd_model_rollout_tf_bwd(*(args(ns - 1, nw, tf) if short == "saved bwd" else args(ns, nw - 1, tf))),
                EWORKSPACE, short)
    for name, alter in (bad or {}).items():
        snap = b.freeze()
        a = args(ns, nw, alter(tf))
        refused(L.dstd_model_rollout_tf_bwd(*a), EINVAL, "bwd: " + name)
        refused(L.dstd_model_rollout_tf_bwd_window(*a[:4], K - 1, *a[4:]), EINVAL, "bwd_window: " + name)
    if stepwise:
        a = args(ns, nw, tf)
        for k in range(K - 1, -1, -1):
            native.check(L.dstd_model_rollout_tf_bwd_window(*a[:4], k, *a[4:]), "dstd_model_rollout_tf_bwd_window")
    else:
        native.check(L.dstd_model_rollout_tf_bwd(*args(ns, nw, tf)), "dstd_model_rollout_tf_bwd")
    b.check()  # (synchronises) no write outside out, saved, dobs, the workspace or the arena
    assert torch.equal(saved.tensor, saved0), "the backward wrote to saved"
    assert torch.equal(g_mask.tensor, mask0) and torch.equal(g_mask.tensor, mask.reshape(-1)), "mask was written"
    assert torch.equal(d_truth.view(torch.int32), truth0.view(torch.int32)) and torch.equal(d_truth, truth), "truth was written"
    _unchanged(stats, stats0, "running statistics across the backward")
    res = {"out": out, "dobs": dobs}
    res.update({f"stat{i}": s for i, s in enumerate(stats)})
    res.update({"grad " + n: g for (n, _), g in zip(m.named_parameters(), arena.views()) if g is not None})
    return _keep(res)


def _contract_case(case, flags, seed):
    m, Tin, V, H = case_model(case)
    m.train(not flags & native.TRAIN_RUNNING_STATS)
    B = 4
    pair = bool(flags & native.TRAIN_PAIRED)
    Bt = B // 2 if pair else B
    K = windows(Tin + m.output_time_frame, Tin, H)
    obs, dout = observations(B, Tin, V, seed), observations(B, H, V, seed + 1)
    truth = observations(Bt, Tin + H, V, seed + 2)
    maps = [(0, 1), (Tin + H - 1, -1)] if pair else [(0, 1), (0, 0)]
    mask = mask_of("mixed", K, B, pair)
    return m, obs, dout, H, truth, maps, mask


@pytest.mark.parametrize("case,flags", [("T6-4-2", 0), ("T6-5-1", native.TRAIN_PAIRED),
                                        ("T6-3-3", native.TRAIN_RUNNING_STATS), ("T6-1-5", native.TRAIN_ONE_STREAM)],
                         ids=["T6-4-2", "T6-5-1-paired", "T6-3-3-running", "T6-1-5-one-stream"])
def test_teacher_memory_contract(case, flags):
    """Exact-size saved / out / dobs / workspace / arena / truth / mask between
    sentinel guards: nothing is written outside them, the results do not depend
    on what saved and the workspace held before (0x00, 0xFF, 0x4B), the backward
    leaves saved, the mask, the truth and the running statistics alone, the
    inputs are not written; one window per call gives the same bits."""
    m, obs, dout, H, truth, maps, mask = _contract_case(case, flags, 101)
    inputs = [obs, dout, truth, mask] + list(m.parameters()) + list(m.buffers())
    before = _clones(inputs)
    what = f"teacher {case} flags {flags}"
    got = run_fills(lambda fill: teacher_call(m, obs, dout, H, flags, truth, maps, mask, fill), what)
    _unchanged(inputs, before, what)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (what, k)
    _same(got, teacher_call(m, obs, dout, H, flags, truth, maps, mask, 0xFF, stepwise=True), what + ": stepwise")
    assert float(got["dobs"].abs().max()) > 0


def test_teacher_size_checks_and_refusals():
    """Each size one byte short is DSTD_EWORKSPACE and each new DSTD_EINVAL of
    the header is refused, with nothing written and nothing left pending, in
    both directions; the valid call on the same buffers then gives the
    reference result."""
    m, obs, dout, H, truth, maps, mask = _contract_case("T6-5-1", native.TRAIN_PAIRED, 111)
    flags = native.TRAIN_PAIRED
    Ttot = truth.shape[1]
    base = teacher_call(m, obs, dout, H, flags, truth, maps, mask, 0x4B)
    for short in ("saved fwd", "saved bwd", "workspace"):
        _same(base, teacher_call(m, obs, dout, H, flags, truth, maps, mask, 0x4B, short=short), short)
    bads = {
        "truth alone": lambda t: (t[0], *t[1:4], None),
        "mask alone": lambda t: (None, *t[1:]),
        "no frame map": lambda t: (*t[:2], None, t[3], t[4]),
        "step 0": lambda t: (*t[:3], _ints(1, 0), t[4]),
        "step 2": lambda t: (*t[:3], _ints(2, -1), t[4]),
        "one frame short": lambda t: (t[0], Ttot - 2, *t[2:]),  # the first half's last read is frame Ttot - 2
        "second half below frame 0": lambda t: (*t[:2], _ints(0, Ttot - 3), *t[3:]),
        "first half before frame 0": lambda t: (*t[:2], _ints(-2, Ttot - 1), *t[3:]),
    }
    _same(base, teacher_call(m, obs, dout, H, flags, truth, maps, mask, 0x4B, bad=bads), "after the refusals")


# ---- 5. the engine ------------------------------------------------------------------
def test_engine_teacher_step_is_the_hand_composed_step():
    """One train(horizon=12, teacher_ratio=0.5) step (four windows, the inverse
    pass) under torch.manual_seed against the step composed by hand on a twin
    from the same draw: losses and every parameter and buffer, bit for bit."""
    from engine.loss import prepare_joint_weights, weighted_losses
    from test_gpu_rollout import _engine_setup
    eng, hand, loader, weights = _engine_setup(15, 41)
    steps, step = [], eng._step_rollout
    eng._step_rollout = lambda *a: steps.append(step(*a)) or steps[-1]
    torch.manual_seed(1234)
    total = eng.train(loader, 0, weights=weights, horizon=12, teacher_ratio=0.5)
    assert len(steps) == 1 and np.isfinite(total)

    inputs, inputs_inv, targets, _ = next(iter(loader))
    net = hand.model.model
    torch.manual_seed(1234)
    mask = torch.rand(4, 4, device=DEV) < 0.5
    assert 0 < int(mask[1:].sum()) < mask[1:].numel()
    net._dstd_inplace_grads = True
    try:
        x, xi = hand.transform(inputs.float()), hand.transform(inputs_inv.float())
        o1, o2 = net.rollout_pair(x[:, :3].contiguous(), xi[:, :3].contiguous(), 12,
                                  teacher=hand.transform(targets.float()), teacher_mask=mask)
        out = weighted_losses(hand.model.loss_spec, [hand.inverse(o1), hand.inverse(o2)], targets.float(),
                              [(3, 1), (11, -1)], prepare_joint_weights(weights, DEV))
        hand.optimizer.zero_grad()
        (out.sum() / 2).backward()
        hand.optimizer.step()
    finally:
        net._dstd_inplace_grads = False
    got = torch.stack([v.reshape(()) for v in steps[0]])
    assert got.shape == (2,) and bool((got > 0).all())
    assert torch.equal(got, out[0].detach()), (got, out[0])
    _state_equal(eng.model.model, net, "engine step, teacher_ratio 0.5")
    # and it is another step than the free-running one
    free, _, _, _ = _engine_setup(15, 41)
    free.train(loader, 0, weights=weights, horizon=12)
    assert any(not torch.equal(p, q) for p, q in zip(free.model.model.parameters(), net.parameters()))


def test_engine_teacher_ratio_zero_is_the_free_running_step():
    from test_gpu_rollout import _engine_setup
    eng, twin, loader, weights = _engine_setup(15, 42)
    state = torch.cuda.get_rng_state(DEV)
    a = eng.train(loader, 0, weights=weights, horizon=12, teacher_ratio=0)
    assert torch.equal(torch.cuda.get_rng_state(DEV), state)  # no mask is drawn
    b = twin.train(loader, 0, weights=weights, horizon=12)
    assert a == b
    _state_equal(eng.model.model, twin.model.model, "teacher_ratio 0")
    with pytest.raises(ValueError, match="teacher_ratio"):
        eng.train(loader, 0, weights=weights, horizon=12, teacher_ratio=1.01)
