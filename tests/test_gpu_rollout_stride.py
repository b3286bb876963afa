"""Training through a strided rollout on the GPU
(include/ext/dstd_gcn_stride_train.h, DSTDGCN.rollout / rollout_pair(stride=),
PredictionEngine.train(horizon=, stride=, teacher_ratio=)).

The reference of every comparison is the loop a caller writes without the
feature (tests/rollout_stride_helper.py StridedLoop: ``model(x_k)`` per window on
a detached leaf built with torch indexing, and the backward composed by hand in
the header's order).  Both sides issue the same native forward and backward
calls on the same bits in the same order, so outputs, BatchNorm buffers and
gradients are compared with torch.equal throughout.

Shapes: T = 6 models (V = 5, C = 8, one layer) with B = 4 (a pair: 2 + 2) at
(Tin, Tout, S, H) = (4, 2, 1, 6) -- every frame is read by four windows --,
(3, 3, 2, 7) -- a truncated last window --, (3, 3, 1, 5), (1, 5, 2, 9) -- Tin < S
-- and (2, 4, 3, 2) -- H < S, one window; K <= 6 windows, so that random-weight
outputs stay finite.  Masks: none, all-zero, all-one and a fixed mixed pattern.
And the two-encoder h36m model at T = 35, B = 2, S = 10, H = 30.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import dstd_native as native
from rollout_stride_helper import glue_acc, glue_dy, model_loop, model_loop_pair, windows
from teacher_helper import mixed_mask
from test_gpu_guards import NAN_OUT, Bufs, _clones, _guard_model_stats, _keep, _on_gpu, _same, _unchanged, run_fills, synth_model
from test_gpu_predict import small_model
from test_gpu_rollout import _equal, _grads_equal, _state_equal, observations

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, EWORKSPACE = -1, -2  # include/dstd_gcn.h
SMALL = [(4, 2, 1, 6), (3, 3, 2, 7), (3, 3, 1, 5), (1, 5, 2, 9), (2, 4, 3, 2)]  # (Tin, Tout, S, H)
CASES = ["T6-%d-%d-S%d-H%d" % c for c in SMALL]
MASKS = ("none", "zero", "one", "mixed")


def case_model(case):
    """(model on the GPU in eval mode, Tin, V, stride, horizon)"""
    if case == "h36m":
        return _on_gpu(synth_model(35, 22, 2)), 10, 22, 10, 30
    Tin, Tout, S, H = (int(s.lstrip("SH")) for s in case.split("-")[1:])
    return small_model(Tin, Tout), Tin, 5, S, H


def mask_of(name, K, N, pair):
    if name == "none":
        return None
    if name == "mixed" and K == 1:  # row 0 is not read: any pattern
        return torch.from_numpy(np.arange(N, dtype=np.uint8).reshape(1, N) % 2).to(DEV)
    m = {"zero": np.zeros((K, N), np.uint8), "one": np.ones((K, N), np.uint8),
         "mixed": mixed_mask(K, N, N // 2 if pair else None) if K > 1 else None}[name]
    return torch.from_numpy(m).to(DEV)


def twins(m, mode, inplace=False, one_stream=False, count=2):
    out = [m] + [copy.deepcopy(m) for _ in range(count - 1)]
    for x in out:
        x.train(mode != "eval")
        x.do_in.p = 0.0  # gradient comparisons: no dropout (the chain and the loop draw their own seeds)
        x._dstd_inplace_grads = inplace
        x._dstd_one_stream = one_stream
    return out


def _loss(outs):
    return sum(o.square().sum() for o in outs) / sum(o.numel() for o in outs) * len(outs)


def _run(case, mode, inplace, mask_name, B, one_stream=False):
    """One forward and backward of the strided chain and of the loop on twin models."""
    m, Tin, V, S, H = case_model(case)
    a, b = twins(m, mode, inplace, one_stream)
    K = windows(H, S)
    what = f"{case} {mode} inplace={inplace} mask={mask_name} one_stream={one_stream}"
    n0 = int(a.bn_in.bn.num_batches_tracked)
    pair = mode == "pair"
    n = B // 2 if pair else B
    mask = mask_of(mask_name, K, B, pair)
    truth = observations(n, Tin + H, V, 81) if mask is not None else None
    tf = {} if mask is None else dict(teacher=truth, teacher_mask=mask.bool() if inplace else mask)
    before = _clones([truth, mask]) if mask is not None else []
    obs_a = [observations(n, Tin, V, 82 + i).requires_grad_() for i in range(2 if pair else 1)]
    obs_b = [o.detach().clone() for o in obs_a]
    if pair:
        out_a = a.rollout_pair(*obs_a, H, stride=S, **tf)
        loop = model_loop_pair(b, *obs_b, H, S, truth, mask)
        out_b = (loop.out[:n], loop.out[n:])
    else:
        out_a = (a.rollout(obs_a[0], H, stride=S, **tf),)
        loop = model_loop(b, obs_b[0], H, S, truth, mask)
        out_b = (loop.out,)
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert x.shape == (n, H, V, 3)
        _equal(x, y, f"{what}: out {i}")
    _state_equal(a, b, what + ": buffers after the forward")
    calls = 0 if mode == "eval" else K * (2 if pair else 1)
    assert int(a.bn_in.bn.num_batches_tracked) == n0 + calls
    _loss(out_a).backward()
    leaves = [o.detach().clone().requires_grad_() for o in out_b]
    _loss(leaves).backward()
    dobs = loop.backward(torch.cat([o.grad for o in leaves]), list(b.parameters()))
    torch.cuda.synchronize()
    for i, x in enumerate(obs_a):
        want = dobs[i * n:(i + 1) * n]
        assert float(want.abs().max()) > 0
        _equal(x.grad, want, f"{what}: observed.grad {i}")
    _grads_equal(a, b, what)
    _state_equal(a, b, what + ": after the backward")
    if mask is not None:
        _unchanged([truth, mask], before, what + ": teacher and mask")
        assert truth.grad is None


# ---- 1. the chain is the loop ---------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["autograd", "inplace"])
@pytest.mark.parametrize("mode", ["train", "pair", "eval"])
@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("case", CASES)
def test_strided_rollout_is_the_loop(case, mask_name, mode, inplace):
    """Outputs, running statistics, num_batches_tracked, observed.grad and every
    parameter's .grad of rollout / rollout_pair(stride=) against the loop, free
    running and for each of the three masks: in train mode, as a pair, and in
    eval mode under autograd; gradients through autograd's arenas (one per
    window, uint8 mask) and accumulated in place (bool mask)."""
    _run(case, mode, inplace, mask_name, 4)


@pytest.mark.parametrize("inplace", [False, True], ids=["autograd", "inplace"])
@pytest.mark.parametrize("case", CASES[:2])
def test_strided_rollout_is_the_loop_on_one_stream(case, inplace):
    _run(case, "train", inplace, "mixed", 4, one_stream=True)


@pytest.mark.parametrize("mode,inplace", [("train", True), ("pair", False)])
def test_strided_rollout_is_the_loop_at_h36m(mode, inplace):
    """The two-encoder H36M model (the split-f16 kernels), S = 10, H = 30: three
    windows, every predicted frame below 20 observed by the next window, a mixed mask."""
    _run("h36m", mode, inplace, "mixed", 4 if mode == "pair" else 2)


# ---- 2. degenerate masks, and the stride of a whole window ---------------------------
@pytest.mark.parametrize("mode", ["train", "pair"])
def test_an_all_zero_mask_is_the_maskless_call(mode):
    m, Tin, V, S, H = case_model(CASES[0])
    a, b = twins(m, "train")
    K, n = windows(H, S), 2
    truth = torch.full((n, Tin + H, V, 3), float("nan"), device=DEV)  # never read
    obs_a = [observations(n, Tin, V, 90 + i).requires_grad_() for i in range(2 if mode == "pair" else 1)]
    obs_b = [o.detach().clone().requires_grad_() for o in obs_a]
    mask = mask_of("zero", K, n * len(obs_a), False)
    if mode == "pair":
        out_a = a.rollout_pair(*obs_a, H, teacher=truth, teacher_mask=mask, stride=S)
        out_b = b.rollout_pair(*obs_b, H, stride=S)
    else:
        out_a, out_b = (a.rollout(obs_a[0], H, truth, mask, S),), (b.rollout(obs_b[0], H, stride=S),)
    for x, y in zip(out_a, out_b):
        _equal(x, y, f"all-zero {mode}: out")
    _loss(out_a).backward()
    _loss(out_b).backward()
    for x, y in zip(obs_a, obs_b):
        _equal(x.grad, y.grad, f"all-zero {mode}: observed.grad")
    _grads_equal(a, b, f"all-zero {mode}")
    _state_equal(a, b, f"all-zero {mode}")


@pytest.mark.parametrize("case", [CASES[0], CASES[3]])
def test_an_all_one_mask_cuts_every_boundary(case):
    """observed.grad is window 0's gradient alone (a one-window rollout of the
    first S frames on a twin), and nothing after window 0 depends on the
    observations: other observations leave out[:, S:] as it is, batch statistics
    included."""
    m, Tin, V, S, H = case_model(case)
    a, c = twins(m, "train")
    n, K = 4, windows(H, S)
    truth = observations(n, Tin + H, V, 91)
    mask = mask_of("one", K, n, False)
    obs = observations(n, Tin, V, 92).requires_grad_()
    out = a.rollout(obs, H, teacher=truth, teacher_mask=mask, stride=S)
    assert bool(torch.isfinite(out).all())
    _loss([out]).backward()
    obs_c = obs.detach().clone().requires_grad_()
    first = c.rollout(obs_c, S, stride=S)
    _equal(out[:, :S], first, f"{case}: window 0")
    (first.square().sum() / out.numel()).backward()
    _equal(obs.grad, obs_c.grad, f"{case}: observed.grad is window 0's")
    with torch.no_grad():
        other = a.rollout(observations(n, Tin, V, 93), H, teacher=truth, teacher_mask=mask, stride=S)
    assert torch.equal(other[:, S:], out[:, S:]) and not torch.equal(other[:, :S], out[:, :S])


def test_a_forced_sample_does_not_see_its_observations_again():
    """Eval mode under autograd (no batch statistics couple the samples): sample
    1 is forced at every boundary.  Changing its observations changes its window
    0 and nothing else, and no gradient reaches them from beyond window 0 --
    although at S = 1 < Tin = 4 a free sample's windows 1 .. 3 still read them."""
    m, Tin, V, S, H = case_model(CASES[0])
    (a,) = twins(m, "eval", count=1)
    n, K = 3, windows(H, S)
    truth = observations(n, Tin + H, V, 94)
    mask = torch.zeros(K, n, dtype=torch.uint8, device=DEV)
    mask[:, 1] = 1
    obs = observations(n, Tin, V, 95)
    obs2 = obs.clone()
    obs2[1] = observations(1, Tin, V, 96)[0]
    o1 = obs.clone().requires_grad_()
    out1 = a.rollout(o1, H, teacher=truth, teacher_mask=mask, stride=S)
    out2 = a.rollout(obs2.requires_grad_(), H, teacher=truth, teacher_mask=mask, stride=S)
    assert torch.equal(out1[[0, 2]], out2[[0, 2]]) and torch.equal(out1[1, S:], out2[1, S:])
    assert not torch.equal(out1[1, :S], out2[1, :S])
    out1[:, S:].square().sum().backward()  # a loss on windows 1 .. K-1 alone
    assert float(o1.grad[1].abs().max()) == 0 and float(o1.grad[0].abs().max()) > 0


def _record_chain_calls(monkeypatch):
    """The nine chain entry points of native.lib() behind pass-throughs that
    note (name, arguments) of every call, for the duration of the test."""
    L, calls = native.lib(), []
    for family in ("", "_tf", "_strided"):
        for step in ("fwd", "bwd", "bwd_window"):
            name = f"dstd_model_rollout{family}_{step}"

            def through(*args, _fn=getattr(L, name), _name=name):
                calls.append((_name, args))
                return _fn(*args)
            monkeypatch.setattr(L, name, through)
    return calls


def test_a_stride_of_a_whole_window_is_the_existing_function_and_eval_is_predict(monkeypatch):
    """Which entry points a call reaches, and in which order: stride None and
    ``output_time_frame`` the plain ones, with a teacher the _tf_ ones, a stride
    below a window the _strided_ ones with a teacher and without; one forward,
    then one _bwd in the in-place gradient mode, or K _bwd_window with
    k = K - 1 .. 0 for autograd; for rollout and rollout_pair alike."""
    m, Tin, V, S, H = case_model(CASES[1])
    a, b = twins(m, "train")
    obs = observations(2, Tin, V, 97)
    truth = observations(2, Tin + H, V, 98)
    calls = _record_chain_calls(monkeypatch)
    for pair in (False, True):
        for stride, teacher, family in ((None, False, ""), (a.output_time_frame, False, ""), (None, True, "_tf"),
                                        (S, False, "_strided"), (S, True, "_strided")):
            K = windows(H, stride or a.output_time_frame)
            tf = dict(teacher=truth, teacher_mask=mask_of("mixed", K, 4 if pair else 2, pair)) if teacher else {}
            for inplace in (False, True):
                a._dstd_inplace_grads = inplace
                a.zero_grad(set_to_none=True)  # (gradients of the other mode would keep the in-place one out)
                del calls[:]
                leaves = [obs.clone().requires_grad_() for _ in range(2 if pair else 1)]
                outs = a.rollout_pair(*leaves, H, stride=stride, **tf) if pair else (
                    a.rollout(leaves[0], H, stride=stride, **tf),)
                _loss(outs).backward()
                stem = f"dstd_model_rollout{family}_"
                want = [stem + "fwd"] + ([stem + "bwd"] if inplace else [stem + "bwd_window"] * K)
                what = f"pair={pair} stride={stride} teacher={teacher} inplace={inplace}"
                assert [name for name, _ in calls] == want, what
                if not inplace:  # (params, B, input_n, horizon[, stride], k, ...)
                    at = 5 if family == "_strided" else 4
                    assert [args[at] for _, args in calls[1:]] == list(range(K - 1, -1, -1)), what
    a._dstd_inplace_grads = False
    b.eval()
    with torch.no_grad():
        _equal(b.rollout(obs, H, stride=S), b.predict(obs, H, stride=S), "eval, nothing to differentiate")
    with pytest.raises(TypeError):
        a.rollout(obs, H, None, None, S, 1)  # stride is the last argument


# ---- 3. the backward glue alone ------------------------------------------------------
@pytest.mark.parametrize("Tin,Tout,S,H", SMALL)
def test_backward_glue_is_the_restatement(Tin, Tout, S, H):
    """Both steps through the test hook on random Gh / dx / dout, B = 3, V = 1, 22,
    25 (rows of 3, 66 and 75 floats: below, just above and above one pass of a
    wave's lanes), every window, with a mask row and without: equal to the fp32
    numpy restatement exactly; dout, dx and the mask row are not written."""
    L, st = native.lib(), native.stream_handle(torch.device(DEV))
    T, B, K = Tin + Tout, 3, windows(H, S)
    for V in (1, 22, 25):
        rng = np.random.default_rng(3000 * Tin + 100 * S + V)
        dout = rng.standard_normal((B, H, V, 3)).astype(np.float32)
        Gh = rng.standard_normal((B, Tin + H, V, 3)).astype(np.float32)
        dx = rng.standard_normal((B, T, V, 3)).astype(np.float32)
        d_dout, d_dx = torch.from_numpy(dout).to(DEV), torch.from_numpy(dx).to(DEV)
        for row in ([1, 0, 1], [0, 1, 0], None):
            mrow = None if row is None else np.array(row, np.uint8)
            d_mrow = None if row is None else torch.from_numpy(mrow).to(DEV)
            for k in range(K):
                what = f"V{V} k{k} {row}"
                d_Gh = torch.from_numpy(Gh).to(DEV)
                dy = torch.full((B, T, V, 3), float("nan"), device=DEV)
                assert L.dstd_model_rollout_strided_glue_bwd(0, d_dout.data_ptr(), None, d_Gh.data_ptr(), dy.data_ptr(),
                                                             None, B, T, Tin, V, H, S, k, st) == 0
                assert np.array_equal(dy.cpu().numpy(), glue_dy(Gh, dout, T, Tin, S, k)), "dy " + what
                assert np.array_equal(d_Gh.cpu().numpy(), Gh), "step 0 wrote Gh " + what
                dobs = torch.full((B, Tin, V, 3), float("nan"), device=DEV)
                assert L.dstd_model_rollout_strided_glue_bwd(1, None, d_dx.data_ptr(), d_Gh.data_ptr(), dobs.data_ptr(),
                                                             None if row is None else d_mrow.data_ptr(), B, T, Tin, V, H,
                                                             S, k, st) == 0
                want = glue_acc(Gh, dx, mrow, T, Tin, S, k)
                assert np.array_equal(d_Gh.cpu().numpy(), want), "Gh " + what
                if k == 0:
                    assert np.array_equal(dobs.cpu().numpy(), want[:, :Tin]), "dobs " + what
                else:
                    assert bool(torch.isnan(dobs).all()), "dobs is window 0's " + what
            if row is not None:
                assert torch.equal(d_mrow.cpu(), torch.from_numpy(mrow))
        assert torch.equal(d_dx.cpu(), torch.from_numpy(dx)) and torch.equal(d_dout.cpu(), torch.from_numpy(dout))


# ---- 4. the entry points: memory contract, refusals, S = Tout ---------------------------
def _ints(a, b):
    return (ctypes.c_int * 2)(a, b)


def strided_call(m, obs, dout, H, S, flags, truth, maps, mask, fill, short=None, stepwise=False, unstrided=False):
    """dstd_model_rollout_strided_fwd and _bwd on exact-size guarded buffers, truth
    and mask (None: free running) guarded too.  ``short`` names a size to pass
    one byte short first: that call must be refused with nothing written and
    nothing left pending, and the valid call follows on the same buffers.
    ``stepwise``: the backward as K calls of _bwd_window.  ``unstrided``: the
    same through dstd_model_rollout_fwd / _bwd (_tf_fwd / _tf_bwd with a mask),
    for S = Tout."""
    L, st = native.lib(), native.stream_handle(obs.device)
    B, Tin, V, _ = obs.shape
    T, C, layers = Tin + m.output_time_frame, m.num_feature, m.num_layers
    K = windows(H, S)
    b = Bufs()
    p = native.ModelParams.from_buffer_copy(m._native_params())
    stats = _guard_model_stats(b, p, m)
    pref = native.ext.model_params_ref(p)
    ns = L.dstd_model_rollout_saved_bytes(B, T, V, C, layers, K)
    nw = (L.dstd_model_rollout_workspace_bytes(B, T, V, C, layers) if unstrided else
          L.dstd_model_rollout_strided_workspace_bytes(B, T, V, C, layers, Tin, H))
    saved = b.new("saved", ns, fill)
    out = b.f32("out", (B, H, V, 3), NAN_OUT)
    tf = (None, 0, None, None, None)
    if mask is not None:
        d_truth = b.f32("truth", truth.shape, 0, like=truth)
        g_mask = b.new("mask", mask.numel(), 0)
        g_mask.tensor.copy_(mask.reshape(-1))
        tf = (d_truth.data_ptr(), truth.shape[1], _ints(*[x[0] for x in maps]), _ints(*[x[1] for x in maps]), g_mask.ptr)

    def refused(code, what):
        torch.cuda.synchronize()  # nothing pending either
        assert code == EWORKSPACE, (what, code)
        b.check_frozen(snap, what)

    def fwd(n):
        head = (pref, obs.data_ptr(), B, Tin, H)
        tail = (0.1, 0.0, None, out.data_ptr(), saved.ptr, n)
        if not unstrided:
            return L.dstd_model_rollout_strided_fwd(*head, S, *tail, *tf, st, flags)
        if mask is None:
            return L.dstd_model_rollout_fwd(*head, *tail, st, flags)
        return L.dstd_model_rollout_tf_fwd(*head, *tail, *tf, st, flags)

    if short == "saved fwd":
        snap = b.freeze()
        refused(fwd(ns - 1), short)
    native.check(fwd(ns), "the forward")
    torch.cuda.synchronize()
    saved0, stats0 = saved.tensor.clone(), _clones(stats)
    ws = b.new("workspace", nw, fill)
    dobs = b.f32("dobs", obs.shape, NAN_OUT)
    params = list(m.parameters())
    arena = native.GradArena(params, obs.device, buf=b.f32("gradient arena", (native.arena_numel(params),), 0))
    gref = native.ext.model_grads_ref(m._native_grads(arena))

    def bwd(a, c, k=None):
        head = (pref, B, Tin, H)
        tail = (0.0, None, saved.ptr, a, dout.data_ptr(), gref, dobs.data_ptr(), ws.ptr, c)
        if not unstrided:
            if k is None:
                return L.dstd_model_rollout_strided_bwd(*head, S, *tail, *tf, st, flags)
            return L.dstd_model_rollout_strided_bwd_window(*head, S, k, *tail, *tf, st, flags)
        assert k is None
        if mask is None:
            return L.dstd_model_rollout_bwd(*head, *tail, st, flags)
        return L.dstd_model_rollout_tf_bwd(*head, *tail, *tf, st, flags)

    if short in ("saved bwd", "workspace"):
        snap = b.freeze()
        refused(bwd(ns - 1, nw) if short == "saved bwd" else bwd(ns, nw - 1), short)
        snap = b.freeze()
        refused(bwd(ns - 1, nw, K - 1) if short == "saved bwd" else bwd(ns, nw - 1, K - 1), short + ", one window")
    if stepwise:
        for k in range(K - 1, -1, -1):
            native.check(bwd(ns, nw, k), "dstd_model_rollout_strided_bwd_window")
    else:
        native.check(bwd(ns, nw), "the backward")
    b.check()  # (synchronises) no write outside out, saved, dobs, the workspace or the arena
    assert torch.equal(saved.tensor, saved0), "the backward wrote to saved"
    if mask is not None:
        assert torch.equal(g_mask.tensor, mask.reshape(-1)), "mask was written"
        assert torch.equal(d_truth.view(torch.int32), truth.view(torch.int32)), "truth was written"
    _unchanged(stats, stats0, "running statistics across the backward")
    res = {"out": out, "dobs": dobs}
    res.update({f"stat{i}": s for i, s in enumerate(stats)})
    res.update({"grad " + n: g for (n, _), g in zip(m.named_parameters(), arena.views()) if g is not None})
    return _keep(res)


def _contract_case(case, flags, seed, masked=True, stride=None):
    m, Tin, V, S, H = case_model(case)
    S = S if stride is None else stride
    m.train(not flags & native.TRAIN_RUNNING_STATS)
    B = 4
    pair = bool(flags & native.TRAIN_PAIRED)
    Bt = B // 2 if pair else B
    obs, dout = observations(B, Tin, V, seed), observations(B, H, V, seed + 1)
    truth = observations(Bt, Tin + H, V, seed + 2) if masked else None
    maps = [(0, 1), (Tin + H - 1, -1)] if pair else [(0, 1), (0, 0)]
    mask = mask_of("mixed", windows(H, S), B, pair) if masked else None
    return m, obs, dout, H, S, truth, maps, mask


@pytest.mark.parametrize("case,flags,masked", [(CASES[0], 0, True), (CASES[1], native.TRAIN_PAIRED, True),
                                               (CASES[2], native.TRAIN_RUNNING_STATS, False),
                                               (CASES[3], native.TRAIN_ONE_STREAM, True)],
                         ids=["S1-masked", "S2-paired-masked", "S1-running-free", "S2-one-stream-masked"])
def test_strided_memory_contract(case, flags, masked):
    """Exact-size saved / out / dobs / workspace / arena / truth / mask between
    sentinel guards: nothing is written outside them, the results do not depend
    on what saved and the workspace held before (0x00, 0xFF, 0x4B) -- Gh is
    zeroed by the call --, two runs give equal bits, the backward leaves saved,
    the mask, the truth and the running statistics alone, the inputs are not
    written; one window per call gives the same bits."""
    m, obs, dout, H, S, truth, maps, mask = _contract_case(case, flags, 101, masked)
    inputs = [obs, dout] + ([truth, mask] if masked else []) + list(m.parameters()) + list(m.buffers())
    before = _clones(inputs)
    what = f"strided {case} flags {flags}"
    got = run_fills(lambda fill: strided_call(m, obs, dout, H, S, flags, truth, maps, mask, fill), what)
    _unchanged(inputs, before, what)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (what, k)
    _same(got, strided_call(m, obs, dout, H, S, flags, truth, maps, mask, 0xFF, stepwise=True), what + ": stepwise")
    assert float(got["dobs"].abs().max()) > 0


def test_strided_size_checks():
    """Each size one byte short is DSTD_EWORKSPACE with nothing written and
    nothing left pending -- saved in the forward; saved and the workspace in the
    backward and in the one-window backward -- and the valid call on the same
    buffers then gives the reference result."""
    m, obs, dout, H, S, truth, maps, mask = _contract_case(CASES[1], native.TRAIN_PAIRED, 111)
    base = strided_call(m, obs, dout, H, S, native.TRAIN_PAIRED, truth, maps, mask, 0x4B)
    for short in ("saved fwd", "saved bwd", "workspace"):
        _same(base, strided_call(m, obs, dout, H, S, native.TRAIN_PAIRED, truth, maps, mask, 0x4B, short=short), short)


@pytest.mark.parametrize("masked", [False, True], ids=["free", "mixed-mask"])
@pytest.mark.parametrize("Tin,Tout", [(3, 3), (4, 2), (5, 1), (1, 5)])
def test_a_stride_of_a_whole_window_is_the_unstrided_chain(Tin, Tout, masked):
    """Direct C calls at S = Tout against dstd_model_rollout_fwd / _bwd (with a
    mixed mask: _tf_fwd / _tf_bwd), three windows with the last one cut, for
    Tin <= Tout and Tin > Tout: out, the running statistics, dobs and every
    parameter gradient, bit for bit."""
    m = small_model(Tin, Tout).train()
    H, B = 3 * Tout - 1 if Tout > 1 else 3, 4
    obs, dout = observations(B, Tin, 5, 121), observations(B, H, 5, 122)
    truth = observations(B, Tin + H, 5, 123) if masked else None
    mask = mask_of("mixed", 3, B, False) if masked else None
    maps = [(0, 1), (0, 0)]
    got = strided_call(m, obs, dout, H, Tout, 0, truth, maps, mask, 0x4B)
    want = strided_call(m, obs, dout, H, Tout, 0, truth, maps, mask, 0x4B, unstrided=True)
    assert set(got) == set(want)
    for name in got:  # torch.equal: Gh starts at +0 where the unstrided chain has no term, so a -0 may come out +0
        _equal(got[name], want[name], f"S = Tout = {Tout}, Tin = {Tin}, masked = {masked}: {name}")
    assert float(got["dobs"].abs().max()) > 0


# ---- 5. the engine ------------------------------------------------------------------
def _engine_setup(seed):
    from test_gpu_rollout import _engine_setup as setup
    return setup(9, seed)  # Tin = 3, Tout = 3, windows of 3 + 6 frames


def test_engine_strided_teacher_step_is_the_hand_composed_step():
    """One train(horizon=6, stride=2, teacher_ratio=0.5) step (three windows, the
    inverse pass) under torch.manual_seed against the step composed by hand on a
    twin from the same draw -- the window loop of the helper, weighted_losses, the
    hand-written backward, Adam: losses and every parameter and buffer, bit for bit."""
    from engine.loss import prepare_joint_weights, weighted_losses
    eng, hand, loader, weights = _engine_setup(51)
    steps, step = [], eng._step_rollout
    eng._step_rollout = lambda *a: steps.append(step(*a)) or steps[-1]
    torch.manual_seed(1234)
    total = eng.train(loader, 0, weights=weights, horizon=6, stride=2, teacher_ratio=0.5)
    assert len(steps) == 1 and np.isfinite(total)

    inputs, inputs_inv, targets, _ = next(iter(loader))
    net = hand.model.model
    torch.manual_seed(1234)
    mask = torch.rand(3, 4, device=DEV) < 0.5
    assert 0 < int(mask[1:].sum()) < mask[1:].numel()
    net._dstd_inplace_grads = True
    try:
        x, xi = hand.transform(inputs.float()), hand.transform(inputs_inv.float())
        loop = model_loop_pair(net, x[:, :3].contiguous(), xi[:, :3].contiguous(), 6, 2,
                               hand.transform(targets.float()), mask)
        o = loop.out.clone().requires_grad_()
        out = weighted_losses(hand.model.loss_spec, [hand.inverse(o[:2]), hand.inverse(o[2:])], targets.float(),
                              [(3, 1), (5, -1)], prepare_joint_weights(weights, DEV))
        hand.optimizer.zero_grad()
        (out.sum() / 2).backward()
        loop.backward(o.grad, list(net.parameters()))
        hand.optimizer.step()
    finally:
        net._dstd_inplace_grads = False
    got = torch.stack([v.reshape(()) for v in steps[0]])
    assert got.shape == (2,) and bool((got > 0).all())
    assert torch.equal(got, out[0].detach()), (got, out[0])
    _state_equal(eng.model.model, net, "engine step, stride 2, teacher_ratio 0.5")
    assert not getattr(eng.model.model, "_dstd_inplace_grads", False)


def test_engine_without_a_stride_is_unchanged():
    """train(horizon=6) and train(horizon=6, stride=3) (a whole window) are one
    step, the free-running strided step is another, and a stride needs a horizon."""
    eng, twin, loader, weights = _engine_setup(52)
    a = eng.train(loader, 0, weights=weights, horizon=6)
    b = twin.train(loader, 0, weights=weights, horizon=6, stride=3)
    assert a == b
    _state_equal(eng.model.model, twin.model.model, "stride = output_time_frame")
    other, _, _, _ = _engine_setup(52)
    other.train(loader, 0, weights=weights, horizon=6, stride=1)
    assert any(not torch.equal(p, q) for p, q in zip(other.model.model.parameters(), twin.model.model.parameters()))
    with pytest.raises(ValueError, match="stride.*horizon"):
        eng.train(loader, 0, weights=weights, stride=2)
