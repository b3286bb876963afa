"""MI355X parity of the generic kernels at the edges of the supported shape
envelope (B >= 1, 2 <= T <= 128, 1 <= V <= 32, 1 <= cin, cout <= 64,
1 <= red_channels <= 8): every case of tests/envelope_cases.py against the
fp64 oracle, at the project's bars

  single DSTDGC op, eval forward and train forward + backward : 1e-4
  DSTDGCB eval forward                                       : 1e-4
  DSTDGCB train-mode forward + backward                      : 2e-4
  whole model                                                : conftest.model_tol

(tests/test_gpu_parity.py, tests/test_gpu_train.py headers).  The cases sit
on the dispatch boundaries of the generic kernels -- fragment counts, pad /
no-pad sizes, the slab / strided-GEMM cliff at T = 64 / 65, adjacency row
tiles, channel tails, the streaming GEMM's K and N limits -- which
tests/test_envelope_host.py pins by arithmetic; it also shows that the fp32
oracle itself holds half of each bar on every case.  Shapes past the envelope
are refused without a write and without leaving an error behind.
"""
import pytest
import torch

import dstd_native as native
import envelope_cases as E
from conftest import model_tol, rel_err
from model import DSTDGC, DSTDGCB, get_model
from oracle import dstdgcn_oracle as O
from test_gpu_parity import synth
from test_gpu_train import _bn_of, _realias, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _worst(errs):
    k = max(errs, key=errs.get)
    return k, errs[k]


# ---- single ops ------------------------------------------------------------
@pytest.mark.parametrize("c", E.OP_CASES, ids=E.case_id)
def test_op_eval_forward(c):
    op, x, A, alpha, _ = E.build_op(c)
    y64 = E.op_reference64(c)["y"]
    op = op.to(DEV).eval()
    with torch.no_grad():
        y = op(x.to(DEV), A.to(DEV), alpha.to(DEV))
    torch.cuda.synchronize()
    err = rel(y, y64)
    print(f"{E.case_id(c)} [{E.WHY[c]}]: eval forward {err:.2e}")
    assert err <= E.OP_BAR


def _op_native(c):
    """y, dx, dA, dalpha and the parameter gradients of an op case through the
    module (native train forward + backward)."""
    op, x, A, alpha, w = E.build_op(c)
    op = op.to(DEV)
    xg, Ag, ag = (t.to(DEV).requires_grad_(True) for t in (x, A, alpha))
    y = op(xg, Ag, ag)
    assert y.grad_fn is not None
    (y * w.to(DEV)).sum().backward()
    got = {"y": y, "dx": xg.grad, "dA": Ag.grad, "dalpha": ag.grad}
    got.update({name: p.grad for name, p in op.named_parameters()})
    return got


# agg_bwd's two-launch path (dF on k_aggc, dD on k_agg), which held the channel-tail bug: the
# library reports which kernel its last aggregation backward dispatched (0: two launches)
TWO_LAUNCH = (E.OpCase("temporal", 3, 3, 35, 32, 2, 2), E.OpCase("temporal", 13, 17, 49, 16, 2, 2))
CHUNK_JF4 = E.OpCase("temporal", 20, 24, 64, 5, 2, 2)  # ... and here the 16-channel chunk kernel at JF = 4
assert all(c in E.OP_CASES for c in TWO_LAUNCH + (CHUNK_JF4,))


@pytest.mark.parametrize("c", E.OP_CASES, ids=E.case_id)
def test_op_train_forward_backward(c):
    errs = E.op_errors(_op_native(c), E.op_reference64(c))
    if c in TWO_LAUNCH:  # the backward that ran was the two-launch one, not the channel-chunk kernel
        torch.cuda.synchronize()
        assert E.temporal_bwd_two_launch(c) and native.lib().dstd_debug_aggb_last() == 0
    if c == CHUNK_JF4:
        torch.cuda.synchronize()
        assert not E.temporal_bwd_two_launch(c) and native.lib().dstd_debug_aggb_last() == 16
    name, err = _worst(errs)
    print(f"{E.case_id(c)} [{E.WHY[c]}]: worst {err:.2e} ({name}), y {errs['y']:.2e}, dx {errs['dx']:.2e}")
    for k, v in errs.items():
        assert v < E.OP_BAR, (k, v)


def _raw_op_backward(op, c, x, A, alpha, w, sinks, times):
    """dstd_dstdgc_train_fwd_r + _bwd_r ``times`` times into the same
    gradient buffers ``sinks`` = (arena, dx, dA, dalpha)."""
    L = native.lib()
    mode = native.MODE_SPATIAL if c.mode == "spatial" else native.MODE_TEMPORAL
    arena, dx, dA, dalpha = sinks
    dims = (c.B, c.cin, c.cout, c.T, c.V, c.red)
    y = torch.empty(c.B, c.cout, c.T, c.V, device=DEV)
    nbytes = L.dstd_dstdgc_train_saved_bytes_r(mode, *dims)
    saved = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ws = native.workspace(torch.device(DEV), L.dstd_dstdgc_train_workspace_bytes_r(mode, *dims))
    st = native.stream_handle(torch.device(DEV))
    for _ in range(times):
        native.check(L.dstd_dstdgc_train_fwd_r(mode, x.data_ptr(), *dims, native.gc_weights(op), A.data_ptr(),
                                               alpha.data_ptr(), y.data_ptr(), saved.data_ptr(), nbytes, st),
                     "dstd_dstdgc_train_fwd_r")
        native.check(L.dstd_dstdgc_train_bwd_r(mode, x.data_ptr(), *dims, native.gc_weights(op), alpha.data_ptr(),
                                               saved.data_ptr(), nbytes, w.data_ptr(), dx.data_ptr(),
                                               native.gc_grads(op, arena), dA.data_ptr(), dalpha.data_ptr(),
                                               ws.data_ptr(), ws.numel(), st), "dstd_dstdgc_train_bwd_r")
    torch.cuda.synchronize()


ACCUMULATE = [E.OpCase("spatial", 24, 40, 20, 16, 2, 3),  # slab kernels, no pad
              E.OpCase("temporal", 20, 24, 65, 5, 2, 2),  # strided-GEMM fallback
              E.OpCase("temporal", 13, 17, 49, 16, 2, 2),  # two-launch backward, channel tail
              E.OpCase("temporal", 20, 64, 35, 22, 8, 2),  # K = kCsMax
              E.OpCase("spatial", 6, 5, 3, 2, 2, 3)]  # below the streaming width


@pytest.mark.parametrize("c", ACCUMULATE, ids=E.case_id)
def test_op_backward_accumulates(c):
    """The backward entry point promises (+=) on dx, dA, dalpha and every
    parameter gradient: two runs into the same buffers give twice one run."""
    assert c in E.OP_CASES
    op, x, A, alpha, w = E.build_op(c)
    op = op.to(DEV)
    x, A, alpha, w = (t.to(DEV).contiguous() for t in (x, A.reshape(A.shape[-2], A.shape[-1]), alpha, w))

    def sinks():
        return (native.GradArena(list(op.parameters()), torch.device(DEV)), torch.zeros_like(x), torch.zeros_like(A),
                torch.zeros_like(alpha))

    one, two = sinks(), sinks()
    _raw_op_backward(op, c, x, A, alpha, w, one, 1)
    _raw_op_backward(op, c, x, A, alpha, w, two, 2)
    names = ["dx", "dA", "dalpha"] + [n for n, _ in op.named_parameters()]
    singles = list(one[1:]) + one[0].views()
    doubles = list(two[1:]) + two[0].views()
    ref = E.op_reference64(c)
    for name, g1, g2 in zip(names, singles, doubles):
        assert rel(g1, ref[name]) < E.OP_BAR, name  # the single run is the gradient
        assert rel(g2, 2 * g1) <= 1e-6, (name, rel(g2, 2 * g1))


# ---- blocks ------------------------------------------------------------------
@pytest.mark.parametrize("c", E.BLOCK_EVAL_CASES, ids=E.case_id)
def test_block_eval_forward(c):
    blk, x = E.build_block_eval(c)
    y64 = E.block_eval_reference(c, built=(blk, x))
    blk = blk.to(DEV).eval()
    with torch.no_grad():
        y = blk(x.to(DEV))
    err = rel(y, y64)
    print(f"{E.case_id(c)}: block eval forward {err:.2e}")
    assert err <= E.BLOCK_EVAL_BAR


def _assert_bn_last(c, when):
    """The last BatchNorm launch took the apply path the case is there for
    (another value: probably an unaligned tensor -- report it, keep the shape)."""
    torch.cuda.synchronize()
    got, want = native.lib().dstd_debug_bn_last(), E.BN_APPLY_EXPECT[c]
    assert got == E.bn_code(*want), (when, "path, ns, splits", (got & 15, got >> 4 & 15, got >> 8), "expected", want)


@pytest.mark.parametrize("c", E.BLOCK_TRAIN_CASES + E.BN_APPLY_CASES, ids=E.case_id)
def test_block_train_forward_backward(c):
    blk, x, w = E.build_block_train(c)
    assert blk.A_s.data_ptr() == blk.R_s.data_ptr()
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    ref = E.block_train_reference(c, built=(blk, x, w))
    blk = blk.to(DEV).train()
    _realias(blk)
    xg = x.to(DEV).requires_grad_(True)
    y = blk(xg)
    if c in E.BN_APPLY_EXPECT:
        _assert_bn_last(c, "forward")
    (y * w.to(DEV)).sum().backward()
    if c in E.BN_APPLY_EXPECT:
        _assert_bn_last(c, "backward")
    grads = {}
    for name, p in blk.named_parameters():
        if name in ("A_s", "A_t"):
            assert p.grad is None
            continue
        grads[name] = p.grad
    errs = E.block_train_errors({"y": y, "dx": xg.grad, "grads": grads}, ref)
    name, err = _worst(errs)
    print(f"{E.case_id(c)}: worst {err:.2e} ({name}), y {errs['y']:.2e}, dx {errs['dx']:.2e}")
    assert errs["y"] < E.BLOCK_TRAIN_BAR and errs["dx"] < E.BLOCK_TRAIN_BAR
    for k, v in errs.items():
        assert v <= E.BLOCK_TRAIN_BAR, (k, v)
    # running statistics: (1 - m) * old + m * batch (unbiased variance)
    bns = [m for m in blk.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    assert len(bns) == len(ref["stats"])
    for bn, (mean, var) in zip(bns, ref["stats"]):
        old_m = sd[[k for k in sd if k.endswith("running_mean") and bn is _bn_of(blk, k)][0]]
        old_v = sd[[k for k in sd if k.endswith("running_var") and bn is _bn_of(blk, k)][0]]
        assert rel(bn.running_mean, 0.9 * old_m.double() + 0.1 * mean) < 1e-5
        assert rel(bn.running_var, 0.9 * old_v.double() + 0.1 * var) < 1e-5
        assert int(bn.num_batches_tracked) == 1


# ---- whole model at small T ----------------------------------------------------
@pytest.mark.parametrize("t_in,t_out", [(8, 8), (32, 32)])
def test_model_eval_forward_small_T(t_in, t_out):
    """H36M with 8 in / 8 out (T=16: one fragment, no pad) and 32 in / 32 out
    frames (T=64: the last slab shape): the recipe of test_dstdgcn_generic_T30."""
    torch.manual_seed(3 + t_in)
    opts = dict(input_channels=6, input_time_frame=t_in, output_time_frame=t_out, st_gcnn_dropout=0.1,
                joints_to_consider=22, num_feature=64, num_layers=1, layout="h36m")
    m = get_model("dstdgcn", dstdgcn=opts)
    with torch.no_grad():  # dynamic terms on, BN at non-trivial but tame stats
        for name, p in m.named_parameters():
            if name.endswith(("alpha_sm", "alpha_tm")):
                p.fill_(0.5)
            if name.endswith(("W_s", "R_t")):
                p.copy_(0.1 * torch.randn(p.shape))
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_var.fill_(4.0)
    x = synth(1, t_in + t_out, 22, t_in, 11)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    y64 = O.dstdgcn(x, sd, 1).numpy()
    ref32 = rel_err(O.dstdgcn(x, sd, 1, dtype=torch.float32).numpy(), y64)
    m = m.to(DEV).eval()
    with torch.no_grad():
        y = m(x.to(DEV)).cpu().numpy()
    err = rel_err(y, y64)
    print(f"model T={t_in + t_out}: {err:.2e} (fp32 oracle {ref32:.2e}, bar {model_tol(ref32):.1e})")
    assert err <= model_tol(ref32), ref32


# ---- past the envelope ---------------------------------------------------------
SENTINEL = -7.25
EINVAL, ELIMIT = -1, -3  # include/dstd_gcn.h DSTD_EINVAL, DSTD_ELIMIT
MESSAGE = {EINVAL: "invalid argument", ELIMIT: "envelope"}  # dstd_error_string, as the module raises it
# (what, T, V, cin, cout, red, code) around the valid (T, V, cin, cout, red) = (20, 17, 8, 12, 2);
# T = 1 is a bad shape (DSTD_EINVAL), everything else is past a limit
OUTSIDE = [("V=33", 20, 33, 8, 12, 2, ELIMIT), ("T=129", 129, 17, 8, 12, 2, ELIMIT), ("T=1", 1, 17, 8, 12, 2, EINVAL),
           ("cin=65", 20, 17, 65, 12, 2, ELIMIT), ("cout=65", 20, 17, 8, 65, 2, ELIMIT),
           ("red=9", 20, 17, 8, 12, 9, ELIMIT)]
# blocks: (what, T, V, cin, cout, code of the eval entry point, of the training one -- whose block_ok
# counts a block's channel counts among its arguments: DSTD_EINVAL)
OUTSIDE_BLOCK = [("V=33", 16, 33, 6, 64, ELIMIT, ELIMIT), ("T=129", 129, 25, 6, 64, ELIMIT, ELIMIT),
                 ("T=1", 1, 25, 6, 64, EINVAL, EINVAL), ("cin=65", 16, 25, 65, 64, ELIMIT, EINVAL),
                 ("cout=65", 16, 25, 6, 65, ELIMIT, EINVAL)]
VALID_OP = {"spatial": E.OpCase("spatial", 8, 12, 20, 17, 2, 2), "temporal": E.OpCase("temporal", 8, 12, 20, 17, 2, 2)}


def _filled(*shape, dtype=torch.float32):
    if dtype == torch.uint8:
        return torch.full(shape, 0xA5, dtype=dtype, device=DEV)
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def _untouched(t):
    return bool((t == (0xA5 if t.dtype == torch.uint8 else SENTINEL)).all())


@pytest.mark.parametrize("mode", ["spatial", "temporal"])
def test_outside_envelope_is_refused_op(mode):
    """Op eval and op train: every shape one step past the envelope is
    refused by the C ABI before anything is written (sentinel-filled outputs
    stay as they were) and by the module (RuntimeError; red = 9 at
    construction, NotImplementedError); after each refusal the valid call on
    the same weights meets its bar, so no error was left pending.  Each
    refusal is pinned to its code (and the module's message to that code)."""
    L = native.lib()
    dev = torch.device(DEV)
    c = VALID_OP[mode]
    op, x, A, alpha, w = E.build_op(c)
    ref = E.op_reference(c, built=(op, x, A, alpha, w))
    op = op.to(DEV).eval()
    xv, Av, av = x.to(DEV), A.to(DEV), alpha.to(DEV)
    md = native.MODE_SPATIAL if mode == "spatial" else native.MODE_TEMPORAL
    st = native.stream_handle(dev)
    B = c.B
    for what, T, V, cin, cout, red, want in OUTSIDE:
        NN = V if mode == "spatial" else T
        xb = torch.zeros(B, cin, T, V, device=DEV)
        Ab = torch.zeros(NN, NN, device=DEV)
        y = _filled(B, cout, T, V)
        if red == 2:  # the eval entry point carries red = 2
            ws = native.workspace(dev, L.dstd_dstdgc_workspace_bytes(md, B, cin, cout, T, V))
            code = L.dstd_dstdgc_fwd(md, xb.data_ptr(), B, cin, cout, T, V, native.gc_weights(op), Ab.data_ptr(),
                                     av.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), st)
            torch.cuda.synchronize()
            assert code == want, (what, code)
            assert _untouched(y), what
        nbytes = max(int(L.dstd_dstdgc_train_saved_bytes_r(md, B, cin, cout, T, V, red)), 256)
        saved = _filled(nbytes, dtype=torch.uint8)
        code = L.dstd_dstdgc_train_fwd_r(md, xb.data_ptr(), B, cin, cout, T, V, red, native.gc_weights(op),
                                         Ab.data_ptr(), av.data_ptr(), y.data_ptr(), saved.data_ptr(), nbytes, st)
        torch.cuda.synchronize()
        assert code == want, (what, code)
        assert _untouched(y) and _untouched(saved), what
        dx, dA, dal = _filled(B, cin, T, V), _filled(NN, NN), _filled(1)
        arena = native.GradArena(list(op.parameters()), dev)
        arena.buf.fill_(SENTINEL)
        ws = native.workspace(dev, max(int(L.dstd_dstdgc_train_workspace_bytes_r(md, B, cin, cout, T, V, red)), 256))
        code = L.dstd_dstdgc_train_bwd_r(md, xb.data_ptr(), B, cin, cout, T, V, red, native.gc_weights(op),
                                         av.data_ptr(), saved.data_ptr(), nbytes, y.data_ptr(), dx.data_ptr(),
                                         native.gc_grads(op, arena), dA.data_ptr(), dal.data_ptr(), ws.data_ptr(),
                                         ws.numel(), st)
        torch.cuda.synchronize()
        assert code == want, (what, code)
        assert all(_untouched(t) for t in (dx, dA, dal, arena.buf, saved)), what
        # the module: built at the offending size, under no_grad and under autograd
        if red != 2:
            with pytest.raises(NotImplementedError):
                DSTDGC(cin, cout, T, V, red_channels=red, mode=mode)
        else:
            ref_c, kpt = (T, V) if mode == "spatial" else (V, T)
            bad = DSTDGC(cin, cout, ref_c, kpt, mode=mode).to(DEV)
            with pytest.raises(RuntimeError, match=MESSAGE[want]), torch.no_grad():
                bad(xb, Ab, av)
            with pytest.raises(RuntimeError, match=MESSAGE[want]):
                bad(xb.clone().requires_grad_(True), Ab, av)
        # a valid call straight after: eval forward, then forward + backward
        with torch.no_grad():
            assert rel(op(xv, Av, av), ref["y"]) <= E.OP_BAR, what
        xg = xv.clone().requires_grad_(True)
        (op(xg, Av, av) * w.to(DEV)).sum().backward()
        assert rel(xg.grad, ref["dx"]) < E.OP_BAR, what
        op.zero_grad(set_to_none=True)


def test_outside_envelope_is_refused_block():
    """DSTDGCB eval and train forward at V=33, T=129, T=1, cin=65, cout=65
    (a block carries red = 2): refused without a write to the output, the
    saved state or the running statistics, each with its own code; the valid
    call afterwards meets its bar in both modes."""
    L = native.lib()
    dev = torch.device(DEV)
    c = E.BlockCase(6, 64, "cmu", 16, 25, 2)
    assert c in E.BLOCK_EVAL_CASES
    blk, x = E.build_block_eval(c)
    y64 = E.block_eval_reference(c, built=(blk, x))
    blk = blk.to(DEV).eval()
    _realias(blk)
    xv = x.to(DEV)
    st = native.stream_handle(dev)
    buffers0 = [b.clone() for b in blk.buffers()]
    B = c.B
    for what, T, V, cin, cout, want_eval, want_train in OUTSIDE_BLOCK:
        p = native.block_struct(blk)
        p.cin, p.cout = cin, cout
        xb = torch.zeros(B, cin, T, V, device=DEV)
        y = _filled(B, cout, T, V)
        ws = native.workspace(dev, max(int(L.dstd_block_workspace_bytes(B, cin, cout, T, V)), 256))
        code = L.dstd_block_fwd_ex(p, xb.data_ptr(), B, T, V, y.data_ptr(), ws.data_ptr(), ws.numel(), st, 0)
        torch.cuda.synchronize()
        assert code == want_eval, (what, code)
        assert _untouched(y), what
        nbytes = max(int(L.dstd_block_train_saved_bytes(B, cin, cout, T, V)), 256)
        saved = _filled(nbytes, dtype=torch.uint8)
        code = L.dstd_block_train_fwd_ex(p, xb.data_ptr(), B, T, V, 0.1, y.data_ptr(), saved.data_ptr(), nbytes, st, 0)
        torch.cuda.synchronize()
        assert code == want_train, (what, code)
        assert _untouched(y) and _untouched(saved), what
        assert all(torch.equal(a, b) for a, b in zip(blk.buffers(), buffers0)), what
        # the module, built at the offending size (T = 1 has no temporal prior to build: the valid
        # block is fed the one-frame activation; DSTDGCB.forward checks no shape itself, the
        # message is the C ABI's)
        bad = blk if T == 1 else DSTDGCB(cin, cout, T, V, "cmu").to(DEV).eval()
        stats0 = [b.clone() for b in bad.buffers()]
        with pytest.raises(RuntimeError, match=MESSAGE[want_eval]), torch.no_grad():
            bad(xb)
        bad.train()
        with pytest.raises(RuntimeError, match=MESSAGE[want_train]):
            bad(xb)
        bad.eval()
        assert all(torch.equal(a, b) for a, b in zip(bad.buffers(), stats0)), what
        with torch.no_grad():
            assert rel(blk(xv), y64) <= E.BLOCK_EVAL_BAR, what
    # ... and the train-mode call on the same block
    ct = E.BlockCase(6, 64, "cmu", 16, 25, 4)
    tb, xt, wt = E.build_block_train(ct)
    ref = E.block_train_reference(ct, built=(tb, xt, wt))
    tb = tb.to(DEV).train()
    _realias(tb)
    with pytest.raises(RuntimeError, match=MESSAGE[ELIMIT]):
        tb(torch.zeros(4, 6, 129, 25, device=DEV))
    xg = xt.to(DEV).requires_grad_(True)
    y = tb(xg)
    (y * wt.to(DEV)).sum().backward()
    assert rel(y, ref["y"]) < E.BLOCK_TRAIN_BAR and rel(xg.grad, ref["dx"]) < E.BLOCK_TRAIN_BAR
    assert all(int(m.num_batches_tracked) == 1 for m in tb.modules() if isinstance(m, torch.nn.BatchNorm1d))
