"""MI355X: every entry point on exact-size, guard-banded, poisoned buffers
(tests/guard_helper.py).

The C ABI promises that scratch comes from a caller-owned workspace of
``*_workspace_bytes`` bytes, that the library allocates nothing and keeps no
state, that a train forward's ``saved`` buffer is all its backward needs and
that a refused call writes nothing.  Three kinds of test hold it to that:

  a. scratch independence -- a call on a workspace (and, for a train forward,
     a ``saved`` buffer) of exactly the size asked for, filled with 0x00, 0xFF
     (NaN) and 0x4B (large and finite: it survives a max where a NaN is
     dropped), gives bit-identical outputs; two runs on the same fill do too
     (the control, run first); the zero-fill outputs meet the existing bars
     against the fp64 oracle (envelope_cases, taps_helper, loss_helper,
     conftest.model_tol, unchanged).  Outputs the call defines (=) start as
     NaN, so an element it does not write fails the bar; outputs it
     accumulates into (+=) start as zero.
  b. bounds -- every buffer the call may write sits between two 1 MiB guard
     bands that must come back intact, and every input, and ``saved`` across
     the backward, is bit-unchanged.  Ops, blocks, models, taps, the aux
     layers and the losses are driven through the ABI so that outputs, BN
     running statistics and the gradient arena are guarded too; the Python
     layer (the DSTDGC and DSTDGCB modules, model(x), forward_taps, an
     eval-mode backward, one engine step, the plain ST-GCNN layer) runs under
     guarded_workspaces.
  c. size checks -- size - 1 of every workspace_bytes / saved_bytes argument
     is refused with DSTD_EWORKSPACE (dstd_losses_fwd: DSTD_EINVAL,
     tests/test_loss_host.py) without a write to the workspace interior,
     ``saved``, an output or a running statistic; the valid call afterwards
     meets its bar.  guard_helper.PINNED_SIZES is the host-side comparison of
     the sizes themselves.

Model-level training gradients have no per-tensor bar for synthetic models
(tests/test_gpu_train.py judges the fixture step against measured fp32 noise);
here the train-mode y and running statistics are anchored to the oracle and the
gradients by bit identity across fills, the gradient bars staying with the ops
and blocks the model is made of.  No graph capture: a capture's workspace lives
in the graph's pool (tests/test_gpu_parity.py covers it).
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import dstd_native as native
import envelope_cases as E
import guard_helper as G
import taps_helper as H
from conftest import group, load_npz, model_tol, rel_err
from loss_helper import TERMS, loss_terms
from model import DSTDGCB, get_model
from oracle import dstdgcn_oracle as O
from test_gpu_train import PLAIN, _realias, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, EWORKSPACE = -1, -2  # include/dstd_gcn.h
NAN_OUT = 0xFF  # a (=) output before the call
FUSED = native.FWD_FUSED_TEMPORAL
BLOCK_FLAGS = (0, FUSED, FUSED | native.FWD_SEPARATE_ENCODERS, native.FWD_SEPARATE_BLOCK | FUSED, native.FWD_EXACT_FP32)
MODEL_FLAGS = BLOCK_FLAGS[:4] + (native.FWD_SEPARATE_ADJ, native.FWD_EXACT_FP32)  # (dstd_block_fwd_ex refuses SEPARATE_ADJ)


def _dev():
    return torch.device(DEV)


def _stream():
    return native.stream_handle(_dev())


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class Bufs:
    """The guarded buffers of one call, by name."""

    def __init__(self):
        self.all = {}

    def new(self, name, nbytes, fill):
        assert name not in self.all, name
        g = self.all[name] = G.Guarded(nbytes, fill, DEV)
        return g

    def f32(self, name, shape, fill, like=None):
        t = self.new(name, 4 * _numel(shape), fill).view(torch.float32, tuple(shape))
        if like is not None:
            t.copy_(like)
        return t

    def check(self):
        torch.cuda.synchronize()
        for name, g in self.all.items():
            g.check(name)

    def freeze(self):
        torch.cuda.synchronize()
        return {name: g.tensor.clone() for name, g in self.all.items()}

    def check_frozen(self, snap, what):
        """After a refused call: guards intact and every interior as it was."""
        self.check()
        for name, g in self.all.items():
            assert torch.equal(g.tensor, snap[name]), f"{what}: the refused call wrote to {name}"


def _clones(tensors):
    return [t.detach().clone() for t in tensors]


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _unchanged(tensors, clones, what):
    for i, (t, c) in enumerate(zip(tensors, clones)):
        assert torch.equal(_bits(t), _bits(c)), f"{what}: input {i} was written"


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if not torch.equal(_bits(a[k]), _bits(b[k])):
            d = (a[k].double() - b[k].double()).abs()
            n = int((_bits(a[k]) != _bits(b[k])).sum())
            raise AssertionError(f"{what}: {k} differs in {n} of {a[k].numel()} elements, max |d| "
                                 f"{float(d.nan_to_num(nan=float('inf')).max()):.3e}")


def run_fills(call, what):
    """``call(fill)`` -> {name: output}.  The control first (two zero-fill runs
    bit-identical: fixed-order reductions, no float atomics), then every
    other fill against the zero-fill run.  Returns the zero-fill outputs."""
    base = call(G.FILLS[0])
    _same(base, call(G.FILLS[0]), f"{what}: control, two runs on the 0x00 fill")
    for fill in G.FILLS[1:]:
        _same(base, call(fill), f"{what}: fill 0x{fill:02X} against 0x00")
    return base


def _keep(out):
    return {k: v.detach().clone() for k, v in out.items()}


def _worst(errs):
    k = max(errs, key=errs.get)
    return k, errs[k]


# =====================================================================================
# single ops: every OP_CASES entry, and red = 1 next to the cases' 2, 3 and 8
# =====================================================================================
RED1 = [E.OpCase("spatial", 20, 64, 35, 22, 1, 2), E.OpCase("temporal", 20, 64, 35, 22, 1, 2)]
OPS = E.OP_CASES + RED1
assert {c.red for c in OPS} >= {1, 2, 8}


@functools.lru_cache(maxsize=None)
def _op_ref(c):
    return E.op_reference64(c) if c in E.OP_CASES else E.op_reference(c)


def _mode(c):
    return native.MODE_SPATIAL if c.mode == "spatial" else native.MODE_TEMPORAL


def _op_on_device(c):
    op, x, A, alpha, w = E.build_op(c)
    op = op.to(DEV)
    x, A, alpha, w = (t.to(DEV).contiguous() for t in (x, A.reshape(A.shape[-2], A.shape[-1]), alpha, w))
    return op, x, A, alpha, w


def op_call(c, op, x, A, alpha, w, fill):
    """The eval forward (red = 2), the train forward and the backward of an op
    case through the C ABI, everything written sitting in a Guarded."""
    L, md, st = native.lib(), _mode(c), _stream()
    dims = (c.B, c.cin, c.cout, c.T, c.V)
    b, out = Bufs(), {}
    gw = native.gc_weights(op)
    if c.red == 2:
        n = L.dstd_dstdgc_workspace_bytes(md, *dims)
        ws = b.new("eval workspace", n, fill)
        y = b.f32("eval y", (c.B, c.cout, c.T, c.V), NAN_OUT)
        native.check(L.dstd_dstdgc_fwd(md, x.data_ptr(), *dims, gw, A.data_ptr(), alpha.data_ptr(), y.data_ptr(),
                                       ws.ptr, n, st), "dstd_dstdgc_fwd")
        out["y_eval"] = y
    ns = L.dstd_dstdgc_train_saved_bytes_r(md, *dims, c.red)
    saved = b.new("saved", ns, fill)
    yt = b.f32("train y", (c.B, c.cout, c.T, c.V), NAN_OUT)
    native.check(L.dstd_dstdgc_train_fwd_r(md, x.data_ptr(), *dims, c.red, gw, A.data_ptr(), alpha.data_ptr(),
                                           yt.data_ptr(), saved.ptr, ns, st), "dstd_dstdgc_train_fwd_r")
    torch.cuda.synchronize()
    saved0 = saved.tensor.clone()
    nw = L.dstd_dstdgc_train_workspace_bytes_r(md, *dims, c.red)
    ws2 = b.new("backward workspace", nw, fill)
    dx, dA, dal = b.f32("dx", x.shape, 0), b.f32("dA", A.shape, 0), b.f32("dalpha", (1,), 0)
    params = list(op.parameters())
    arena = native.GradArena(params, _dev(), buf=b.f32("gradient arena", (native.arena_numel(params),), 0))
    native.check(L.dstd_dstdgc_train_bwd_r(md, x.data_ptr(), *dims, c.red, gw, alpha.data_ptr(), saved.ptr, ns,
                                           w.data_ptr(), dx.data_ptr(), native.gc_grads(op, arena), dA.data_ptr(),
                                           dal.data_ptr(), ws2.ptr, nw, st), "dstd_dstdgc_train_bwd_r")
    b.check()
    assert torch.equal(saved.tensor, saved0), "the backward wrote to saved"
    out.update(y=yt, dx=dx, dA=dA, dalpha=dal)
    out.update({name: v for (name, _), v in zip(op.named_parameters(), arena.views())})
    return _keep(out)


@pytest.mark.parametrize("c", OPS, ids=E.case_id)
def test_op(c):
    op, x, A, alpha, w = _op_on_device(c)
    inputs = [x, A, alpha, w] + list(op.parameters())
    before = _clones(inputs)
    got = run_fills(lambda fill: op_call(c, op, x, A, alpha, w, fill), E.case_id(c))
    _unchanged(inputs, before, E.case_id(c))
    ref = _op_ref(c)
    if "y_eval" in got:
        err = rel(got.pop("y_eval"), ref["y"])
        print(f"{E.case_id(c)}: eval forward {err:.2e}")
        assert err <= E.OP_BAR
    errs = E.op_errors(got, ref)
    name, err = _worst(errs)
    print(f"{E.case_id(c)}: train worst {err:.2e} ({name})")
    for k, v in errs.items():
        assert v < E.OP_BAR, (k, v)


# =====================================================================================
# blocks, eval: the generic cases, and the three kinds of block on the split-f16 layouts
# =====================================================================================
SPLIT_BLOCKS = [E.BlockCase(ci, co, G.LAYOUT_OF_V[V], T, V, B) for T, V in G.SPLIT_TV for ci, co in G.SPLIT_CHANNELS
                for B in G.SPLIT_B]


def _block_id(c):
    return f"c{c.cin}x{c.cout}-T{c.T}-V{c.V}-B{c.B}"


def _guard_bn(b, sb, mod, name):
    """Point the running statistics of the ctypes dstd_bn ``sb`` at guarded
    copies of BatchNorm1d ``mod``'s; returns [mean, var] (the guarded views)."""
    out = []
    for which in ("running_mean", "running_var"):
        src = getattr(mod, which)
        t = b.f32(f"{name}.{which}", src.shape, 0, like=src)
        setattr(sb, which, t.data_ptr())
        out.append(t)
    return out


def _guard_block_stats(b, sp, blk, name):
    """... of a block, in the oracle's call order (residual BN, then bn)."""
    out = []
    if blk.in_channels != blk.out_channels:
        out += _guard_bn(b, sp.res_bn, blk.residual[1].bn, name + ".residual")
    return out + _guard_bn(b, sp.bn, blk.bn.bn, name + ".bn")


def block_eval_call(blk, x, flags, fill, taps=None):
    """dstd_block_fwd_ex, or dstd_block_fwd_taps when ``taps`` names taps."""
    L, st = native.lib(), _stream()
    B, cin, T, V = x.shape
    cout = blk.out_channels
    b = Bufs()
    n = (L.dstd_block_taps_workspace_bytes if taps else L.dstd_block_workspace_bytes)(B, cin, cout, T, V)
    ws = b.new("workspace", n, fill)
    y = b.f32("y", (B, cout, T, V), NAN_OUT)
    out = {"y": y}
    if taps:
        shapes = {"adj_s": (B, 2, T, V, V), "adj_t": (B, V, T, T), "x": (B, cin, T, V), "h": (B, cout, T, V)}
        ts = native.BlockTaps()
        for name in taps:
            out[name] = b.f32("tap " + name, shapes[name], NAN_OUT)
            setattr(ts, name, out[name].data_ptr())
        native.check(L.dstd_block_fwd_taps(native.block_struct(blk), x.data_ptr(), B, T, V, y.data_ptr(), ts, ws.ptr,
                                           n, st, flags), "dstd_block_fwd_taps")
    else:
        native.check(L.dstd_block_fwd_ex(native.block_struct(blk), x.data_ptr(), B, T, V, y.data_ptr(), ws.ptr, n, st,
                                         flags), "dstd_block_fwd_ex")
    b.check()
    return _keep(out)


@pytest.mark.parametrize("c", E.BLOCK_EVAL_CASES + SPLIT_BLOCKS, ids=_block_id)
def test_block_eval(c):
    blk, x = E.build_block_eval(c)
    y64 = E.block_eval_reference(c, built=(blk, x))
    blk, x = blk.to(DEV).eval(), x.to(DEV)
    inputs = [x] + list(blk.parameters()) + list(blk.buffers())
    before = _clones(inputs)
    split = (c.T, c.V) in G.SPLIT_TV
    for flags in (BLOCK_FLAGS if split else (0, native.FWD_EXACT_FP32)):
        got = run_fills(lambda fill: block_eval_call(blk, x, flags, fill), f"{_block_id(c)} flags {flags}")
        err = rel(got["y"], y64)
        print(f"{_block_id(c)} flags {flags}: {err:.2e}")
        assert err <= E.BLOCK_EVAL_BAR, flags
    _unchanged(inputs, before, _block_id(c))


# ---- block taps: one split layout, one generic T, both arithmetics ----------------
TAP_BLOCKS = [E.BlockCase(64, 64, "h36m", 35, 22, 3), E.BlockCase(6, 64, "cmu", 17, 25, 2)]


def _check_block_taps(got, x, sd, y64, t64, what):
    """x is the input bit for bit; h against the fp64 oracle; each adjacency
    against the fp64 restatement fed the tapped x / h (tests/test_gpu_taps.py)."""
    assert torch.equal(got["x"], x), what
    a_s, a_t = H.block_adjacencies(got["x"], got["h"], sd)
    errs = {"h": H.rel(got["h"], t64["h"]), "adj_s0": H.rel(got["adj_s"][:, 0], a_s[:, 0]),
            "adj_s1": H.rel(got["adj_s"][:, 1], a_s[:, 1]), "adj_t": H.rel(got["adj_t"], a_t)}
    print(what, {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= H.TAP_BAR, (what, errs)


@pytest.mark.parametrize("c", TAP_BLOCKS, ids=_block_id)
def test_block_taps(c):
    blk, x = E.build_block_eval(c)
    sd = {k: v.detach().clone() for k, v in blk.state_dict().items()}
    y64, t64 = H.oracle_block_taps(x, sd)
    blk, x = blk.to(DEV).eval(), x.to(DEV)
    inputs = [x] + list(blk.parameters()) + list(blk.buffers())
    before = _clones(inputs)
    for flags in (0, native.FWD_EXACT_FP32):
        what = f"{_block_id(c)} taps flags {flags}"
        got = run_fills(lambda fill: block_eval_call(blk, x, flags, fill, taps=native.TAP_NAMES), what)
        assert rel(got["y"], y64) <= E.BLOCK_EVAL_BAR
        _same({"y": got["y"]}, {"y": block_eval_call(blk, x, flags, 0x4B)["y"]}, what + ": y against the plain forward")
        _check_block_taps(got, x, sd, y64, t64[0], what)
    _unchanged(inputs, before, _block_id(c))


# =====================================================================================
# blocks, train mode: every BLOCK_TRAIN_CASES entry
# =====================================================================================
def block_train_call(blk, x, w, flags, fill, need_dx=True):
    L, st = native.lib(), _stream()
    B, cin, T, V = x.shape
    cout = blk.out_channels
    b = Bufs()
    p = native.block_struct(blk)
    stats = _guard_block_stats(b, p, blk, "block")
    ns = L.dstd_block_train_saved_bytes(B, cin, cout, T, V)
    saved = b.new("saved", ns, fill)
    y = b.f32("y", (B, cout, T, V), NAN_OUT)
    native.check(L.dstd_block_train_fwd_ex(p, x.data_ptr(), B, T, V, 0.1, y.data_ptr(), saved.ptr, ns, st, flags),
                 "dstd_block_train_fwd_ex")
    torch.cuda.synchronize()
    saved0 = saved.tensor.clone()
    stats0 = _clones(stats)
    nw = L.dstd_block_train_workspace_bytes(B, cin, cout, T, V)
    ws = b.new("workspace", nw, fill)
    dx = b.f32("dx", x.shape, 0) if need_dx else None
    params = list(blk.parameters())
    arena = native.GradArena(params, _dev(), buf=b.f32("gradient arena", (native.arena_numel(params),), 0))
    native.check(L.dstd_block_train_bwd_ex(p, x.data_ptr(), B, T, V, saved.ptr, ns, w.data_ptr(),
                                           dx.data_ptr() if need_dx else None, native.block_grads(blk, arena), ws.ptr,
                                           nw, st, flags), "dstd_block_train_bwd_ex")
    b.check()
    assert torch.equal(saved.tensor, saved0), "the backward wrote to saved"
    _unchanged(stats, stats0, "running statistics across the backward")
    out = {"y": y}
    if need_dx:
        out["dx"] = dx
    out.update({f"stat{i}": s for i, s in enumerate(stats)})
    out.update({"grad " + name: v for (name, _), v in zip(blk.named_parameters(), arena.views()) if v is not None})
    return _keep(out)


@functools.lru_cache(maxsize=None)
def _block_train_ref(c):
    return E.block_train_reference(c)


def _check_running_stats(got_stats, old_stats, ref_stats, what, tol=1e-5):
    """(1 - m) * old + m * batch (unbiased variance), m = 0.1, within 1e-5 of
    the vector's max for a block (tests/test_gpu_envelope.py).  For a whole
    model ``tol`` is the model's own output bar: a statistic is a mean over
    activations that carry the error of the blocks before them, which that bar
    bounds at the output."""
    assert len(got_stats) == 2 * len(ref_stats)
    for i, (mean, var) in enumerate(ref_stats):
        assert rel(got_stats[2 * i], 0.9 * old_stats[2 * i].double().cpu() + 0.1 * mean) < tol, (what, i)
        assert rel(got_stats[2 * i + 1], 0.9 * old_stats[2 * i + 1].double().cpu() + 0.1 * var) < tol, (what, i)


def _block_stats_of(blk):
    out = []
    if blk.in_channels != blk.out_channels:
        out += [blk.residual[1].bn.running_mean, blk.residual[1].bn.running_var]
    return out + [blk.bn.bn.running_mean, blk.bn.bn.running_var]


@pytest.mark.parametrize("c", E.BLOCK_TRAIN_CASES, ids=E.case_id)
def test_block_train(c):
    blk, x, w = E.build_block_train(c)
    ref = _block_train_ref(c)
    blk = blk.to(DEV).train()
    _realias(blk)
    x, w = x.to(DEV), w.to(DEV)
    inputs = [x, w] + list(blk.parameters()) + list(blk.buffers())
    before = _clones(inputs)
    got = run_fills(lambda fill: block_train_call(blk, x, w, 0, fill), E.case_id(c))
    _unchanged(inputs, before, E.case_id(c))  # (the module's own running statistics: the call updated guarded copies)
    grads = {k[5:]: v for k, v in got.items() if k.startswith("grad ")}
    errs = E.block_train_errors({"y": got["y"], "dx": got["dx"], "grads": grads}, ref)
    name, err = _worst(errs)
    print(f"{E.case_id(c)}: worst {err:.2e} ({name})")
    assert errs["y"] < E.BLOCK_TRAIN_BAR and errs["dx"] < E.BLOCK_TRAIN_BAR
    for k, v in errs.items():
        assert v <= E.BLOCK_TRAIN_BAR, (k, v)
    stats = [got[f"stat{i}"] for i in range(2 * len(ref["stats"]))]
    _check_running_stats(stats, _block_stats_of(blk), ref["stats"], E.case_id(c))


# =====================================================================================
# models on the split-f16 layouts
# =====================================================================================
FIXTURE_OF = {(35, 22): "h36m", (35, 25): "cmu", (40, 23): "3dpw", (75, 22): "h36m75"}
ENC_GAMMA_L9 = 0.5


@functools.lru_cache(maxsize=None)
def synth_model(T, V, layers):
    """A model (CPU, eval) of ``layers`` encoder blocks with the weights of the
    layout's five-layer fixture model (every dynamic term alive): encoder i
    takes fixture encoder i % 5.  These are random-weight models and their
    conditioning falls with depth -- in fp64 a half-ulp change of the input
    moves the two-layer outputs by 9e-7..4e-6 of their max (the fp32 oracle is
    at 3e-6..1.2e-5) but a nine-layer one by 6e-3 (fp32 oracle 1.6e-2: no
    anchor at all).  The nine-layer model therefore halves the gain of the
    BatchNorm after each encoder block, which brings it to 1e-6 (fp32 oracle
    2e-6)."""
    d = load_npz(f"model_{FIXTURE_OF[T, V]}.npz")
    opts = {k[4:]: d[k].item() for k in d.files if k.startswith("opt/")}
    src, n_src = group(d, "sd/"), opts["num_layers"]
    assert opts["input_time_frame"] + opts["output_time_frame"] == T and opts["joints_to_consider"] == V
    m = get_model("dstdgcn", dstdgcn=dict(opts, num_layers=layers))
    sd = {k: torch.from_numpy(v) for k, v in src.items() if not k.startswith("encoders.")}
    for i in range(layers):
        pre = f"encoders.{i % n_src}."
        for k, v in src.items():
            if k.startswith(pre):
                t = torch.from_numpy(v).clone()
                if layers > n_src and k.endswith(".1.bn.weight"):
                    t *= ENC_GAMMA_L9
                sd[f"encoders.{i}." + k[len(pre):]] = t
    m.load_state_dict(sd)
    return m.eval()


def _model_input(T, V, B):
    return H.synth_input(B, T, V, synth_model(T, V, 2).input_time_frame, 700 + 7 * T + V + B)


@functools.lru_cache(maxsize=None)
def _model_ref(T, V, layers, B, training=False):
    """(fp64 y, the bar: conftest.model_tol of the fp32 oracle's own error,
    [(batch mean, unbiased batch variance)] per BatchNorm in call order)."""
    m, x = synth_model(T, V, layers), _model_input(T, V, B)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    O.BN_RECORD = rec = [] if training else None
    try:
        y64 = O.dstdgcn(x, sd, layers, training=training).numpy()
    finally:
        O.BN_RECORD = None
    ref32 = rel_err(O.dstdgcn(x, sd, layers, dtype=torch.float32, training=training).numpy(), y64)
    return y64, model_tol(ref32), rec


@functools.lru_cache(maxsize=None)
def _model_ref_paired(T, V, layers, B):
    """DSTD_TRAIN_PAIRED is two train-mode forwards of B/2: _model_ref's
    triple for each half of the same input, the oracle run on the half alone."""
    m, x = synth_model(T, V, layers), _model_input(T, V, B)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    halves = []
    for xh in x.chunk(2):
        O.BN_RECORD = rec = []
        try:
            y64 = O.dstdgcn(xh, sd, layers, training=True).numpy()
        finally:
            O.BN_RECORD = None
        ref32 = rel_err(O.dstdgcn(xh, sd, layers, dtype=torch.float32, training=True).numpy(), y64)
        halves.append((y64, model_tol(ref32), rec))
    return halves


def _on_gpu(m, train=False):
    m = copy.deepcopy(m).to(DEV)
    _realias(m)
    return m.train() if train else m.eval()


def _model_blocks(m):
    """[(ctypes path, module, name)] of the model's DSTDGCBs and the BatchNorms
    between them, in forward (= the oracle's BatchNorm call) order."""
    out = [("st_in", m.conv_st_in.stgcn[0][0]), ("bn_in", m.bn_in.bn)]
    for i, enc in enumerate(m.encoders):
        out += [(("enc", i), enc[0].stgcn[0][0]), (("enc_bn", i), enc[1].bn)]
    return out + [("st_out", m.conv_st_out.stgcn[0][0])]


def _guard_model_stats(b, p, m):
    stats = []
    for path, mod in _model_blocks(m):
        sp = getattr(p, path) if isinstance(path, str) else getattr(p, path[0])[path[1]]
        name = path if isinstance(path, str) else f"{path[0]}{path[1]}"
        stats += _guard_block_stats(b, sp, mod, name) if isinstance(mod, DSTDGCB) else _guard_bn(b, sp, mod, name)
    return stats


def _model_stats_of(m):
    out = []
    for _, mod in _model_blocks(m):
        out += _block_stats_of(mod) if isinstance(mod, DSTDGCB) else [mod.running_mean, mod.running_var]
    return out


def model_eval_call(m, x, flags, fill, taps=None):
    """dstd_model_fwd_ex, or dstd_model_fwd_taps (every tap of every block)
    when ``taps`` is set."""
    L, st = native.lib(), _stream()
    n, t, v, _ = x.shape
    C, nb = m.num_feature, m.num_layers + 2
    b = Bufs()
    nbytes = (L.dstd_model_taps_workspace_bytes if taps else L.dstd_model_workspace_bytes)(n, t, v, C, m.num_layers)
    ws = b.new("workspace", nbytes, fill)
    y = b.f32("y", x.shape, NAN_OUT)
    out = {"y": y}
    if taps:
        arr = (native.BlockTaps * nb)()
        for k in range(nb):
            cin, cout = (6 if k == 0 else C), (3 if k == nb - 1 else C)
            shapes = {"adj_s": (n, 2, t, v, v), "adj_t": (n, v, t, t), "x": (n, cin, t, v), "h": (n, cout, t, v)}
            for name in native.TAP_NAMES:
                out[f"{k}.{name}"] = b.f32(f"tap {k}.{name}", shapes[name], NAN_OUT)
                setattr(arr[k], name, out[f"{k}.{name}"].data_ptr())
        native.check(L.dstd_model_fwd_taps(m._native_params(), x.data_ptr(), n, y.data_ptr(), arr, ws.ptr, nbytes, st,
                                           flags), "dstd_model_fwd_taps")
    else:
        native.check(L.dstd_model_fwd_ex(m._native_params(), x.data_ptr(), n, y.data_ptr(), ws.ptr, nbytes, st, flags,
                                         None), "dstd_model_fwd_ex")
    b.check()
    return _keep(out)


MODELS = [(T, V, 2, B) for T, V in G.SPLIT_TV for B in G.SPLIT_B] + [(35, 22, 9, 3)]


def _model_id(a):
    return "T{}-V{}-L{}-B{}".format(*a)


@pytest.mark.parametrize("T,V,layers,B", MODELS, ids=[_model_id(a) for a in MODELS])
def test_model_eval(T, V, layers, B):
    y64, bar, _ = _model_ref(T, V, layers, B)
    m = _on_gpu(synth_model(T, V, layers))
    x = _model_input(T, V, B).to(DEV)
    inputs = [x] + list(m.parameters()) + list(m.buffers())
    before = _clones(inputs)
    first = None
    for flags in MODEL_FLAGS:
        what = f"{_model_id((T, V, layers, B))} flags {flags}"
        got = run_fills(lambda fill: model_eval_call(m, x, flags, fill), what)
        err = rel_err(got["y"].cpu().numpy(), y64)
        print(f"{what}: {err:.2e} (bar {bar:.1e})")
        assert err <= bar, what
        if flags & native.FWD_EXACT_FP32 == 0:  # the launch schedules give the same results bit for bit (dstd_gcn.h)
            first = first or got
            _same(first, got, what + " against flags 0")
    _unchanged(inputs, before, "model eval")


@pytest.mark.parametrize("name", ["split-T35-V22-L2-B3", "syn-T12-B3"])
def test_model_taps(name):
    """dstd_model_fwd_taps in both arithmetics on a split layout and on the
    generic kernels (taps_helper's T = 12 model)."""
    if name.startswith("split"):
        m0, x0 = synth_model(35, 22, 2), _model_input(35, 22, 3)
        sd = {k: v.detach().clone() for k, v in m0.state_dict().items()}
        y64, taps64 = H.oracle_taps(x0, sd, 2)
        layers = 2
    else:
        c = H.case(name)
        m0, x0, sd, y64, taps64, layers = c.module, c.x, c.sd, c.y64, c.taps64, c.num_layers
    m, x = _on_gpu(m0), x0.to(DEV)
    inputs = [x] + list(m.parameters()) + list(m.buffers())
    before = _clones(inputs)
    sd64 = H.cast_sd(sd, torch.float64)
    for flags in (0, native.FWD_EXACT_FP32):
        what = f"{name} taps flags {flags}"
        got = run_fills(lambda fill: model_eval_call(m, x, flags, fill, taps=True), what)
        _same({"y": got["y"]}, {"y": model_eval_call(m, x, flags, 0x4B)["y"]}, what + ": y against the plain forward")
        assert torch.equal(got["0.x"], H.model_input6(x).contiguous())
        for k, pre in enumerate(H.block_prefixes(layers)):
            blk = {n: got[f"{k}.{n}"] for n in native.TAP_NAMES}
            a_s, a_t = H.block_adjacencies(blk["x"], blk["h"], O.sub(sd64, pre))
            errs = [H.rel(blk["adj_s"][:, i], a_s[:, i]) for i in range(2)] + [H.rel(blk["adj_t"], a_t)]
            print(f"{what} block {k}: adj_s {errs[0]:.2e} {errs[1]:.2e} adj_t {errs[2]:.2e}")
            assert max(errs) <= H.TAP_BAR, (what, k, errs)
            # ... and through the fp64 oracle pieces: x and adj_s give h
            p = O.sub(sd64, pre)
            e_h = H.rel(blk["h"], H.spatial_half(blk["x"].double().cpu(), blk["adj_s"].double().cpu(), p))
            assert e_h <= H.TAP_BAR, (what, k, e_h)
    _unchanged(inputs, before, name)


# ---- model train forward + backward through the ABI ------------------------------------
PAIRED, RUNNING, ONE_STREAM = native.TRAIN_PAIRED, native.TRAIN_RUNNING_STATS, native.TRAIN_ONE_STREAM
# (T, V, flags, B, dropout, dx): every flag, both dropout rates and dx NULL / non-NULL on one layout,
# the plain call on the others
MODEL_TRAIN = [(35, 22, 0, 3, 0.0, True), (35, 22, 0, 3, 0.1, False), (35, 22, PAIRED, 2, 0.0, True),
               (35, 22, PAIRED, 2, 0.1, True), (35, 22, RUNNING, 3, 0.0, True), (35, 22, ONE_STREAM, 3, 0.0, False),
               (35, 22, ONE_STREAM, 3, 0.1, True), (35, 25, 0, 3, 0.0, True), (40, 23, 0, 3, 0.1, True),
               (75, 22, 0, 2, 0.0, True)]
SEED = 0x5DEECE66D


def model_train_call(m, x, dy, flags, drop, need_dx, fill):
    L, st = native.lib(), _stream()
    n, t, v, _ = x.shape
    C, layers = m.num_feature, m.num_layers
    b = Bufs()
    p = native.ModelParams.from_buffer_copy(m._native_params())
    stats = _guard_model_stats(b, p, m)
    ns = L.dstd_model_train_saved_bytes(n, t, v, C, layers)
    saved = b.new("saved", ns, fill)
    y = b.f32("y", x.shape, NAN_OUT)
    native.check(L.dstd_model_train_fwd_ex(p, x.data_ptr(), n, 0.1, drop, SEED, y.data_ptr(), saved.ptr, ns, st, flags),
                 "dstd_model_train_fwd_ex")
    torch.cuda.synchronize()
    saved0 = saved.tensor.clone()
    stats0 = _clones(stats)
    nw = L.dstd_model_train_workspace_bytes(n, t, v, C, layers)
    ws = b.new("workspace", nw, fill)
    dx = b.f32("dx", x.shape, NAN_OUT) if need_dx else None  # the model's dx is (=)
    params = list(m.parameters())
    arena = native.GradArena(params, _dev(), buf=b.f32("gradient arena", (native.arena_numel(params),), 0))
    native.check(L.dstd_model_train_bwd_ex(p, x.data_ptr(), n, drop, SEED, saved.ptr, ns, dy.data_ptr(),
                                           m._native_grads(arena), dx.data_ptr() if need_dx else None, ws.ptr, nw, st,
                                           flags), "dstd_model_train_bwd_ex")
    b.check()
    assert torch.equal(saved.tensor, saved0), "the backward wrote to saved"
    _unchanged(stats, stats0, "running statistics across the backward")
    out = {"y": y}
    if need_dx:
        out["dx"] = dx
    out.update({f"stat{i}": s for i, s in enumerate(stats)})
    out.update({"grad " + name: g for (name, _), g in zip(m.named_parameters(), arena.views()) if g is not None})
    return _keep(out)


@pytest.mark.parametrize("T,V,flags,B,drop,need_dx", MODEL_TRAIN,
                         ids=[f"T{a[0]}-V{a[1]}-f{a[2]}-B{a[3]}-p{a[4]}-dx{int(a[5])}" for a in MODEL_TRAIN])
def test_model_train(T, V, flags, B, drop, need_dx):
    m = _on_gpu(synth_model(T, V, 2), train=True)
    x = _model_input(T, V, B).to(DEV)
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(800 + T + V)).to(DEV)
    inputs = [x, dy] + list(m.parameters()) + list(m.buffers())
    before = _clones(inputs)
    what = f"model train T{T} V{V} flags {flags} B{B} p{drop}"
    got = run_fills(lambda fill: model_train_call(m, x, dy, flags, drop, need_dx, fill), what)
    _unchanged(inputs, before, what)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (what, k)
    old = _model_stats_of(m)
    stats = [got[f"stat{i}"] for i in range(len(old))]
    if flags & RUNNING:  # eval-mode BatchNorm: the eval forward's function, statistics untouched
        _unchanged(stats, _clones(old), what + ": running statistics under RUNNING_STATS")
        y64, bar, _ = _model_ref(T, V, 2, B)
        assert rel_err(got["y"].cpu().numpy(), y64) <= bar
    elif drop == 0.0 and not flags & PAIRED:
        y64, bar, rec = _model_ref(T, V, 2, B, training=True)
        err = rel_err(got["y"].cpu().numpy(), y64)
        print(f"{what}: y {err:.2e} (bar {bar:.1e})")
        assert err <= bar
        _check_running_stats(stats, old, rec, what, tol=bar)
    elif drop == 0.0:  # PAIRED: each half against the oracle on that half alone, statistics updated by one then the other
        halves = _model_ref_paired(T, V, 2, B)
        for yh, (y64, bar, _) in zip(got["y"].chunk(2), halves):
            err = rel_err(yh.cpu().numpy(), y64)
            print(f"{what}: half y {err:.2e} (bar {bar:.1e})")
            assert err <= bar
        tol = max(h[1] for h in halves)
        assert len(stats) == 2 * len(halves[0][2])
        for i, ((m1, v1), (m2, v2)) in enumerate(zip(halves[0][2], halves[1][2])):
            for j, (s1, s2) in enumerate(((m1, m2), (v1, v2))):
                want = 0.9 * (0.9 * old[2 * i + j].double().cpu() + 0.1 * s1) + 0.1 * s2
                assert rel(stats[2 * i + j], want) < tol, (what, i, j)
    # (dropout: held here by finiteness and bit identity across the fills; the mask restated on the host and the
    # step against the fp64 oracle with it: tests/dropout_helper.py, tests/test_gpu_dropout.py)


# =====================================================================================
# the Python layer under guarded_workspaces
# =====================================================================================
@pytest.mark.parametrize("T,V", G.SPLIT_TV, ids=[f"T{T}-V{V}" for T, V in G.SPLIT_TV])
def test_python_model_paths(T, V):
    """model(x), forward_taps and an eval-mode backward: every workspace the
    modules and autograd functions ask for is exact-size and poisoned."""
    B = 3
    y64, bar, _ = _model_ref(T, V, 2, B)
    m = _on_gpu(synth_model(T, V, 2))
    x = _model_input(T, V, B).to(DEV)
    w = torch.randn(x.shape, generator=torch.Generator().manual_seed(900 + T)).to(DEV)

    def call(fill):
        with G.guarded_workspaces(fill) as rec:
            with torch.no_grad():
                out = {"y": m(x)}
            yt, taps = m.forward_taps(x)
            out["y taps"] = yt
            for k, t in taps.items():
                out.update({f"{k}.{n}": getattr(t, n) for n in native.TAP_NAMES})
            m.zero_grad(set_to_none=True)
            xg = x.clone().requires_grad_(True)
            yg = m(xg)
            (yg * w).sum().backward()
            out.update({"y grad": yg, "dx": xg.grad})
            out.update({"grad " + n: p.grad for n, p in m.named_parameters() if p.grad is not None})
            sizes = [g.nbytes for g in rec.handed]
        L = native.lib()
        assert sizes == [L.dstd_model_workspace_bytes(B, T, V, 64, 2), L.dstd_model_taps_workspace_bytes(B, T, V, 64, 2),
                         L.dstd_model_train_workspace_bytes(B, T, V, 64, 2)], sizes
        return _keep(out)

    got = run_fills(call, f"python model T{T} V{V}")
    assert torch.equal(got["y"], got["y taps"])
    assert torch.equal(got["y"], model_eval_call(m, x, 0, 0x00)["y"])
    assert rel_err(got["y"].cpu().numpy(), y64) <= bar
    assert rel_err(got["y grad"].cpu().numpy(), y64) <= bar  # the fp32 training kernels on running statistics
    assert sum(k.startswith("grad ") for k in got) == sum(p.requires_grad for p in m.parameters())


PY_OPS = [E.OpCase("spatial", 24, 40, 20, 17, 2, 3), E.OpCase("temporal", 13, 17, 49, 16, 2, 2),
          E.OpCase("temporal", 20, 64, 35, 22, 8, 2)]
PY_BLOCKS = [E.BlockCase(6, 64, "cmu", 17, 25, 4), E.BlockCase(64, 3, "3dpw", 65, 23, 1)]
assert all(c in E.OP_CASES for c in PY_OPS) and all(c in E.BLOCK_TRAIN_CASES for c in PY_BLOCKS)


@pytest.mark.parametrize("c", PY_OPS, ids=E.case_id)
def test_python_op(c):
    """The DSTDGC module (eval forward, autograd forward + backward) on
    guarded workspaces gives what the ABI calls of test_op give, bit for bit."""
    op, x, A, alpha, w = _op_on_device(c)
    want = op_call(c, op, x, A, alpha, w, 0x00)
    L, md, dims = native.lib(), _mode(c), (c.B, c.cin, c.cout, c.T, c.V)
    for fill in G.FILLS[1:]:
        op.zero_grad(set_to_none=True)
        xg, Ag, ag = (t.clone().requires_grad_(True) for t in (x, A, alpha))
        with G.guarded_workspaces(fill) as rec:
            with torch.no_grad():
                y_eval = op(x, A, alpha)
            y = op(xg, Ag, ag)
            (y * w).sum().backward()
            sizes = [g.nbytes for g in rec.handed]
        assert sizes == ([L.dstd_dstdgc_workspace_bytes(md, *dims)] if c.red == 2 else []) + [
            L.dstd_dstdgc_train_workspace_bytes_r(md, *dims, c.red)], sizes
        got = {"y": y, "dx": xg.grad, "dA": Ag.grad, "dalpha": ag.grad}
        got.update({name: p.grad for name, p in op.named_parameters()})
        got["y_eval"] = y_eval if c.red == 2 else None
        _same({k: v for k, v in want.items()}, {k: v for k, v in got.items() if v is not None},
              f"{E.case_id(c)}: the module on fill 0x{fill:02X} against the ABI calls")


@pytest.mark.parametrize("c", PY_BLOCKS, ids=E.case_id)
def test_python_block(c):
    """The DSTDGCB module in train mode (and its eval forward) on guarded
    workspaces against the ABI calls of test_block_train / test_block_eval."""
    blk0, x, w = E.build_block_train(c)
    x, w = x.to(DEV), w.to(DEV)
    ref_blk = blk0.to(DEV).train()
    _realias(ref_blk)
    want = block_train_call(ref_blk, x, w, 0, 0x00)
    want_eval = block_eval_call(ref_blk.eval(), x, 0, 0x00)["y"]
    ref_blk.train()
    L = native.lib()
    for fill in G.FILLS[1:]:
        blk = copy.deepcopy(ref_blk)  # (the module's own running statistics are updated in place)
        _realias(blk)
        xg = x.clone().requires_grad_(True)
        with G.guarded_workspaces(fill) as rec:
            y = blk(xg)
            (y * w).sum().backward()
            with torch.no_grad():
                y_eval = copy.deepcopy(ref_blk).eval()(x)
            sizes = [g.nbytes for g in rec.handed]
        assert sizes == [L.dstd_block_train_workspace_bytes(c.B, c.cin, c.cout, c.T, c.V),
                         L.dstd_block_workspace_bytes(c.B, c.cin, c.cout, c.T, c.V)], sizes
        got = {"y": y, "dx": xg.grad}
        got.update({f"stat{i}": s for i, s in enumerate(_block_stats_of(blk))})
        got.update({"grad " + name: p.grad for name, p in blk.named_parameters() if p.grad is not None})
        _same(want, got, f"{E.case_id(c)}: the module on fill 0x{fill:02X} against the ABI calls")
        assert torch.equal(y_eval, want_eval)


class _Log:
    def __init__(self):
        self.lines = []

    def info(self, msg, *a, **k):
        self.lines.append(msg)


def test_python_engine_step():
    """One PredictionEngine train step -- the batch and its time reversal, joint
    weights, three loss terms -- on the 3DPW fixture model, B = 2: the reported
    terms against loss_helper on the step's own outputs (the bar of
    tests/test_gpu_losses.py), and losses, parameters and buffers after the
    step bit-identical across the fills."""
    from engine import PredictionEngine
    d = load_npz("engine.npz")
    opts = dict(input_channels=6, input_time_frame=10, output_time_frame=30, st_gcnn_dropout=0.0,
                joints_to_consider=23, num_feature=64, num_layers=5, layout="3dpw")
    loss_cfg = dict(joint=["jl2", 1], transition=["tl2", 0.5], coordinate=["cl1", 0.1])
    wj = np.random.default_rng(14).uniform(0.2, 1.5, 23)
    wj[7] = 0.0
    batch = tuple(torch.from_numpy(d[f"train/{n}0"])[:2] for n in ("inp", "inv", "seq", "seq"))
    want = {}

    def call(fill):
        m = get_model("dstdgcn", dstdgcn=opts)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in group(d, "train/sd0/").items()})
        m = m.to(DEV)
        _realias(m)
        cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5), loss=loss_cfg, n_out=1,
                   transform="tsc", use_weight=True, inverse=True)
        eng = PredictionEngine(cfg, m.train(), _Log())
        captured, reported = [], []
        forward_pair = m.forward_pair  # (the engine's paired forward is no Module call: no forward hook fires)
        m.forward_pair = lambda a, a_inv: captured.append(forward_pair(a, a_inv)) or captured[-1]
        step = eng._step
        eng._step = lambda *a: reported.append(step(*a)) or reported[-1]
        with G.guarded_workspaces(fill) as rec:
            total = eng.train([batch], 0, weights=wj, max_iter=1)
            assert len(rec.handed) >= 2  # the loss and the model backward, at the least
        assert len(reported) == 1 and len(reported[0]) == 3 and len(captured) == 1
        if not want:
            ref = loss_terms(captured[0][0].detach().cpu().reshape(2, 40, 69), batch[2], wj)
            want.update({name: cw * float(ref[name]) for name, cw in loss_cfg.values()})
        out = {"total": torch.tensor(total, dtype=torch.float64),
               "terms": torch.stack([v.detach().double().cpu().reshape(()) if torch.is_tensor(v) else
                                     torch.tensor(float(v), dtype=torch.float64) for v in reported[0]])}
        out.update({"param " + n: p for n, p in m.named_parameters()})
        out.update({"buffer " + n: t for n, t in m.named_buffers()})
        return _keep(out)

    got = run_fills(call, "engine step")
    for g, (name, r) in zip(got["terms"].tolist(), want.items()):
        print(name, g, r)
        assert abs(g - r) <= 1e-5 * abs(r), (name, g, r)
    # the epoch total of one step is the sum of the forward pass's terms (tests/test_gpu_losses.py)
    total, total_ref = float(got["total"]), sum(want.values())
    print("total", total, total_ref)
    assert abs(total - total_ref) <= 1e-5 * total_ref
    assert all(bool(torch.isfinite(v).all()) for v in got.values())


@pytest.mark.parametrize("name", list(PLAIN))
def test_python_plain_layer(name):
    """ST_GCNN_layer(refine=False) -- ConvTemporalGraphical + Conv2d, both
    directions -- against the fp64 oracle at the bar of
    test_plain_st_gcnn_layer_forward_backward."""
    from model import ST_GCNN_layer
    cin, cout, ks, T = PLAIN[name]
    d = load_npz("plain_layers.npz")
    sd = group(d, f"{name}/sd/")
    layer = ST_GCNN_layer(cin, cout, ks, 1, T, 22, True, False, True, "h36m")
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    layer = layer.to(DEV)
    x = torch.from_numpy(d[f"{name}/x"])[:2]
    w = torch.randn(2, cout, T, 22, generator=torch.Generator().manual_seed(5))
    xd, wd = x.to(DEV), w.to(DEV)

    def call(fill):
        layer.zero_grad(set_to_none=True)
        xg = xd.clone().requires_grad_(True)
        with G.guarded_workspaces(fill) as rec:
            y = layer(xg)
            (y * wd).sum().backward()
            assert len(rec.handed) >= 4
        out = {"y": y, "dx": xg.grad}
        out.update({"grad " + k: p.grad for k, p in layer.named_parameters() if p.grad is not None})
        return _keep(out)

    got = run_fills(call, name)
    P = {k: torch.from_numpy(v).double().requires_grad_(not k.endswith("A_fixed")) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    y64 = O.st_gcnn_layer_plain(x64, P, ks, 1)
    (y64 * w.double()).sum().backward()
    assert rel(got["y"], y64) < 1e-4 and rel(got["dx"], x64.grad) < 1e-4
    for k, p in P.items():
        if p.grad is not None:
            assert rel(got["grad " + k], p.grad) < 1e-4, k


# =====================================================================================
# aux layers through the ABI: dx / db NULL and non-NULL
# =====================================================================================
def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("shape", G.CTG_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("need_dx", [True, False])
def test_ctg(shape, need_dx):
    L, st = native.lib(), _stream()
    B, C, T, V = shape
    x, Tm, A, Af, dy = (_randn(*s, seed=i) * sc for i, (s, sc) in enumerate(
        (((B, C, T, V), 1.0), ((V, T, T), T ** -0.5), ((T, V, V), V ** -0.5), ((V, V), 0.3), ((B, C, T, V), 1.0))))
    x64, Tm64, A64 = (t.double().requires_grad_(True) for t in (x, Tm, A))
    y64 = O.ctg(x64, {"T": Tm64, "A": A64, "A_fixed": Af.double()})
    (y64 * dy.double()).sum().backward()
    x, Tm, A, Af, dy = inputs = [t.to(DEV) for t in (x, Tm, A, Af, dy)]
    before = _clones(inputs)
    n = L.dstd_ctg_workspace_bytes(B, C, T, V)

    def call(fill):
        b = Bufs()
        ws = b.new("forward workspace", n, fill)
        y = b.f32("y", x.shape, NAN_OUT)
        native.check(L.dstd_ctg_fwd(x.data_ptr(), B, C, T, V, Tm.data_ptr(), A.data_ptr(), Af.data_ptr(), y.data_ptr(),
                                    ws.ptr, n, st), "dstd_ctg_fwd")
        ws2 = b.new("backward workspace", n, fill)
        dx = b.f32("dx", x.shape, 0) if need_dx else None
        dTm, dA = b.f32("dTm", Tm.shape, 0), b.f32("dA", A.shape, 0)
        native.check(L.dstd_ctg_bwd(x.data_ptr(), B, C, T, V, Tm.data_ptr(), A.data_ptr(), Af.data_ptr(),
                                    dy.data_ptr(), dx.data_ptr() if need_dx else None, dTm.data_ptr(), dA.data_ptr(),
                                    ws2.ptr, n, st), "dstd_ctg_bwd")
        b.check()
        out = {"y": y, "dTm": dTm, "dA": dA}
        if need_dx:
            out["dx"] = dx
        return _keep(out)

    got = run_fills(call, f"ctg {shape}")
    _unchanged(inputs, before, "ctg")
    ref = {"y": y64, "dTm": Tm64.grad, "dA": A64.grad, "dx": x64.grad}
    for k, v in got.items():
        assert rel(v, ref[k]) < 1e-4, (k, rel(v, ref[k]))  # test_plain_st_gcnn_layer_forward_backward


def _conv_bar(shape):
    """Each shape's bar where it comes from: 1e-4 for the three plain-layer
    convolutions (test_plain_st_gcnn_layer_forward_backward), 1e-5 for the
    strided, padded one (test_native_conv2d_strided_padded)."""
    assert len(G.CONV_SHAPES) == 4 and G.CONV_SHAPES[3][7:9] == (2, 1)
    return 1e-5 if shape == G.CONV_SHAPES[3] else 1e-4


@pytest.mark.parametrize("shape", G.CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("need_dx,need_db", [(True, True), (False, False)])
def test_conv2d(shape, need_dx, need_db):
    L, st = native.lib(), _stream()
    B, cin, cout, Hh, Ww, kh, kw, sh, sw, ph, pw = shape
    geom = (kh, kw, sh, sw, ph, pw)
    x, wt, bias = _randn(B, cin, Hh, Ww, seed=1), _randn(cout, cin, kh, kw, seed=2) * (cin * kh * kw) ** -0.5, \
        _randn(cout, seed=3) * 0.1
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, wt, bias))
    y64 = torch.nn.functional.conv2d(x64, w64, b64 if need_db else None, stride=(sh, sw), padding=(ph, pw))
    dy = _randn(*y64.shape, seed=4)
    (y64 * dy.double()).sum().backward()
    x, wt, bias, dy = inputs = [t.to(DEV) for t in (x, wt, bias, dy)]
    before = _clones(inputs)
    n = L.dstd_conv2d_workspace_bytes(B, cin, cout, Hh, Ww, *geom)

    def call(fill):
        b = Bufs()
        ws = b.new("forward workspace", n, fill)
        y = b.f32("y", y64.shape, NAN_OUT)
        native.check(L.dstd_conv2d_fwd(x.data_ptr(), B, cin, Hh, Ww, wt.data_ptr(), bias.data_ptr() if need_db else None,
                                       cout, *geom, y.data_ptr(), ws.ptr, n, st), "dstd_conv2d_fwd")
        ws2 = b.new("backward workspace", n, fill)
        dx = b.f32("dx", x.shape, 0) if need_dx else None
        dw = b.f32("dw", wt.shape, 0)
        db = b.f32("db", bias.shape, 0) if need_db else None
        native.check(L.dstd_conv2d_bwd(x.data_ptr(), B, cin, Hh, Ww, wt.data_ptr(), cout, *geom, dy.data_ptr(),
                                       dx.data_ptr() if need_dx else None, dw.data_ptr(),
                                       db.data_ptr() if need_db else None, ws2.ptr, n, st), "dstd_conv2d_bwd")
        b.check()
        out = {"y": y, "dw": dw}
        if need_dx:
            out["dx"] = dx
        if need_db:
            out["db"] = db
        return _keep(out)

    got = run_fills(call, f"conv2d {shape}")
    _unchanged(inputs, before, "conv2d")
    ref = {"y": y64, "dw": w64.grad, "dx": x64.grad, "db": b64.grad}
    bar = _conv_bar(shape)
    for k, v in got.items():
        print(f"conv2d {shape} {k}: {rel(v, ref[k]):.2e} (bar {bar:.0e})")
        assert rel(v, ref[k]) < bar, (k, rel(v, ref[k]))


# =====================================================================================
# losses through the ABI
# =====================================================================================
VALUE_TOL = GRAD_TOL = 1e-5  # tests/test_gpu_losses.py
ALL_TERMS = 15


def _loss_problems():
    d = load_npz("losses.npz")
    targets = _randn(3, 35, 66, seed=11)
    preds = [torch.from_numpy(d["positive/pred"]), torch.from_numpy(d["minmax/pred"])]
    return preds, targets, [(10, 1), (24, -1)], torch.from_numpy(d["minmax/w"])


def _slice(targets, t, step):
    return targets[:, -t:] if step == 1 else targets.flip(1)[:, -t:]


@pytest.mark.parametrize("nprob", [1, 2])
def test_losses(nprob):
    """dstd_losses_fwd / _bwd, all four terms, one and two problems."""
    from engine.loss import _problems
    L, st = native.lib(), _stream()
    preds, targets, maps, w = _loss_problems()
    preds, maps = preds[:nprob], maps[:nprob]
    assert all(p.shape[0] == 3 and p.shape[2] == 66 for p in preds)
    coef = torch.tensor([[3.0, 0.5, 2.0, 0.25], [1.5, 2.5, 0.75, 4.0]])[:nprob].contiguous()
    ref_v, ref_g = [], []
    for p, (_, step), cf in zip(preds, maps, coef):
        p64 = p.double().requires_grad_(True)
        terms = loss_terms(p64, _slice(targets, p.shape[1], step).contiguous(), w)
        ref_v.append([float(terms[t].detach()) for t in TERMS])
        (0.5 * sum(float(c) * terms[t] for t, c in zip(TERMS, cf))).backward()
        ref_g.append(p64.grad)
    preds = [p.to(DEV).contiguous() for p in preds]
    targets, w, coef = targets.to(DEV), w.to(DEV), coef.to(DEV)
    inputs = preds + [targets, w, coef]
    before = _clones(inputs)
    n = L.dstd_losses_workspace_bytes()

    def call(fill):
        b = Bufs()
        ws = b.new("workspace", n, fill)
        values = b.f32("values", (nprob, native.LOSS_NTERMS), NAN_OUT)
        native.check(L.dstd_losses_fwd(_problems(preds, targets, maps), nprob, ALL_TERMS, w.data_ptr(),
                                       values.data_ptr(), ws.ptr, n, st), "dstd_losses_fwd")
        dps = [b.f32(f"dpred {i}", p.shape, NAN_OUT) for i, p in enumerate(preds)]
        ptrs = (ctypes.c_void_p * nprob)(*[t.data_ptr() for t in dps])
        native.check(L.dstd_losses_bwd(_problems(preds, targets, maps), nprob, ALL_TERMS, w.data_ptr(), coef.data_ptr(),
                                       0.5, ptrs, st), "dstd_losses_bwd")
        b.check()
        return _keep({"values": values, **{f"dpred {i}": t for i, t in enumerate(dps)}})

    got = run_fills(call, f"losses, {nprob} problem(s)")
    _unchanged(inputs, before, "losses")
    for i in range(nprob):
        for k, t in enumerate(TERMS):
            assert abs(float(got["values"][i, k]) - ref_v[i][k]) < VALUE_TOL, (i, t)
        assert rel(got[f"dpred {i}"], ref_g[i]) < GRAD_TOL, i


def test_mpjpe():
    L, st = native.lib(), _stream()
    pred, targ = _randn(3, 25, 66, seed=21), _randn(3, 25, 66, seed=22)
    p64 = pred.double().requires_grad_(True)
    l64 = O.mpjpe_error_3d(p64, targ.double())
    (3.0 * l64).backward()
    pred, targ, g = inputs = [pred.to(DEV), targ.to(DEV), torch.tensor([1.5], device=DEV)]
    before = _clones(inputs)
    n, npts = L.dstd_loss_workspace_bytes(), pred.numel() // 3

    def call(fill):
        b = Bufs()
        ws = b.new("workspace", n, fill)
        loss = b.f32("loss", (1,), NAN_OUT)
        native.check(L.dstd_mpjpe_fwd(pred.data_ptr(), targ.data_ptr(), npts, loss.data_ptr(), ws.ptr, n, st),
                     "dstd_mpjpe_fwd")
        dp = b.f32("dpred", pred.shape, NAN_OUT)
        native.check(L.dstd_mpjpe_bwd(pred.data_ptr(), targ.data_ptr(), npts, g.data_ptr(), 2.0, dp.data_ptr(), st),
                     "dstd_mpjpe_bwd")
        b.check()
        return _keep({"loss": loss, "dpred": dp})

    got = run_fills(call, "mpjpe")
    _unchanged(inputs, before, "mpjpe")
    assert abs(float(got["loss"][0]) - float(l64.detach())) < 1e-5  # test_mpjpe_forward_backward
    assert rel(got["dpred"], p64.grad) < 1e-5


def test_frame_mpjpe():
    """dstd_frame_mpjpe (no workspace; sums accumulate): 22 of 32 joints
    predicted, two ignored joints copied from others, five frames.  Bar: an
    fp32 sum of B * J = 96 norms of O(1) carries a few ulp, 1e-5 relative is
    two orders above that."""
    L, st = native.lib(), _stream()
    B, T, J, t_out0 = 3, 35, 32, 10
    D = 3 * J
    rng = np.random.default_rng(31)
    used_joints = np.sort(rng.choice(J, 22, replace=False))
    dim_used = np.concatenate([3 * used_joints + c for c in range(3)])
    dim_used.sort()
    used_pos = -np.ones(D, dtype=np.int32)
    used_pos[dim_used] = np.arange(len(dim_used), dtype=np.int32)
    joint_src = np.arange(J, dtype=np.int32)
    unused = [j for j in range(J) if j not in set(used_joints)]
    joint_src[unused[0]], joint_src[unused[1]] = used_joints[0], used_joints[3]
    frames = np.array([10, 11, 17, 33, 34], dtype=np.int32)
    seqs, outs = _randn(B, T, D, seed=32), _randn(B, T - t_out0, len(dim_used), seed=33)
    ref = np.zeros(len(frames))
    s64, o64 = seqs.double().numpy(), outs.double().numpy()
    for k, f in enumerate(frames):
        pred = s64[:, f].copy()
        pred[:, dim_used] = o64[:, f - t_out0]
        pj = pred.reshape(B, J, 3)[:, joint_src]
        ref[k] = np.linalg.norm(s64[:, f].reshape(B, J, 3) - pj, axis=-1).sum() / J
    seqs, outs = seqs.to(DEV), outs.to(DEV)
    up, js, fr = (torch.from_numpy(a).to(DEV) for a in (used_pos, joint_src, frames))
    inputs = [seqs, outs, up, js, fr]
    before = _clones(inputs)

    def call(fill):
        b = Bufs()
        sums = b.f32("sums", (len(frames),), 0)
        for _ in range(2):  # (+=): two calls, twice the sums
            native.check(L.dstd_frame_mpjpe(seqs.data_ptr(), outs.data_ptr(), B, T, D, t_out0, up.data_ptr(),
                                            len(dim_used), js.data_ptr(), fr.data_ptr(), len(frames), sums.data_ptr(),
                                            st), "dstd_frame_mpjpe")
        b.check()
        return _keep({"sums": sums})

    got = run_fills(call, "frame_mpjpe")
    for t, c in zip(inputs, before):
        assert torch.equal(t, c)
    assert rel(got["sums"], torch.from_numpy(2 * ref)) < 1e-5


# =====================================================================================
# size checks: size - 1 of every workspace_bytes / saved_bytes is refused without a write
# =====================================================================================
def _refused(code, want, b, snap, what):
    torch.cuda.synchronize()
    assert code == want, (what, code)
    b.check_frozen(snap, what)


def test_size_checks_op():
    G.check_pinned_sizes([n for n, _ in G.PINNED_SIZES if "dstdgc" in n])
    L, st = native.lib(), _stream()
    c = E.OpCase("spatial", 24, 40, 20, 17, 2, 3)
    assert c in E.OP_CASES
    op, x, A, alpha, w = _op_on_device(c)
    md, dims = _mode(c), (c.B, c.cin, c.cout, c.T, c.V)
    gw = native.gc_weights(op)
    n, ns, nw = (L.dstd_dstdgc_workspace_bytes(md, *dims), L.dstd_dstdgc_train_saved_bytes(md, *dims),
                 L.dstd_dstdgc_train_workspace_bytes(md, *dims))
    assert ns == L.dstd_dstdgc_train_saved_bytes_r(md, *dims, 2) and nw == L.dstd_dstdgc_train_workspace_bytes_r(md, *dims, 2)
    b = Bufs()
    ws, saved, ws2 = b.new("eval workspace", n, 0x4B), b.new("saved", ns, 0x4B), b.new("backward workspace", nw, 0x4B)
    y = b.f32("y", (c.B, c.cout, c.T, c.V), NAN_OUT)
    dx, dA, dal = b.f32("dx", x.shape, 0x4B), b.f32("dA", A.shape, 0x4B), b.f32("dalpha", (1,), 0x4B)
    params = list(op.parameters())
    arena = native.GradArena(params, _dev(), buf=b.f32("gradient arena", (native.arena_numel(params),), 0x4B))
    gg = native.gc_grads(op, arena)
    snap = b.freeze()
    xa = (md, x.data_ptr(), *dims)
    _refused(L.dstd_dstdgc_fwd(*xa, gw, A.data_ptr(), alpha.data_ptr(), y.data_ptr(), ws.ptr, n - 1, st), EWORKSPACE, b,
             snap, "dstd_dstdgc_fwd")
    _refused(L.dstd_dstdgc_train_fwd(*xa, gw, A.data_ptr(), alpha.data_ptr(), y.data_ptr(), saved.ptr, ns - 1, st),
             EWORKSPACE, b, snap, "dstd_dstdgc_train_fwd")
    _refused(L.dstd_dstdgc_train_fwd_r(*xa, 2, gw, A.data_ptr(), alpha.data_ptr(), y.data_ptr(), saved.ptr, ns - 1, st),
             EWORKSPACE, b, snap, "dstd_dstdgc_train_fwd_r")
    for fn, red in ((L.dstd_dstdgc_train_bwd, ()), (L.dstd_dstdgc_train_bwd_r, (2,))):
        for s_bytes, w_bytes in ((ns - 1, nw), (ns, nw - 1)):
            _refused(fn(*xa, *red, gw, alpha.data_ptr(), saved.ptr, s_bytes, w.data_ptr(), dx.data_ptr(), gg,
                        dA.data_ptr(), dal.data_ptr(), ws2.ptr, w_bytes, st), EWORKSPACE, b, snap,
                     f"op backward saved {s_bytes - ns} workspace {w_bytes - nw}")
    got = op_call(c, op, x, A, alpha, w, 0xFF)  # the exact sizes succeed, straight after
    ref = _op_ref(c)
    assert rel(got.pop("y_eval"), ref["y"]) <= E.OP_BAR
    assert max(E.op_errors(got, ref).values()) < E.OP_BAR


def test_size_checks_block():
    G.check_pinned_sizes([n for n, _ in G.PINNED_SIZES if "block" in n])
    L, st = native.lib(), _stream()
    c = E.BlockCase(6, 64, "cmu", 17, 25, 2)
    ct = E.BlockCase(6, 64, "cmu", 17, 25, 4)
    assert c in E.BLOCK_EVAL_CASES and ct in E.BLOCK_TRAIN_CASES
    blk, x = E.build_block_eval(c)
    y64 = E.block_eval_reference(c, built=(blk, x))
    blk, x = blk.to(DEV).eval(), x.to(DEV)
    B, cin, T, V = x.shape
    cout = c.cout
    b = Bufs()
    p = native.block_struct(blk)
    stats = _guard_block_stats(b, p, blk, "block")
    n, ns, nw = (L.dstd_block_workspace_bytes(B, cin, cout, T, V), L.dstd_block_train_saved_bytes(B, cin, cout, T, V),
                 L.dstd_block_train_workspace_bytes(B, cin, cout, T, V))
    assert L.dstd_block_taps_workspace_bytes(B, cin, cout, T, V) == n
    ws, saved, ws2 = b.new("eval workspace", n, 0x4B), b.new("saved", ns, 0x4B), b.new("backward workspace", nw, 0x4B)
    y, dx = b.f32("y", (B, cout, T, V), NAN_OUT), b.f32("dx", x.shape, 0x4B)
    ts = native.BlockTaps()
    for name, shape in (("adj_s", (B, 2, T, V, V)), ("adj_t", (B, V, T, T)), ("x", x.shape), ("h", (B, cout, T, V))):
        setattr(ts, name, b.f32("tap " + name, shape, NAN_OUT).data_ptr())
    params = list(blk.parameters())
    arena = native.GradArena(params, _dev(), buf=b.f32("gradient arena", (native.arena_numel(params),), 0x4B))
    gg = native.block_grads(blk, arena)
    snap = b.freeze()
    xp, yp = x.data_ptr(), y.data_ptr()
    _refused(L.dstd_block_fwd(p, xp, B, T, V, yp, ws.ptr, n - 1, st), EWORKSPACE, b, snap, "dstd_block_fwd")
    _refused(L.dstd_block_fwd_ex(p, xp, B, T, V, yp, ws.ptr, n - 1, st, FUSED), EWORKSPACE, b, snap, "dstd_block_fwd_ex")
    _refused(L.dstd_block_fwd_taps(p, xp, B, T, V, yp, ts, ws.ptr, n - 1, st, 0), EWORKSPACE, b, snap,
             "dstd_block_fwd_taps")
    _refused(L.dstd_block_train_fwd(p, xp, B, T, V, 0.1, yp, saved.ptr, ns - 1, st), EWORKSPACE, b, snap,
             "dstd_block_train_fwd")
    _refused(L.dstd_block_train_fwd_ex(p, xp, B, T, V, 0.1, yp, saved.ptr, ns - 1, st, 0), EWORKSPACE, b, snap,
             "dstd_block_train_fwd_ex")
    for s_bytes, w_bytes in ((ns - 1, nw), (ns, nw - 1)):
        _refused(L.dstd_block_train_bwd(p, xp, B, T, V, saved.ptr, s_bytes, yp, dx.data_ptr(), gg, ws2.ptr, w_bytes, st),
                 EWORKSPACE, b, snap, "dstd_block_train_bwd")
        _refused(L.dstd_block_train_bwd_ex(p, xp, B, T, V, saved.ptr, s_bytes, yp, dx.data_ptr(), gg, ws2.ptr, w_bytes,
                                           st, 0), EWORKSPACE, b, snap, "dstd_block_train_bwd_ex")
    assert len(stats) == 4
    assert rel(block_eval_call(blk, x, 0, 0xFF)["y"], y64) <= E.BLOCK_EVAL_BAR
    # ... and the train-mode call
    tb, xt, wt = E.build_block_train(ct)
    ref = _block_train_ref(ct)
    tb = tb.to(DEV).train()
    _realias(tb)
    got = block_train_call(tb, xt.to(DEV), wt.to(DEV), 0, 0xFF)
    grads = {k[5:]: v for k, v in got.items() if k.startswith("grad ")}
    errs = E.block_train_errors({"y": got["y"], "dx": got["dx"], "grads": grads}, ref)
    assert max(errs.values()) <= E.BLOCK_TRAIN_BAR, errs


def test_size_checks_model():
    G.check_pinned_sizes([n for n, _ in G.PINNED_SIZES if "model" in n])
    L, st = native.lib(), _stream()
    T, V, layers, B = 35, 22, 2, 3
    m = _on_gpu(synth_model(T, V, layers), train=True)
    x = _model_input(T, V, B).to(DEV)
    C = 64
    b = Bufs()
    p = native.ModelParams.from_buffer_copy(m._native_params())
    _guard_model_stats(b, p, m)
    n, ns, nw = (L.dstd_model_workspace_bytes(B, T, V, C, layers), L.dstd_model_train_saved_bytes(B, T, V, C, layers),
                 L.dstd_model_train_workspace_bytes(B, T, V, C, layers))
    assert L.dstd_model_taps_workspace_bytes(B, T, V, C, layers) == n
    ws, saved, ws2 = b.new("eval workspace", n, 0x4B), b.new("saved", ns, 0x4B), b.new("backward workspace", nw, 0x4B)
    y, dx = b.f32("y", x.shape, NAN_OUT), b.f32("dx", x.shape, 0x4B)
    arr = (native.BlockTaps * (layers + 2))()
    arr[1].h = b.f32("tap 1.h", (B, C, T, V), NAN_OUT).data_ptr()
    params = list(m.parameters())
    arena = native.GradArena(params, _dev(), buf=b.f32("gradient arena", (native.arena_numel(params),), 0x4B))
    gg = m._native_grads(arena)
    snap = b.freeze()
    xp, yp = x.data_ptr(), y.data_ptr()
    _refused(L.dstd_model_fwd(p, xp, B, yp, ws.ptr, n - 1, st), EWORKSPACE, b, snap, "dstd_model_fwd")
    _refused(L.dstd_model_fwd_ex(p, xp, B, yp, ws.ptr, n - 1, st, FUSED, None), EWORKSPACE, b, snap, "dstd_model_fwd_ex")
    _refused(L.dstd_model_fwd_profiled(p, xp, B, yp, ws.ptr, n - 1, st, None), EWORKSPACE, b, snap,
             "dstd_model_fwd_profiled")
    _refused(L.dstd_model_fwd_taps(p, xp, B, yp, arr, ws.ptr, n - 1, st, 0), EWORKSPACE, b, snap, "dstd_model_fwd_taps")
    _refused(L.dstd_model_train_fwd(p, xp, B, 0.1, 0.1, SEED, yp, saved.ptr, ns - 1, st), EWORKSPACE, b, snap,
             "dstd_model_train_fwd")
    _refused(L.dstd_model_train_fwd_ex(p, xp, B, 0.1, 0.1, SEED, yp, saved.ptr, ns - 1, st, 0), EWORKSPACE, b, snap,
             "dstd_model_train_fwd_ex")
    _refused(L.dstd_model_train_fwd_sync(p, xp, B, 0.1, 0.1, SEED, yp, saved.ptr, ns - 1, st, 0, None), EWORKSPACE, b,
             snap, "dstd_model_train_fwd_sync")
    for s_bytes, w_bytes in ((ns - 1, nw), (ns, nw - 1)):
        _refused(L.dstd_model_train_bwd(p, xp, B, 0.1, SEED, saved.ptr, s_bytes, yp, gg, ws2.ptr, w_bytes, st),
                 EWORKSPACE, b, snap, "dstd_model_train_bwd")
        _refused(L.dstd_model_train_bwd_ex(p, xp, B, 0.1, SEED, saved.ptr, s_bytes, yp, gg, dx.data_ptr(), ws2.ptr,
                                           w_bytes, st, 0), EWORKSPACE, b, snap, "dstd_model_train_bwd_ex")
        _refused(L.dstd_model_train_bwd_sync(p, xp, B, 0.1, SEED, saved.ptr, s_bytes, yp, gg, dx.data_ptr(), ws2.ptr,
                                             w_bytes, st, 0, None), EWORKSPACE, b, snap, "dstd_model_train_bwd_sync")
    y64, bar, _ = _model_ref(T, V, layers, B)
    assert rel_err(model_eval_call(m.eval(), x, 0, 0xFF)["y"].cpu().numpy(), y64) <= bar
    y64t, bart, _ = _model_ref(T, V, layers, B, training=True)
    got = model_train_call(m.train(), x, torch.ones_like(x), 0, 0.0, True, 0xFF)
    assert rel_err(got["y"].cpu().numpy(), y64t) <= bart


def test_size_checks_aux_and_losses():
    G.check_pinned_sizes(["dstd_ctg_workspace_bytes", "dstd_conv2d_workspace_bytes", "dstd_loss_workspace_bytes",
                          "dstd_losses_workspace_bytes"])
    from engine.loss import _problems
    L, st = native.lib(), _stream()
    b = Bufs()
    # ConvTemporalGraphical
    B, C, T, V = G.CTG_SHAPES[1]
    x, Tm, A, Af = (_randn(*s, seed=i).to(DEV) for i, s in enumerate(((B, C, T, V), (V, T, T), (T, V, V), (V, V))))
    n = L.dstd_ctg_workspace_bytes(B, C, T, V)
    ws = b.new("ctg workspace", n, 0x4B)
    y, dx, dTm, dA = (b.f32("ctg " + k, t.shape, 0x4B) for k, t in (("y", x), ("dx", x), ("dTm", Tm), ("dA", A)))
    # Conv2d
    cs = G.CONV_SHAPES[3]
    Bc, cin, cout, Hh, Ww, kh, kw, sh, sw, ph, pw = cs
    Ho, Wo = (Hh + 2 * ph - kh) // sh + 1, (Ww + 2 * pw - kw) // sw + 1
    xc, wc, bc, dyc = (_randn(*s, seed=10 + i).to(DEV) for i, s in enumerate(
        ((Bc, cin, Hh, Ww), (cout, cin, kh, kw), (cout,), (Bc, cout, Ho, Wo))))
    nc = L.dstd_conv2d_workspace_bytes(*cs)
    wsc = b.new("conv2d workspace", nc, 0x4B)
    yc, dxc, dwc, dbc = (b.f32("conv2d " + k, t.shape, 0x4B) for k, t in (("y", dyc), ("dx", xc), ("dw", wc), ("db", bc)))
    # losses
    preds, targets, maps, w = _loss_problems()
    preds, targets, w = [p.to(DEV).contiguous() for p in preds], targets.to(DEV), w.to(DEV)
    nl, nm = L.dstd_losses_workspace_bytes(), L.dstd_loss_workspace_bytes()
    wsl, wsm = b.new("losses workspace", nl, 0x4B), b.new("mpjpe workspace", nm, 0x4B)
    values, loss = b.f32("values", (2, 4), NAN_OUT), b.f32("loss", (1,), NAN_OUT)
    snap = b.freeze()
    g = cs[5:]
    _refused(L.dstd_ctg_fwd(x.data_ptr(), B, C, T, V, Tm.data_ptr(), A.data_ptr(), Af.data_ptr(), y.data_ptr(), ws.ptr,
                            n - 1, st), EWORKSPACE, b, snap, "dstd_ctg_fwd")
    _refused(L.dstd_ctg_bwd(x.data_ptr(), B, C, T, V, Tm.data_ptr(), A.data_ptr(), Af.data_ptr(), y.data_ptr(),
                            dx.data_ptr(), dTm.data_ptr(), dA.data_ptr(), ws.ptr, n - 1, st), EWORKSPACE, b, snap,
             "dstd_ctg_bwd")
    _refused(L.dstd_conv2d_fwd(xc.data_ptr(), Bc, cin, Hh, Ww, wc.data_ptr(), bc.data_ptr(), cout, *g, yc.data_ptr(),
                               wsc.ptr, nc - 1, st), EWORKSPACE, b, snap, "dstd_conv2d_fwd")
    _refused(L.dstd_conv2d_fwd(xc.data_ptr(), Bc, cin, Hh, Ww, wc.data_ptr(), bc.data_ptr(), cout, *g, yc.data_ptr(),
                               None, nc, st), EINVAL, b, snap, "dstd_conv2d_fwd without a workspace")  # as the backward
    _refused(L.dstd_conv2d_bwd(xc.data_ptr(), Bc, cin, Hh, Ww, wc.data_ptr(), cout, *g, dyc.data_ptr(), dxc.data_ptr(),
                               dwc.data_ptr(), dbc.data_ptr(), wsc.ptr, nc - 1, st), EWORKSPACE, b, snap,
             "dstd_conv2d_bwd")
    _refused(L.dstd_losses_fwd(_problems(preds, targets, maps), 2, ALL_TERMS, w.data_ptr(), values.data_ptr(), wsl.ptr,
                               nl - 1, st), EINVAL, b, snap, "dstd_losses_fwd")  # tests/test_loss_host.py pins EINVAL
    _refused(L.dstd_mpjpe_fwd(preds[0].data_ptr(), preds[1].data_ptr(), 10, loss.data_ptr(), wsm.ptr, nm - 1, st),
             EWORKSPACE, b, snap, "dstd_mpjpe_fwd")
    # the exact sizes straight after, on the same buffers
    native.check(L.dstd_ctg_fwd(x.data_ptr(), B, C, T, V, Tm.data_ptr(), A.data_ptr(), Af.data_ptr(), y.data_ptr(),
                                ws.ptr, n, st), "dstd_ctg_fwd")
    y64 = O.ctg(x.double().cpu(), {"T": Tm.double().cpu(), "A": A.double().cpu(), "A_fixed": Af.double().cpu()})
    assert rel(y, y64) < 1e-4
    native.check(L.dstd_conv2d_fwd(xc.data_ptr(), Bc, cin, Hh, Ww, wc.data_ptr(), bc.data_ptr(), cout, *g, yc.data_ptr(),
                                   wsc.ptr, nc, st), "dstd_conv2d_fwd")
    ref = torch.nn.functional.conv2d(xc.double().cpu(), wc.double().cpu(), bc.double().cpu(), stride=(sh, sw),
                                     padding=(ph, pw))
    assert rel(yc, ref) < 1e-5  # test_native_conv2d_strided_padded
    # the backwards accumulate: onto zeros, with y and dyc as the upstream gradients as in the refused calls
    dy = y.clone()
    for t in (dx, dTm, dA, dxc, dwc, dbc):
        t.zero_()
    native.check(L.dstd_ctg_bwd(x.data_ptr(), B, C, T, V, Tm.data_ptr(), A.data_ptr(), Af.data_ptr(), dy.data_ptr(),
                                dx.data_ptr(), dTm.data_ptr(), dA.data_ptr(), ws.ptr, n, st), "dstd_ctg_bwd")
    x64, Tm64, A64 = (t.double().cpu().requires_grad_(True) for t in (x, Tm, A))
    (O.ctg(x64, {"T": Tm64, "A": A64, "A_fixed": Af.double().cpu()}) * dy.double().cpu()).sum().backward()
    for k, t, r in (("dx", dx, x64), ("dTm", dTm, Tm64), ("dA", dA, A64)):
        assert rel(t, r.grad) < 1e-4, ("dstd_ctg_bwd", k, rel(t, r.grad))
    native.check(L.dstd_conv2d_bwd(xc.data_ptr(), Bc, cin, Hh, Ww, wc.data_ptr(), cout, *g, dyc.data_ptr(), dxc.data_ptr(),
                                   dwc.data_ptr(), dbc.data_ptr(), wsc.ptr, nc, st), "dstd_conv2d_bwd")
    xc64, wc64, bc64 = (t.double().cpu().requires_grad_(True) for t in (xc, wc, bc))
    (torch.nn.functional.conv2d(xc64, wc64, bc64, stride=(sh, sw), padding=(ph, pw)) * dyc.double().cpu()).sum().backward()
    for k, t, r in (("dx", dxc, xc64), ("dw", dwc, wc64), ("db", dbc, bc64)):
        assert rel(t, r.grad) < 1e-5, ("dstd_conv2d_bwd", k, rel(t, r.grad))
    native.check(L.dstd_mpjpe_fwd(preds[0].data_ptr(), preds[1].data_ptr(), 10, loss.data_ptr(), wsm.ptr, nm, st),
                 "dstd_mpjpe_fwd")
    pa, pb = (p.flatten()[:30].double().cpu().view(10, 3) for p in preds)
    assert abs(float(loss[0]) - float((pa - pb).norm(dim=1).mean())) < 1e-5  # test_mpjpe
    native.check(L.dstd_losses_fwd(_problems(preds, targets, maps), 2, ALL_TERMS, w.data_ptr(), values.data_ptr(),
                                   wsl.ptr, nl, st), "dstd_losses_fwd")
    for i, (_, step) in enumerate(maps):
        terms = loss_terms(preds[i].cpu(), _slice(targets.cpu(), preds[i].shape[1], step).contiguous(), w.cpu())
        for k, t in enumerate(TERMS):
            assert abs(float(values[i, k]) - float(terms[t])) < VALUE_TOL, (i, t)
    b.check()
