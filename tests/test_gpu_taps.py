"""MI355X: forward_taps (include/dstd_gcn_taps.h) -- the dynamic adjacencies
and block activations of an eval forward.

Cases (tests/taps_helper.py CASES), each in both GC arithmetics:
  fix-*      the four fixture models on their own inputs: split planes with
             SL = 24 (V = 22, 23) and 32 (V = 25), the T = 75 temporal planes;
             in exact fp32 rows padded 625 -> 628 (cmu) and 529 -> 532 (3dpw)
  syn-T*-B*  h36m-layout models, num_layers = 1, at T = 5, 12, 128: the generic
             kernels' fp32 rows (25 -> 28 at T = 5, two adjacency row groups at
             T = 128), B = 1 and 3
  blk-range  one DSTDGCB 64 -> 64 at (35, 22) with alpha_sm = alpha_tm = 3e4:
             planes stored under a range shift sa > 0

Bars: a tapped adjacency against the fp64 restatement of the oracle fed the
tapped x / h, and the taps against each other through the fp64 oracle pieces,
both max|d| / max|ref| <= 1e-4 (the project's per-op / per-block bar;
tests/test_taps_host.py shows an fp32 evaluation of the same adjacencies
sits at 1e-6..3e-6).  Everything else is bit equality.
"""
import copy
import functools

import pytest
import torch

import taps_helper as H
from model import DSTDGCN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARITH = ("split", "fp32")
NAMES = ("adj_s", "adj_t", "x", "h")


def on_gpu(c, arith):
    m = copy.deepcopy(c.module).to(DEV).eval()
    if isinstance(m, DSTDGCN):
        m.set_gc_arithmetic(arith)
    else:
        m.gc_arithmetic = arith
    return m


def call(m, x, blocks=None, what=NAMES):
    """forward_taps of a model or a block as (y, {block index: taps})."""
    if isinstance(m, DSTDGCN):
        return m.forward_taps(x, blocks=blocks, what=what)
    y, t = m.forward_taps(x, what=what)
    return y, {0: t}


@functools.lru_cache(maxsize=None)
def run(name, arith):
    """One case on the GPU: the plain forward, then forward_taps twice."""
    c = H.case(name)
    m = on_gpu(c, arith)
    x = c.x.to(DEV)
    with torch.no_grad():
        y_plain = m(x)
    y, taps = call(m, x)
    y2, taps2 = call(m, x)
    torch.cuda.synchronize()
    return {"m": m, "x": x, "y_plain": y_plain, "y": y, "taps": taps, "y2": y2, "taps2": taps2}


CASE_ARITH = [(n, a) for n in H.CASES for a in ARITH]
both = pytest.mark.parametrize("name,arith", CASE_ARITH, ids=[f"{n}-{a}" for n, a in CASE_ARITH])


@both
def test_output_is_the_forward(name, arith):
    """y of forward_taps is module(x) bit for bit; the taps are detached
    tensors of the documented shapes."""
    c, r = H.case(name), run(name, arith)
    assert torch.equal(r["y"], r["y_plain"])
    assert sorted(r["taps"]) == list(range(len(c.taps64)))
    for b, t in r["taps"].items():
        for n in NAMES:
            got = getattr(t, n)
            assert tuple(got.shape) == tuple(c.taps64[b][n].shape), (b, n)
            assert got.dtype == torch.float32 and got.is_contiguous() and not got.requires_grad
            assert bool(torch.isfinite(got).all()), (b, n)


@both
def test_adjacencies_against_the_fp64_restatement(name, arith):
    c, r = H.case(name), run(name, arith)
    worst = 0.0
    for b, t in r["taps"].items():
        a_s, a_t = H.block_adjacencies(t.x, t.h, c.block_sd(b))
        errs = [H.rel(t.adj_s[:, i], a_s[:, i]) for i in range(2)] + [H.rel(t.adj_t, a_t)]
        print(f"{name} {arith} block {b}: adj_s {errs[0]:.2e} {errs[1]:.2e} adj_t {errs[2]:.2e}")
        worst = max(worst, *errs)
    assert worst <= H.TAP_BAR, worst


@both
def test_taps_are_consistent_with_each_other(name, arith):
    """In fp64 with the oracle's conv1x1 / batchnorm / prelu: x and adj_s give
    h; h and adj_t, then what follows the block in the model, give the next
    block's x (the last block: y)."""
    c, r = H.case(name), run(name, arith)
    sd = H.cast_sd(c.sd, torch.float64)
    x_model = c.x.double()
    nb = len(r["taps"])
    worst = 0.0
    for b in range(nb):
        t, p = r["taps"][b], c.block_sd(b)
        x, h = t.x.double().cpu(), t.h.double().cpu()
        e_h = H.rel(h, H.spatial_half(x, t.adj_s.double().cpu(), p))
        out = H.temporal_half(h, t.adj_t.double().cpu(), p)
        if c.kind == "model":
            out = H.after_block(b, out, x, x_model, sd, c.num_layers)
        nxt = r["taps"][b + 1].x if b + 1 < nb else r["y"]
        e_o = H.rel(nxt, out)
        print(f"{name} {arith} block {b}: h {e_h:.2e} next {e_o:.2e}")
        worst = max(worst, e_h, e_o)
    assert worst <= H.TAP_BAR, worst


@both
def test_block0_input_is_the_model_input(name, arith):
    c, r = H.case(name), run(name, arith)
    x0 = r["taps"][0].x
    if c.kind == "model":
        assert torch.equal(x0, H.model_input6(r["x"]).contiguous())
    else:
        assert torch.equal(x0, r["x"])


@both
def test_restricted_call(name, arith):
    """blocks / what restrict what is returned; what is returned equals the
    all-taps call's."""
    c, r = H.case(name), run(name, arith)
    nb = len(r["taps"])
    blocks = [nb - 1] if nb == 1 else [1, nb - 1]
    for what in (("adj_t", "h"), ("adj_s",), ("x",)):
        y, taps = call(r["m"], r["x"], blocks=blocks if c.kind == "model" else None, what=what)
        assert torch.equal(y, r["y"])
        assert sorted(taps) == blocks
        for b in blocks:
            for n in NAMES:
                got = getattr(taps[b], n)
                if n in what:
                    assert torch.equal(got, getattr(r["taps"][b], n)), (b, n)
                else:
                    assert got is None, (b, n)


@both
def test_two_calls_are_equal(name, arith):
    r = run(name, arith)
    assert torch.equal(r["y"], r["y2"])
    for b, t in r["taps"].items():
        for n in NAMES:
            assert torch.equal(getattr(t, n), getattr(r["taps2"][b], n)), (b, n)


def test_plain_forward_after_a_tap_call():
    """A tap call leaves the workspace unclaimed: the next plain forward folds
    its constants again and returns what it returned before."""
    r = run("fix-h36m", "split")
    with torch.no_grad():
        assert torch.equal(r["m"](r["x"]), r["y_plain"])
        assert torch.equal(r["m"](r["x"]), r["y_plain"])


def test_full_batch_against_the_fused_schedule():
    """B = the device's compute units: the default forward runs one workgroup
    per sample (fused launches, adjacencies in LDS), the tap call the
    unit-parallel schedule -- same y bit for bit, and a sample's adjacency is
    the one of its own B = 1 run."""
    c = H.case("fix-h36m")
    m = on_gpu(c, "split")
    B = torch.cuda.get_device_properties(DEV).multi_processor_count
    x = H.synth_input(B, 35, 22, 10, 77).to(DEV)
    with torch.no_grad():
        y_plain = m(x)
    y, taps = m.forward_taps(x, blocks=[3], what=("adj_t",))
    assert torch.equal(y, y_plain)
    assert sorted(taps) == [3] and tuple(taps[3].adj_t.shape) == (B, 22, 35, 35)
    assert taps[3].adj_s is None and taps[3].x is None and taps[3].h is None
    for n in (0, B - 1):
        y1, t1 = m.forward_taps(x[n:n + 1], blocks=[3], what=("adj_t",))
        assert torch.equal(y1[0], y[n])
        assert torch.equal(t1[3].adj_t[0], taps[3].adj_t[n]), n
