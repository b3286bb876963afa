"""The encoder run as one launch (k_enc_chain, DSTD_FWD_SEPARATE_ENCODERS off):
one workgroup per sample loops over the consecutive encoder blocks, so the
eval forward is conv_st_in, the encoder run, conv_st_out -- 3 launches instead
of num_layers + 2.  The same unit code in the same order as one k_block_fused
launch per block: every comparison here is torch.equal against the per-block
schedule (DSTD_FWD_SEPARATE_ENCODERS), which the oracle tests of
test_gpu_parity.py cover.  What a kernel boundary gave the per-block schedule
(the previous block's stores complete, its LDS reads over) the run provides
itself at every block boundary; a missing guarantee shows as samples that
differ from run to run at full occupancy (B = 256), hence the repeat test.
"""
import ctypes

import pytest
import torch

import dstd_native as native
from conftest import group, load_npz
from model import get_model
from test_gpu_model_chain import expected_plans, planned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def synth(B, T, V, Tin, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, 3, generator=g)
    x[:, Tin:] = x[:, Tin - 1:Tin]
    return x


def load_model(tag):
    d = load_npz(f"model_{tag}.npz")
    opts = {k[4:]: d[k].item() for k in d.files if k.startswith("opt/")}
    m = get_model("dstdgcn", dstdgcn=opts)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in group(d, "sd/").items()})
    return m.to(DEV).eval(), opts


def both(m, x, flags):
    """(default schedule, one launch per encoder block) outputs of one input."""
    y0, y1 = torch.empty_like(x), torch.empty_like(x)
    # the two calls run different launches: blocks sharing a launch (the whole
    # forward for up to kModelChainMaxEnc encoder blocks, else the encoder runs)
    # against one BLOCK per block
    shared, _, per_block = expected_plans(len(m.encoders))
    assert planned(m, x, flags) == shared and shared != per_block
    assert planned(m, x, flags | native.FWD_SEPARATE_ENCODERS) == per_block
    with torch.no_grad():
        m._forward_native(x, y0, arith=flags)
        m._forward_native(x, y1, arith=flags | native.FWD_SEPARATE_ENCODERS)
    torch.cuda.synchronize()
    return y0, y1


@pytest.mark.parametrize("tag", ["h36m", "cmu", "3dpw"])
def test_enc_chain_bit_identical(tag):
    """B=3 (the smallest ragged grid, fused schedule forced), B=16 with inputs
    x1000 (range-shifted operands, the direct tanh of phase 3) and B=256 (the
    default schedule at full occupancy)."""
    m, opts = load_model(tag)
    Tin = opts["input_time_frame"]
    T, V = Tin + opts["output_time_frame"], opts["joints_to_consider"]
    cases = [(synth(3, T, V, Tin, 31).to(DEV), native.FWD_FUSED_TEMPORAL),
             ((synth(16, T, V, Tin, 32) * 1000.0).to(DEV), native.FWD_FUSED_TEMPORAL),
             (synth(256, T, V, Tin, 33).to(DEV), 0)]
    for x, fl in cases:
        y0, y1 = both(m, x, fl)
        assert torch.isfinite(y0).all()
        assert torch.equal(y0, y1), (tag, x.shape[0], float((y0 - y1).abs().max()))


@pytest.mark.parametrize("layers", [1, 2, 10])
def test_enc_chain_length(layers):
    """num_layers 1 and 2 (the blocks share the one whole-forward launch) and
    10 (more than one launch holds: a run of 8, then a run of 2), random
    weights; both() checks these plans."""
    torch.manual_seed(40 + layers)
    opts = dict(input_channels=6, input_time_frame=10, output_time_frame=25, st_gcnn_dropout=0.0,
                joints_to_consider=22, num_feature=64, num_layers=layers, layout="h36m")
    m = get_model("dstdgcn", dstdgcn=opts).to(DEV).eval()
    x = synth(5, 35, 22, 10, 41).to(DEV)
    y0, y1 = both(m, x, native.FWD_FUSED_TEMPORAL)
    assert torch.isfinite(y0).all()
    assert torch.equal(y0, y1), float((y0 - y1).abs().max())


def test_enc_chain_repeatable_full_batch():
    """The B=256 h36m forward 20 times in one process on one input: every
    output equals the first and the per-block schedule's (round 6's one-launch
    model gave 13-57 wrong samples, another count each run)."""
    m, opts = load_model("h36m")
    Tin = opts["input_time_frame"]
    x = synth(256, Tin + opts["output_time_frame"], 22, Tin, 51).to(DEV)
    ref = torch.empty_like(x)
    ys = [torch.empty_like(x) for _ in range(20)]
    with torch.no_grad():
        m._forward_native(x, ref, arith=native.FWD_SEPARATE_ENCODERS)
        for y in ys:
            m._forward_native(x, y, arith=0)
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    for i, y in enumerate(ys):
        bad = int((y != ref).flatten(1).any(1).sum())
        assert torch.equal(y, ref), (i, bad)


def test_profiled_call_stays_per_block():
    """A call that carries a profile runs one launch per block (its event
    brackets are per block): one KIND_BLOCK bracket per block, the same output."""
    m, opts = load_model("h36m")
    Tin = opts["input_time_frame"]
    x = synth(256, Tin + opts["output_time_frame"], 22, Tin, 61).to(DEV)
    L = native.lib()
    pairs = 64
    events = (ctypes.c_void_p * (2 * pairs))()
    native.check(L.dstd_events_create(2 * pairs, events), "dstd_events_create")
    try:
        kinds, block = (ctypes.c_int * pairs)(), (ctypes.c_int * pairs)()
        prof = native.Profile(1 << native.KIND_BLOCK, pairs, 0, events, kinds, block, -1)
        y0, y1 = torch.empty_like(x), torch.empty_like(x)
        with torch.no_grad():
            m._forward_native(x, y0)
            m._forward_native(x, y1, ctypes.byref(prof))
        torch.cuda.synchronize()
        nb = opts["num_layers"] + 2
        assert prof.count == nb
        assert [kinds[i] for i in range(nb)] == [native.KIND_BLOCK] * nb
        assert [block[i] for i in range(nb)] == list(range(nb))
        assert torch.equal(y0, y1)
    finally:
        L.dstd_events_destroy(2 * pairs, events)


@pytest.mark.parametrize("flags", [native.FWD_FUSED_TEMPORAL, native.FWD_FUSED_TEMPORAL | native.FWD_SEPARATE_BLOCK,
                                   native.FWD_FUSED_TEMPORAL | native.FWD_SEPARATE_ADJ, 0, native.FWD_EXACT_FP32])
def test_profiled_launches_follow_the_plan(flags):
    """What a forward launches is what dstd_model_fwd_schedule plans: with every
    family bracketed, the recorded (kind, block) sequence without the
    parameter-preparation brackets is the plan of the profiled call, for every
    schedule a profile can see (whole blocks; spatial + fused temporal; planes
    in launches of their own; unit-parallel split; generic fp32 with its PREP).
    B=3: the smallest ragged grid."""
    m, opts = load_model("h36m")
    Tin = opts["input_time_frame"]
    x = synth(3, Tin + opts["output_time_frame"], 22, Tin, 81).to(DEV)
    family = {native.LAUNCH_PREP: native.KIND_PREP, native.LAUNCH_ADJ_S: native.KIND_ADJ_S,
              native.LAUNCH_SPATIAL: native.KIND_SPATIAL, native.LAUNCH_ADJ_T: native.KIND_ADJ_T,
              native.LAUNCH_TEMPORAL: native.KIND_TEMPORAL, native.LAUNCH_TEMPORAL_FUSED: native.KIND_TEMPORAL,
              native.LAUNCH_BLOCK: native.KIND_BLOCK}
    B, T, V, _ = x.shape
    plan = native.model_schedule(B, T, V, 64, opts["num_layers"], flags, profiled=True)
    assert all(n == (0 if k == native.LAUNCH_PREP else 1) for k, _, n in plan)
    want = [(family[k], b) for k, b, _ in plan]
    L = native.lib()
    pairs = 64
    events = (ctypes.c_void_p * (2 * pairs))()
    native.check(L.dstd_events_create(2 * pairs, events), "dstd_events_create")
    try:
        kinds, block = (ctypes.c_int * pairs)(), (ctypes.c_int * pairs)()
        prof = native.Profile((1 << len(native.KIND_NAMES)) - 1, pairs, 0, events, kinds, block, -1)
        y = torch.empty_like(x)
        with torch.no_grad():
            m._forward_native(x, y, ctypes.byref(prof), arith=flags)
        torch.cuda.synchronize()
        assert prof.count < pairs
        got = [(kinds[i], block[i]) for i in range(prof.count) if kinds[i] != native.KIND_FOLD]
        assert got == want
        assert torch.isfinite(y).all()
    finally:
        L.dstd_events_destroy(2 * pairs, events)


def test_enc_chain_graph_replay():
    """DSTDGCN.graphed(x, frozen=True) at B=32 with the fused schedule forced:
    the captured forward (DSTD_FWD_SEPARATE_ENDS: conv_st_in, the encoder run
    as one node, conv_st_out) replays to the eager result."""
    m, opts = load_model("h36m")
    chained = native.FWD_FUSED_TEMPORAL | native.FWD_SEPARATE_ENDS
    m._dstd_fwd_flags = chained
    Tin = opts["input_time_frame"]
    T = Tin + opts["output_time_frame"]
    x1, x2 = synth(32, T, 22, Tin, 71).to(DEV), synth(32, T, 22, Tin, 72).to(DEV)
    nl = opts["num_layers"]
    assert planned(m, x1, chained) == [(native.LAUNCH_BLOCK, 0, 1), (native.LAUNCH_ENC_RUN, 1, nl),
                                       (native.LAUNCH_BLOCK, nl + 1, 1)]
    with torch.no_grad():
        run = m.graphed(x1, frozen=True)
        y1 = run(x1).clone()  # folds
        y2 = run(x2).clone()  # the frozen graph
        assert torch.equal(run(x1), y1)
        m._dstd_fwd_flags = native.FWD_FUSED_TEMPORAL | native.FWD_SEPARATE_ENCODERS
        assert torch.equal(y1, m(x1)) and torch.equal(y2, m(x2))
        m._dstd_fwd_flags = chained
        assert torch.equal(y2, m(x2))
