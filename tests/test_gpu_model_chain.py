"""The whole eval forward as one launch (k_model_chain, DSTD_FWD_SEPARATE_ENDS
off): one workgroup per sample runs conv_st_in, the encoder blocks and
conv_st_out of its sample in turn -- 1 launch instead of 3 (conv_st_in, the
encoder run, conv_st_out: DSTD_FWD_SEPARATE_ENDS) or num_layers + 2
(DSTD_FWD_SEPARATE_ENCODERS).  The same unit code in the same order as one
k_block_fused launch per block: every comparison here is torch.equal against
those two schedules, which test_gpu_enc_chain.py and the oracle tests of
test_gpu_parity.py cover.  A profiled call stays per block
(test_gpu_enc_chain.py::test_profiled_call_stays_per_block).
"""
import os
import re

import pytest
import torch

import dstd_native as native
from conftest import group, load_npz
from model import get_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# encoder blocks per one-launch forward: kModelChainMaxEnc of the native header
_HILO_H = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dstd-gcn_amd", "csrc", "dstd_hilo.h")
MAX_ENC = int(re.search(r"constexpr int kModelChainMaxEnc = (\d+);", open(_HILO_H).read()).group(1))


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


def expected_plans(layers):
    """(default, DSTD_FWD_SEPARATE_ENDS, DSTD_FWD_SEPARATE_ENCODERS) launch lists
    of a forward whose every block can be a whole-block launch: one MODEL launch
    for 1..MAX_ENC encoder blocks; conv_st_in, the encoder runs (at most 8 blocks
    each, a left-over single block on its own), conv_st_out; one BLOCK per block."""
    per_block = [(native.LAUNCH_BLOCK, b, 1) for b in range(layers + 2)]
    runs, b = per_block[:1], 1
    while b <= layers:
        n = min(8, layers + 1 - b)
        runs.append((native.LAUNCH_ENC_RUN, b, n) if n >= 2 else per_block[b])
        b += n
    runs.append(per_block[-1])
    return ([(native.LAUNCH_MODEL, 0, layers + 2)] if 1 <= layers <= MAX_ENC else runs), runs, per_block


def planned(m, x, flags):
    """dstd_model_fwd_schedule for m(x) with these flags on this device."""
    B, T, V, _ = x.shape
    return native.model_schedule(B, T, V, 64, len(m.encoders), flags)


def three(m, x, flags):
    """(one launch, conv_st_in + encoder run + conv_st_out, one launch per block) outputs of one input."""
    ys = [torch.empty_like(x) for _ in range(3)]
    want = expected_plans(len(m.encoders))
    for extra, w in zip((0, native.FWD_SEPARATE_ENDS, native.FWD_SEPARATE_ENCODERS), want):
        assert planned(m, x, flags | extra) == w, (extra, planned(m, x, flags | extra))
    if 1 <= len(m.encoders) <= MAX_ENC:  # else the default falls back to the runs
        assert want[0] != want[1] and want[0] != want[2]
    with torch.no_grad():
        for y, extra in zip(ys, (0, native.FWD_SEPARATE_ENDS, native.FWD_SEPARATE_ENCODERS)):
            m._forward_native(x, y, arith=flags | extra)
    torch.cuda.synchronize()
    return ys


@pytest.mark.parametrize("tag", ["h36m", "cmu", "3dpw"])
def test_model_chain_bit_identical(tag):
    """B=3 (the smallest ragged grid, fused schedule forced), B=16 with inputs
    x1000 (range-shifted operands, the direct tanh of phases 0 and 3) and
    B=256 (the default schedule at full occupancy)."""
    m, opts = load_model(tag)
    Tin = opts["input_time_frame"]
    T, V = Tin + opts["output_time_frame"], opts["joints_to_consider"]
    cases = [(synth(3, T, V, Tin, 31).to(DEV), native.FWD_FUSED_TEMPORAL),
             ((synth(16, T, V, Tin, 32) * 1000.0).to(DEV), native.FWD_FUSED_TEMPORAL),
             (synth(256, T, V, Tin, 33).to(DEV), 0)]
    for x, fl in cases:
        y0, y1, y2 = three(m, x, fl)
        assert torch.isfinite(y0).all()
        assert torch.equal(y0, y1), (tag, x.shape[0], "ends", float((y0 - y1).abs().max()))
        assert torch.equal(y0, y2), (tag, x.shape[0], "encoders", float((y0 - y2).abs().max()))


@pytest.mark.parametrize("layers", [0, 1, MAX_ENC, MAX_ENC + 1, 10])
def test_model_chain_length(layers):
    """num_layers 0 (no encoder block: falls back), 1 (the shortest one-launch
    forward), kModelChainMaxEnc (the longest), kModelChainMaxEnc + 1 (falls
    back to conv_st_in, one encoder run, conv_st_out) and 10 (conv_st_in, two
    runs, conv_st_out), random weights."""
    torch.manual_seed(140 + layers)
    opts = dict(input_channels=6, input_time_frame=10, output_time_frame=25, st_gcnn_dropout=0.0,
                joints_to_consider=22, num_feature=64, num_layers=layers, layout="h36m")
    m = get_model("dstdgcn", dstdgcn=opts).to(DEV).eval()
    x = synth(5, 35, 22, 10, 141).to(DEV)
    y0, y1, y2 = three(m, x, native.FWD_FUSED_TEMPORAL)
    assert torch.isfinite(y0).all()
    assert torch.equal(y0, y1), float((y0 - y1).abs().max())
    assert torch.equal(y0, y2), float((y0 - y2).abs().max())


def test_model_chain_repeatable():
    """The B=256 h36m forward 20 times in one process, two inputs in turn:
    every output equals the per-block schedule's for its input (a block that
    read a predecessor's stale activation, P/Q or plane buffer would show the
    other input's values)."""
    m, opts = load_model("h36m")
    Tin = opts["input_time_frame"]
    T = Tin + opts["output_time_frame"]
    xs = [synth(256, T, 22, Tin, 151).to(DEV), synth(256, T, 22, Tin, 152).to(DEV)]
    refs = [torch.empty_like(x) for x in xs]
    ys = [torch.empty_like(xs[0]) for _ in range(20)]
    with torch.no_grad():
        for x, r in zip(xs, refs):
            m._forward_native(x, r, arith=native.FWD_SEPARATE_ENCODERS)
        for i, y in enumerate(ys):
            m._forward_native(xs[i % 2], y, arith=0)
    torch.cuda.synchronize()
    assert all(torch.isfinite(r).all() for r in refs) and not torch.equal(refs[0], refs[1])
    for i, y in enumerate(ys):
        bad = int((y != refs[i % 2]).flatten(1).any(1).sum())
        assert torch.equal(y, refs[i % 2]), (i, bad)


def test_model_chain_staggered_workgroups():
    """B=805 h36m (more than three workgroups per CU, the last round ragged):
    workgroups start whenever a CU falls free, so one sample's conv_st_out runs
    while others are in their encoder blocks.  Anything a block keeps outside
    its own sample's slice of the workspace (conv_st_out's 3-channel h once lay
    across other samples' 64-channel activations) shows here."""
    m, opts = load_model("h36m")
    Tin = opts["input_time_frame"]
    x = synth(805, Tin + opts["output_time_frame"], 22, Tin, 161).to(DEV)
    y0, y1, y2 = three(m, x, 0)
    assert torch.isfinite(y0).all()
    assert torch.equal(y0, y1), int((y0 != y1).flatten(1).any(1).sum())
    assert torch.equal(y0, y2), int((y0 != y2).flatten(1).any(1).sum())


def test_model_chain_graph_replay():
    """DSTDGCN.graphed(x, frozen=True) at B=32 with the fused schedule forced:
    the captured forward (one kernel node) replays to the eager result for two
    inputs."""
    m, opts = load_model("h36m")
    m._dstd_fwd_flags = native.FWD_FUSED_TEMPORAL
    Tin = opts["input_time_frame"]
    T = Tin + opts["output_time_frame"]
    x1, x2 = synth(32, T, 22, Tin, 171).to(DEV), synth(32, T, 22, Tin, 172).to(DEV)
    assert planned(m, x1, m._dstd_fwd_flags) == [(native.LAUNCH_MODEL, 0, opts["num_layers"] + 2)]
    with torch.no_grad():
        run = m.graphed(x1, frozen=True)
        y1 = run(x1).clone()  # folds
        y2 = run(x2).clone()  # the frozen graph
        assert torch.equal(run(x1), y1)
        m._dstd_fwd_flags = native.FWD_FUSED_TEMPORAL | native.FWD_SEPARATE_ENCODERS
        assert torch.equal(y1, m(x1)) and torch.equal(y2, m(x2))
        m._dstd_fwd_flags = native.FWD_FUSED_TEMPORAL
        assert torch.equal(y2, m(x2))
