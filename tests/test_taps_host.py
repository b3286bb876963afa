"""Host-side checks of the tap entry points (include/dstd_gcn_taps.h,
forward_taps) and of the reference the GPU tests compare against (no GPU
needed)."""
import ctypes
import os
import re

import pytest
import torch

import taps_helper as H
from conftest import ROOT
import dstd_native as native
from model import DSTDGCB, Taps, get_model
from oracle import dstdgcn_oracle as O

EINVAL, ELIMIT = -1, -3  # include/dstd_gcn.h
H36M = dict(input_channels=6, input_time_frame=10, output_time_frame=25, st_gcnn_dropout=0.1,
            joints_to_consider=22, num_feature=64, num_layers=5, layout="h36m")


def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\*?(dstd_\w+)\s*\(", src, re.M)))


def test_library_exports_every_taps_header_symbol():
    L = native.lib()
    syms = header_symbols("dstd_gcn_taps.h")
    assert len(syms) == 4, syms
    for s in syms:
        assert hasattr(L, s), s
    assert set(syms) == set(native.TAPS_EXPORTS)
    assert [n for n, _ in native.BlockTaps._fields_] == ["adj_s", "adj_t", "x", "h"]
    assert ctypes.sizeof(native.BlockTaps) == 4 * ctypes.sizeof(ctypes.c_void_p)


def test_taps_need_no_more_workspace_than_the_forward():
    L = native.lib()
    assert L.dstd_block_taps_workspace_bytes(4, 64, 64, 35, 22) == L.dstd_block_workspace_bytes(4, 64, 64, 35, 22)
    assert L.dstd_model_taps_workspace_bytes(4, 35, 22, 64, 5) == L.dstd_model_workspace_bytes(4, 35, 22, 64, 5)


FAKE = 0x1000  # a non-null "device pointer" for calls that must return before they touch anything


def _fake(struct):
    """Every pointer member of a parameter struct non-null (never followed:
    the calls below are refused by their shape or flags)."""
    for name, typ in struct._fields_:
        if typ is ctypes.c_void_p:
            setattr(struct, name, FAKE)
        elif issubclass(typ, ctypes.Structure):
            _fake(getattr(struct, name))
        elif issubclass(typ, ctypes.Array):
            arr = getattr(struct, name)
            for i in range(len(arr)):
                if issubclass(typ._type_, ctypes.Structure):
                    _fake(arr[i])
                elif typ._type_ is ctypes.c_void_p:
                    arr[i] = FAKE
    return struct


def _block_params(cin, cout):
    p = _fake(native.BlockParams())
    p.cin, p.cout = cin, cout
    p.bn.eps = p.res_bn.eps = 1e-5
    return p


def _model_params(T, V, C=64, layers=1):
    p = _fake(native.ModelParams())
    p.T, p.V, p.num_layers, p.num_feature, p.in_channels = T, V, layers, C, 6
    p.st_in.cin, p.st_in.cout = 6, C
    p.st_out.cin, p.st_out.cout = C, 3
    for i in range(min(layers, native.MAX_LAYERS)):
        p.enc[i].cin = p.enc[i].cout = C
    return p


def test_block_fwd_taps_refuses_bad_arguments_without_gpu():
    L = native.lib()
    taps = native.BlockTaps()
    p = _block_params(64, 64)
    assert L.dstd_block_fwd_taps(None, FAKE, 2, 35, 22, FAKE, taps, FAKE, 1 << 30, None, 0) == EINVAL  # null params
    assert L.dstd_block_fwd_taps(p, FAKE, 2, 35, 22, FAKE, None, FAKE, 1 << 30, None, 0) == EINVAL  # null taps
    assert L.dstd_block_fwd_taps(p, None, 2, 35, 22, FAKE, taps, FAKE, 1 << 30, None, 0) == EINVAL  # null x
    # flags: DSTD_FWD_EXACT_FP32 (2) only -- every other bit, even one dstd_block_fwd_ex takes
    for bad in (1, 4, 8, 16, 32, 64, 2 | 8, 1 << 31):
        assert L.dstd_block_fwd_taps(p, FAKE, 2, 35, 22, FAKE, taps, FAKE, 1 << 30, None, bad) == EINVAL, bad
    assert L.dstd_block_fwd_taps(p, FAKE, 2, 1, 22, FAKE, taps, FAKE, 1 << 30, None, 0) == EINVAL  # T = 1
    assert L.dstd_block_fwd_taps(p, FAKE, 0, 35, 22, FAKE, taps, FAKE, 1 << 30, None, 0) == EINVAL  # B = 0
    for T, V, cin, cout in ((129, 22, 64, 64), (35, 33, 64, 64), (35, 22, 65, 64), (35, 22, 6, 65)):
        q = _block_params(cin, cout)
        for flags in (0, native.FWD_EXACT_FP32):
            assert L.dstd_block_fwd_taps(q, FAKE, 2, T, V, FAKE, taps, FAKE, 1 << 30, None, flags) == ELIMIT


def test_model_fwd_taps_refuses_bad_arguments_without_gpu():
    L = native.lib()
    taps = (native.BlockTaps * 3)()
    p = _model_params(35, 22)
    assert L.dstd_model_fwd_taps(None, FAKE, 2, FAKE, taps, FAKE, 1 << 30, None, 0) == EINVAL
    assert L.dstd_model_fwd_taps(p, FAKE, 2, FAKE, None, FAKE, 1 << 30, None, 0) == EINVAL
    assert L.dstd_model_fwd_taps(p, FAKE, 2, None, taps, FAKE, 1 << 30, None, 0) == EINVAL
    for bad in (1, 4, 8, 16, 32, 64, 2 | 1):  # 1: DSTD_FWD_REUSE_CONSTANTS is not for a tap call either
        assert L.dstd_model_fwd_taps(p, FAKE, 2, FAKE, taps, FAKE, 1 << 30, None, bad) == EINVAL, bad
    assert L.dstd_model_fwd_taps(_model_params(1, 22), FAKE, 2, FAKE, taps, FAKE, 1 << 30, None, 0) == EINVAL
    assert L.dstd_model_fwd_taps(_model_params(35, 22, layers=17), FAKE, 2, FAKE, taps, FAKE, 1 << 30, None, 0) == EINVAL
    for T, V, C in ((129, 22, 64), (35, 33, 64), (35, 22, 65)):
        assert L.dstd_model_fwd_taps(_model_params(T, V, C), FAKE, 2, FAKE, taps, FAKE, 1 << 30, None, 2) == ELIMIT


def test_forward_taps_refusals():
    m = get_model("dstdgcn", dstdgcn=H36M)
    blk = DSTDGCB(64, 64, 35, 22, "h36m")
    with pytest.raises(RuntimeError, match="eval"):
        m.train().forward_taps(torch.zeros(2, 35, 22, 3))
    with pytest.raises(RuntimeError, match="eval"):
        blk.train().forward_taps(torch.zeros(2, 64, 35, 22))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.eval().forward_taps(torch.zeros(2, 35, 22, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blk.eval().forward_taps(torch.zeros(2, 64, 35, 22))
    with pytest.raises(ValueError, match="unknown tap"):
        m.forward_taps(torch.zeros(2, 35, 22, 3), what=("adj",))
    with pytest.raises(ValueError, match="block 7"):
        m.forward_taps(torch.zeros(2, 35, 22, 3), blocks=[7])
    t = Taps()
    assert all(getattr(t, n) is None for n in native.TAP_NAMES)


# ---- the reference of the GPU tests -------------------------------------------
@pytest.mark.parametrize("T", [5, 12])
@pytest.mark.parametrize("V", [5, 22])
@pytest.mark.parametrize("mode", ["spatial", "temporal"])
def test_helper_restates_the_oracle(mode, V, T):
    """The helper's adjacency, contracted with conv1x1(conv_f) as O.dstdgc
    does, is O.dstdgc (fp64, 1e-12)."""
    g = torch.Generator().manual_seed(31 * T + V)
    ref_c = T if mode == "spatial" else V
    NA = V if mode == "spatial" else T
    cin, cout = 7, 5
    f64 = dict(generator=g, dtype=torch.float64)
    p = {"conv_f.weight": torch.randn(cout, cin, 1, 1, **f64), "conv_f.bias": torch.randn(cout, **f64),
         "conv_m1.weight": torch.randn(2, cin, 1, 1, **f64), "conv_m1.bias": torch.randn(2, **f64),
         "conv_m2.weight": torch.randn(2, cin, 1, 1, **f64), "conv_m2.bias": torch.randn(2, **f64),
         "conv_rm.weight": torch.randn(ref_c, 2 * ref_c, 1, 1, **f64), "conv_rm.bias": torch.randn(ref_c, **f64)}
    x = torch.randn(3, cin, T, V, **f64)
    A = torch.randn(1, NA, NA, **f64)
    alpha = torch.tensor(0.7, dtype=torch.float64)
    adj = H.dynamic_adj(x, p, A, alpha, mode)
    assert adj.shape == ((3, T, V, V) if mode == "spatial" else (3, V, T, T))
    xf = O.conv1x1(x, p["conv_f.weight"], p["conv_f.bias"])
    y = torch.einsum("nctv,ntvw->nctw" if mode == "spatial" else "nctv,nvtu->ncuv", xf, adj)
    assert H.rel(y, O.dstdgc(x, p, A, alpha, mode)) <= 1e-12


@pytest.mark.parametrize("name", ["fix-h36m", "syn-T12-B3", "blk-range"])
def test_oracle_walk_is_the_oracle(name):
    """oracle_taps / oracle_block_taps (the pieces the consistency checks are
    made of) reproduce O.dstdgcn / O.dstdgcb_forward."""
    c = H.case(name)
    if c.kind == "model":
        ref = O.dstdgcn(c.x, {k: v.numpy() for k, v in c.sd.items()}, c.num_layers)
    else:
        ref = O.dstdgcb_forward(c.x.numpy(), {k: v.numpy() for k, v in c.sd.items()})
    assert H.rel(c.y64, ref) <= 1e-12


@pytest.mark.parametrize("name", H.CASES)
def test_fp32_reference_error_is_half_the_gpu_bar(name):
    """The same formula in fp32 on the fp64 oracle's block inputs stays within
    half the bar the GPU taps are held to: the bar leaves room for an fp32
    evaluation of these adjacencies."""
    c = H.case(name)
    worst = 0.0
    for b, t in enumerate(c.taps64):
        a32_s, a32_t = H.block_adjacencies(t["x"], t["h"], c.block_sd(b), torch.float32)
        for i in range(2):
            worst = max(worst, H.rel(a32_s[:, i], t["adj_s"][:, i]))
        worst = max(worst, H.rel(a32_t, t["adj_t"]))
    print(f"{name}: fp32 helper vs fp64 helper, worst max|d| / max|adj64| = {worst:.2e}")
    assert worst <= H.TAP_BAR / 2


def test_range_case_shifts_the_planes():
    """blk-range: the bound the split kernels take a plane's range shift from
    reaches 2^14 for all three graphs, so sa > 0 and the decode has a shift to
    undo."""
    c = H.case("blk-range")
    for which in (0, 1, "t"):
        assert H.plane_bound(c.sd, which) >= 2 ** 14, which
    # ... while the fixture models' planes are unshifted
    f = H.case("fix-h36m")
    assert all(H.plane_bound(f.block_sd(b), w) < 2 ** 14 for b in range(7) for w in (0, 1, "t"))
