"""Cases at the edges of the supported shape envelope (B >= 1, 2 <= T <= 128,
1 <= V <= 32, 1 <= cin, cout <= 64, 1 <= red_channels <= 8), shared by
tests/test_gpu_envelope.py (the kernels against the fp64 oracle) and
tests/test_envelope_host.py (the fp32 oracle against the fp64 one on the same
inputs, and the arithmetic of the coverage claims).

Every op case names the dispatch branch it is there for.  The builders are
deterministic per case; references and error measures live here so that both
tests normalise every tensor the same way.
"""
import collections
import functools

import torch

from model import DSTDGC, DSTDGCB
from oracle import dstdgcn_oracle as O
from test_gpu_train import randomise

OpCase = collections.namedtuple("OpCase", "mode cin cout T V red B")
BlockCase = collections.namedtuple("BlockCase", "cin cout layout T V B")

OP_BAR = 1e-4  # tests/test_gpu_parity.py, tests/test_gpu_train.py: per op
BLOCK_EVAL_BAR = 1e-4  # tests/test_gpu_parity.py: per block
BLOCK_TRAIN_BAR = 2e-4  # tests/test_gpu_train.py: train-mode BN subtracts two O(1) means

OP_CASES = []
WHY = {}


def _add(why, mode, cin, cout, T, V, red=2, B=2):
    c = OpCase(mode, cin, cout, T, V, red, B)
    if c in WHY:  # one shape serving several targets
        WHY[c] += "; " + why
        return
    OP_CASES.append(c)
    WHY[c] = why


# ---- corners of the envelope, widest and narrowest channels ----------------
for _mode in ("spatial", "temporal"):
    for _T, _V in ((2, 1), (2, 32), (128, 1), (128, 32)):
        _add(f"corner T={_T} V={_V}, full channels", _mode, 64, 64, _T, _V, B=2)
        _add(f"corner T={_T} V={_V}, one channel (M=1, cin=1 transpose)", _mode, 1, 1, _T, _V, B=1)

# ---- aggregation column fragments JF = cdiv(NN, 16), pad / no-pad NN --------
_add("spatial JF=1 with pad (V=15, V%4=3)", "spatial", 24, 40, 20, 15, B=3)
_add("spatial JF=1 no pad (V=16, V%4=0: agg_split's 4-frame branch)", "spatial", 24, 40, 20, 16, B=3)
_add("spatial JF=2, first column past one fragment (V=17)", "spatial", 24, 40, 20, 17, B=3)
_add("spatial JF=2 with pad (V=31)", "spatial", 24, 40, 20, 31, B=3)
_add("spatial JF=2 no pad, V=32: two full column tiles", "spatial", 24, 40, 20, 32, B=3)
_add("spatial V%4=0 at odd T: T*V%4=0 keeps the 16-byte vector path", "spatial", 24, 40, 21, 16, B=3)
for _V, _cin, _cout in ((5, 20, 24), (16, 32, 48)):
    _add(f"temporal JF=1 with pad (T=15), V={_V}", "temporal", _cin, _cout, 15, _V, B=3)
    _add(f"temporal JF=1 no pad (T=16), V={_V}", "temporal", _cin, _cout, 16, _V, B=3)
    _add(f"temporal JF=2 (T=17), V={_V}", "temporal", _cin, _cout, 17, _V, B=3)
    _add(f"temporal JF=3 no pad (T=48), V={_V}", "temporal", _cin, _cout, 48, _V, B=2)
    _add(f"temporal JF=4 with pad (T=49, pitch 80), V={_V}", "temporal", _cin, _cout, 49, _V, B=2)
    _add(f"temporal JF=4 with pad (T=63), V={_V}", "temporal", _cin, _cout, 63, _V, B=2)
    _add(f"temporal JF=4 no pad, T=64: the last slab shape (kAggMaxNN), V={_V}", "temporal", _cin, _cout, 64, _V, B=2)
    _add(f"temporal T=65: the first strided-GEMM fallback shape, V={_V}", "temporal", _cin, _cout, 65, _V, B=2)

# ---- temporal backward whose 16-channel slab does not fit LDS: dF on the
# channel-chunk kernel, dD on the a-chunk kernel (agg_bwd's two-launch path) --
_add("two-launch temporal backward, channel tail cout%4=1 (k_agg dD: whole groups of 4 + tail)",
     "temporal", 13, 17, 49, 16, B=2)

# ---- eval adjacency row tiles RT = cdiv(T, 16) -------------------------------
for _T, _why in ((48, "RT=3 full"), (64, "RT=4 single group, full"), (65, "RT=5"), (112, "RT=7: last single group"),
                 (113, "RT=8: first two-group shape at V=22"), (127, "RT=8 with a row tail")):
    _add(f"k_adj spatial T={_T} V=22: {_why}", "spatial", 32, 32, _T, 22, B=2)
for _T in (120, 128):
    for _V in (4, 8, 9):
        _add(f"k_adj spatial T={_T} V={_V}: RT=8 single group and its LDS boundary", "spatial", 8, 12, _T, _V, B=2)

# ---- channel tails: ks_for(cin), M=1, C % 4, cout < 16 ------------------------
for _cin, _cout in ((1, 1), (4, 5), (9, 16), (13, 17), (16, 15), (63, 1), (64, 63)):
    _add(f"channel tail cin={_cin} cout={_cout}, spatial", "spatial", _cin, _cout, 20, 17, B=3)
    _add(f"channel tail cin={_cin} cout={_cout}, temporal", "temporal", _cin, _cout, 18, 11, B=3)

# ---- red channels against kCsMax: backward-data K = cout + 2 red ------------
for _mode in ("spatial", "temporal"):
    for _red in (3, 8):
        for _cin in (64, 20):
            _add(f"red={_red}: K={64 + 2 * _red} (KS=20{', K = kCsMax' if _red == 8 else ''}), cin={_cin}",
                 _mode, _cin, 64, 35, 22, red=_red, B=2)

# ---- k_temporal_wave<T>: compile-time T, runtime V ---------------------------
for _T in (35, 40, 75):
    for _V in (1, 32):
        for _B in (1, 2):
            _add(f"temporal wave T={_T} at V={_V}, B*V={_B * _V} units", "temporal", 64, 64, _T, _V, B=_B)
_add("temporal 3->3 wave kernel at V=32", "temporal", 3, 3, 35, 32, B=2)

# ---- below the streaming GEMM's width: T*V < 16 -----------------------------
for _mode in ("spatial", "temporal"):
    _add("T*V=6 < 16: off the streaming conv path", _mode, 6, 5, 3, 2, B=3)
    _add("T*V=10 < 16 at full channels", _mode, 64, 64, 2, 5, B=2)

T_BLOCK = (2, 16, 17, 64, 65, 113)
_BLOCK_CH = ((64, 64, "h36m", 22), (6, 64, "cmu", 25), (64, 3, "3dpw", 23))
BLOCK_EVAL_CASES = [BlockCase(ci, co, lay, T, V, 2) for T in T_BLOCK for ci, co, lay, V in _BLOCK_CH]
BLOCK_TRAIN_CASES = [BlockCase(ci, co, lay, T, V, B) for T in T_BLOCK for ci, co, lay, V in _BLOCK_CH for B in (1, 4)]

# ---- train-mode BatchNorm apply paths (bn_path, csrc/dstd_train.hip) -----------
# The smallest blocks whose two BatchNorms (C = 64) put more than one sample in
# an apply workgroup (ns > 1: C * B / ns >= 1024), by float4 items (T*V % 4 == 0)
# and by elements; the expected dstd_debug_bn_last() fields ride along.
BN_FLAT, BN_MERGED_VEC, BN_MERGED_SCALAR = 0, 1, 2
BN_APPLY_CASES = [
    BlockCase(64, 64, "h36m", 4, 22, 32),  # 44 items: one clamped batch, k in {0, 1}
    BlockCase(64, 64, "h36m", 4, 22, 64),  # 88 items, all four k
    BlockCase(64, 64, "h36m", 26, 22, 64),  # 572 items: a second batch whose second item is past the end
    BlockCase(6, 64, "cmu", 3, 25, 32),  # T*V = 75 odd, with the residual BatchNorm
    BlockCase(6, 64, "cmu", 3, 25, 64),  # the same at ns 4
]
BN_APPLY_EXPECT = dict(zip(BN_APPLY_CASES, (  # (path, ns, splits)
    (BN_MERGED_VEC, 2, 2), (BN_MERGED_VEC, 4, 4), (BN_MERGED_VEC, 4, 16),
    (BN_MERGED_SCALAR, 2, 2), (BN_MERGED_SCALAR, 4, 3))))


def bn_path(B, C, T, V, groups=1, aligned=True):
    """(path, ns, splits) of a train-mode BatchNorm: the arithmetic of bn_path,
    bn_sep, bn_apply_samples and bn_splits (csrc/dstd_train.hip)."""
    total, vec, Bg = B * C * T * V, (T * V) % 4 == 0 and aligned, B // groups
    splits = max(1, min(16, cdiv(Bg * T, 64)))
    if total >= 1 << 24 and vec and total < 1 << 31:
        return BN_FLAT, 0, splits
    ns = next((n for n in (4, 2) if Bg % n == 0 and C * (B // n) >= 1024), 1)
    return (BN_MERGED_VEC if vec and ns <= 4 else BN_MERGED_SCALAR), ns, splits


def bn_code(path, ns, splits):
    return path | ns << 4 | splits << 8


# Cases whose default draw is ill-conditioned in fp32 (tests/test_envelope_host.py
# measures it): another seed (salt) or input scale, never another shape.
#  * temporal 64 -> 64 at (T, V) = (2, 1): conv_rm is [1 x 2] over a tanh that
#    64-channel P - Q saturates; the conv_m1 / conv_m2 gradients are then the
#    difference of near-equal terms (fp32 oracle 3.5e-4 of their own max);
#    half-scale inputs leave the tanh unsaturated
#  * train-mode blocks at T = 2, B = 1: each BatchNorm channel sees two values,
#    x_hat = +-1 up to eps / var, and the gradient reaching everything before
#    the BatchNorm is a cancelling difference amplified by 1 / sigma of the
#    narrowest channel; over 80 draws per case the fp32 oracle's worst tensor
#    ranges over three decades (5e-6 .. 1e-2 in the bar's unit, median 1e-3).
#    The draws below have no narrow channel; two of them also shrink the
#    input (x 0.01, x 0.1), which brings the batch variance of the BatchNorm
#    inputs towards eps = 1e-5 so that less of the difference cancels: the
#    conditioning changes through the scale as well as through the draw.
#  * other train-mode blocks whose default draw left the fp32 oracle above
#    4e-5 of the bar's unit (the bias of a conv feeding a BatchNorm, alpha_sm:
#    sums that cancel), up to 1.06e-4 depending on the summation order (CPU
#    thread count): another seed, same scale.
# fp32-oracle worst tensor of each block case below, the larger of 1 and 8
# CPU threads, in TUNE order: 5e-6, 2.8e-5, 2.6e-5, 1.5e-5, 1.4e-6, 7.4e-6,
# 1.9e-5, 9.5e-6, 1.4e-5, 1.7e-5 (half bar 1e-4; every other case <= 4e-5).
# The two CMU cases of BN_APPLY_CASES: 4.3e-5 and 5.1e-5 at salt 0, 2.6e-5 and
# 3.9e-5 at salt 3 (the h36m ones 2.0e-6, 4.1e-6, 3.5e-6 as drawn).
TUNE = {
    OpCase("temporal", 64, 64, 2, 1, 2, 2): dict(salt=0, x_scale=0.5),
    BlockCase(64, 64, "h36m", 2, 22, 1): dict(salt=22, x_scale=0.01),
    BlockCase(6, 64, "cmu", 2, 25, 1): dict(salt=160, x_scale=0.1),
    BlockCase(64, 3, "3dpw", 2, 23, 1): dict(salt=46, x_scale=1.0),
    BlockCase(6, 64, "cmu", 2, 25, 4): dict(salt=27),
    BlockCase(64, 64, "h36m", 17, 22, 4): dict(salt=1),
    BlockCase(6, 64, "cmu", 64, 25, 1): dict(salt=15),
    BlockCase(6, 64, "cmu", 64, 25, 4): dict(salt=22),
    BlockCase(64, 3, "3dpw", 64, 23, 1): dict(salt=1),
    BlockCase(6, 64, "cmu", 65, 25, 4): dict(salt=2),
    BlockCase(6, 64, "cmu", 113, 25, 4): dict(salt=16),
    BlockCase(6, 64, "cmu", 3, 25, 32): dict(salt=3),
    BlockCase(6, 64, "cmu", 3, 25, 64): dict(salt=3),
}


def _tune(c):
    t = TUNE.get(c, {})
    return t.get("salt", 0), t.get("x_scale", 1.0)


def case_id(c):
    if isinstance(c, OpCase):
        return f"{c.mode[0]}-c{c.cin}x{c.cout}-T{c.T}-V{c.V}-r{c.red}-B{c.B}"
    return f"c{c.cin}x{c.cout}-{c.layout}-T{c.T}-B{c.B}"


def cdiv(a, b):
    return (a + b - 1) // b


def nn_of(c):
    """The aggregated dimension of an op case: V (spatial) or T (temporal)."""
    return c.V if c.mode == "spatial" else c.T


def rup(a, b):
    return cdiv(a, b) * b


def temporal_bwd_two_launch(c):
    """Whether a temporal op's aggregation backward leaves the channel-chunk
    kernel for the two-launch path: the arithmetic of agg_bwd / agg_tile
    (csrc/dstd_train.hip) -- a 2 x 16-channel slab of pitch T*V (raised to
    4 mod 64) plus one [RK][P] adjacency tile per wave (4 waves) against 160 KB."""
    if c.mode != "temporal" or c.T > 64:
        return False
    qp = c.T * c.V
    while qp & 63 != 4:
        qp += 1
    jf = cdiv(c.T, 16)
    rk, p = rup(c.T, 4), 16 * (jf if jf & 1 else jf + 1)
    return 4 * (2 * 16 * qp + 4 * rk * p) > 160 * 1024


def case_seed(c):
    h = 0
    for v in (c.mode == "temporal", c.cin, c.cout, c.T, c.V, c.red, c.B):
        h = h * 131 + int(v)
    return h % (2 ** 31 - 1)


# ---- single ops ------------------------------------------------------------
def build_op(c):
    """(module on the CPU, x, A, alpha, upstream gradient w) of an op case:
    kaiming conv weights under the case's seed, the rest as randomise() of
    tests/test_gpu_train.py, A = 0.3 randn, alpha = 0.7."""
    salt, x_scale = _tune(c)
    seed = case_seed(c) + 7919 * salt
    torch.manual_seed(seed)
    ref_c, kpt = (c.T, c.V) if c.mode == "spatial" else (c.V, c.T)
    op = DSTDGC(c.cin, c.cout, ref_c, kpt, red_channels=c.red, mode=c.mode)
    randomise(op, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    NN = nn_of(c)
    x = x_scale * torch.randn(c.B, c.cin, c.T, c.V, generator=g)
    A = 0.3 * torch.randn(1, NN, NN, generator=g)
    alpha = torch.tensor([0.7])
    w = torch.randn(c.B, c.cout, c.T, c.V, generator=g)
    return op, x, A, alpha, w


def op_reference(c, dtype=torch.float64, built=None):
    """Oracle outputs and gradients of an op case in ``dtype``: {"y", "dx",
    "dA", "dalpha", <parameter name>: gradient}."""
    op, x, A, alpha, w = built if built is not None else build_op(c)
    sd = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in op.state_dict().items()}
    xr, Ar, ar = (t.detach().clone().to(dtype).requires_grad_(True) for t in (x, A, alpha))
    y = O.dstdgc(xr, sd, Ar, ar.reshape(()), c.mode)
    (y * w.to(dtype)).sum().backward()
    out = {"y": y.detach(), "dx": xr.grad, "dA": Ar.grad, "dalpha": ar.grad}
    out.update({k: v.grad for k, v in sd.items()})
    return out


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def op_errors(got, ref):
    """Per tensor: max |got - ref| / max |ref| (the per-op normalisation of
    tests/test_gpu_train.py)."""
    assert set(got) == set(ref), set(got) ^ set(ref)
    return {k: rel(got[k], ref[k]) for k in ref}


@functools.lru_cache(maxsize=None)
def op_reference64(c):
    return op_reference(c)


# ---- blocks, eval mode (the recipe of test_dstdgcb_generic_T30) -------------
def build_block_eval(c):
    torch.manual_seed(c.cin + c.cout + 7 * c.T)
    blk = DSTDGCB(c.cin, c.cout, c.T, c.V, c.layout)
    with torch.no_grad():
        blk.alpha_sm.fill_(0.6)
        blk.alpha_tm.fill_(0.4)
        blk.W_s.copy_(0.2 * torch.randn(blk.W_s.shape))
        blk.R_t.copy_(0.1 * torch.randn(blk.R_t.shape))
        for mod in blk.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape))
                mod.running_var.uniform_(0.5, 2.0)
                mod.weight.uniform_(0.8, 1.2)
            if isinstance(mod, torch.nn.Conv2d):
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape))
    x = torch.randn(c.B, c.cin, c.T, c.V)
    return blk, x


def block_eval_reference(c, dtype=torch.float64, built=None):
    blk, x = built if built is not None else build_block_eval(c)
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    return O.dstdgcb_forward(x, sd, dtype=dtype)


# ---- blocks, train mode (the recipe of test_dstdgcb_train_forward_backward) -
def build_block_train(c):
    salt, x_scale = _tune(c)
    torch.manual_seed(c.cin + c.cout + 7 * c.T + c.B + 1000 * salt)
    blk = DSTDGCB(c.cin, c.cout, c.T, c.V, c.layout)
    randomise(blk, 100 + c.cin + c.cout + c.T + salt)
    x = x_scale * torch.randn(c.B, c.cin, c.T, c.V)
    w = torch.randn(c.B, c.cout, c.T, c.V)
    return blk, x, w


def block_train_reference(c, dtype=torch.float64, built=None):
    """Oracle train-mode forward + backward of a block case in ``dtype``:
    {"y", "dx", "grads": {name: gradient}, "stats": [(batch mean, unbiased
    batch variance) per BatchNorm in call order]}.  A_s is a constant holding
    R_s's values (the alias)."""
    blk, x, w = built if built is not None else build_block_train(c)
    skip = ("running_mean", "running_var", "num_batches_tracked")
    P = {k: v.detach().clone().to(dtype) for k, v in blk.state_dict().items() if not k.endswith(skip)}
    for k in P:
        if not k.endswith(("A_s", "A_t")):
            P[k].requires_grad_(True)
    P["A_s"] = P["R_s"].detach()
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    O.BN_RECORD = []
    try:
        y = O.dstdgcb(xr, P, training=True)
        stats = O.BN_RECORD
    finally:
        O.BN_RECORD = None
    (y * w.to(dtype)).sum().backward()
    return {"y": y.detach(), "dx": xr.grad, "grads": {k: v.grad for k, v in P.items() if v.grad is not None},
            "stats": stats}


def block_train_errors(got, ref):
    """Errors of ``got`` against ``ref`` in units of the bar's normalisation:
    y and dx relative to their own max; a parameter gradient relative to
    max(its own max, 1e-3 of the block's largest gradient) -- a conv bias
    feeding a train-mode BN has a true gradient of ~0 (the BN mean removes
    it), so every tensor is judged against the block's gradient scale."""
    out = {"y": rel(got["y"], ref["y"]), "dx": rel(got["dx"], ref["dx"])}
    gscale = max(float(g.abs().max()) for g in ref["grads"].values())
    assert set(got["grads"]) == set(ref["grads"]), set(got["grads"]) ^ set(ref["grads"])
    for k, r in ref["grads"].items():
        err = float((got["grads"][k].detach().double().cpu() - r.double()).abs().max())
        out[k] = err / max(float(r.abs().max()), 1e-3 * gscale)
    return out
