"""The do_in dropout mask of the native training path restated on the host
(tests/test_dropout_host.py, tests/test_gpu_dropout.py).

k_dropout (csrc/dstd_train.hip) keeps element e of h[0] when

    u(e) = (mix64(seed * 0x9e3779b97f4a7c15 + e) >> 40) * 2^-24  >=  p

with mix64 the splitmix64 finaliser, every product and sum modulo 2^64, u and p
in float32, and scales what it keeps by 1.f / (1.f - p) in float32.  e is the
flat index into h[0] [B][C][T][V] (S.h[0] of csrc/dstd_train_capi.hip); under
DSTD_TRAIN_PAIRED B covers both halves and the halves share the seed, so the
second half's mask is the second half of the one stream.

The mask is a pure function of (seed, e, p): with it the fp64 oracle
(oracle/dstdgcn_oracle.py, ``drop=``) is a reference for dropout training.
"""
import numpy as np
import torch

GOLDEN = 0x9E3779B97F4A7C15
M1 = 0xBF58476D1CE4E5B9
M2 = 0x94D049BB133111EB
MASK64 = (1 << 64) - 1


def uniforms(seed, n):
    """u(e) for e < n as float32 (24-bit values in [0, 1): exact)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK64) * np.uint64(GOLDEN) + np.arange(n, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_mask(seed, n, p):
    """bool [n]: the elements k_dropout keeps."""
    return uniforms(seed, n) >= np.float32(p)


def keep_scale(p):
    """1.f / (1.f - p) as the kernel computes it."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def uniforms_scalar(seed, n):
    """uniforms() in plain Python integers, one element at a time."""
    out = []
    for e in range(n):
        z = ((seed & MASK64) * GOLDEN + e) & MASK64
        z = ((z ^ (z >> 30)) * M1) & MASK64
        z = ((z ^ (z >> 27)) * M2) & MASK64
        z ^= z >> 31
        out.append(np.float32(z >> 40) * np.float32(2.0 ** -24))
    return np.array(out, dtype=np.float32)


def drop_tensor(seed, shape, p, dtype=torch.float64):
    """mask * scale over h[0]'s shape [B, C, T, V] -- the oracle's ``drop``
    (permute(0, 2, 3, 1) for the channels-last oracle).  The scale is the
    kernel's float32 value, exact in ``dtype``."""
    n = int(np.prod(shape))
    m = keep_mask(seed, n, p).reshape(shape)
    return torch.from_numpy(m.astype(np.float64) * float(keep_scale(p))).to(dtype)


def drawn_seeds(s, device, windows=1):
    """The seeds an eager forward draws after ``torch.manual_seed(s)``:
    _ModelTrain.forward draws torch.randint(0, 2**62, (1,)) on the input's
    device, the rollouts (windows,) in one call.  Leaves the generators as
    manual_seed(s) leaves them, so the model call that follows draws these."""
    torch.manual_seed(s)
    v = torch.randint(0, 2 ** 62, (windows,), device=device, dtype=torch.int64)
    torch.manual_seed(s)
    return [int(a) for a in v.tolist()]


# ---- the two models of the dropout tests, on the CPU -------------------------------------
def cut_to(m, V):
    """A model built on the layout's skeleton cut to its first V joints, as
    test_gpu_predict.small_model cuts it."""
    import torch.nn as nn

    from model import DSTDGCB
    for blk in m.modules():
        if isinstance(blk, DSTDGCB):
            A = blk.A_s.data[:, :V, :V].clone()
            blk.A_s = nn.Parameter(A, False)
            blk.W_s = nn.Parameter(torch.zeros_like(A))
            blk.R_s = nn.Parameter(A.clone())
    return m


def model_a():
    """test_gpu_predict.small_model(3, 3) before its move to the GPU: T 6, the
    h36m skeleton's first 5 joints, 8 channels, one encoder layer (the generic
    kernels)."""
    from model import get_model
    from test_gpu_train import randomise
    Tin, Tout, V = 3, 3, 5
    torch.manual_seed(900 + 10 * Tin + Tout)
    m = cut_to(get_model("dstdgcn", dstdgcn=dict(input_channels=6, input_time_frame=Tin, output_time_frame=Tout,
                                                 st_gcnn_dropout=0.0, joints_to_consider=V, num_feature=8,
                                                 num_layers=1, layout="h36m")), V)
    randomise(m, 17 + Tin)
    return m.eval()


def model_b():
    """One encoder layer at the H36M shape (T 35, V 22, 64 channels: the
    split-f16 layout's training kernels), randomise()d."""
    from model import get_model
    from test_gpu_train import randomise
    torch.manual_seed(935)
    m = get_model("dstdgcn", dstdgcn=dict(input_channels=6, input_time_frame=10, output_time_frame=25,
                                          st_gcnn_dropout=0.0, joints_to_consider=22, num_feature=64, num_layers=1,
                                          layout="h36m"))
    randomise(m, 36)
    return m.eval()


def step_inputs(m, B, seed):
    """(x, dy) [B, T, V, 3]: a sequence whose future frames repeat the last
    observed one (the engine's input), and a random upstream gradient."""
    g = torch.Generator().manual_seed(seed)
    T, V = m.input_time_frame + m.output_time_frame, m.joints_to_consider
    x = 0.6 * torch.randn(B, T, V, 3, generator=g)
    x[:, m.input_time_frame:] = x[:, m.input_time_frame - 1:m.input_time_frame]
    return x, torch.randn(B, T, V, 3, generator=g)


def fast_state(sd, V):
    """The state dict of model/dstdgcn_fast.py's DSTDGCN that computes what the
    base model of state dict ``sd`` computes (the inverse of the derivation in
    dstdgcn_fast._links): A_s is the whole spatial adjacency transposed, A_t /
    R_t are transposed, conv_m1 and conv_m2 trade places, conv_rm's weight
    changes sign, conv_f and the block residual are nn.Linear, BatchNorm
    channels are ordered (v, c)."""
    out = {}
    for k, v in sd.items():
        pre, leaf = k.rsplit(".", 1)
        if leaf in ("W_s", "R_s"):
            continue
        if leaf == "A_s":
            v = (sd[pre + ".A_s"] * sd[pre + ".W_s"] + sd[pre + ".R_s"]).transpose(-1, -2)
        elif leaf in ("A_t", "R_t"):
            v = v.transpose(-1, -2)
        elif pre.endswith(".bn") and leaf != "num_batches_tracked":
            v = v.reshape(-1, V).t().reshape(-1)
        elif pre.endswith("conv_m1"):
            k = pre[:-1] + "2." + leaf
        elif pre.endswith("conv_m2"):
            k = pre[:-1] + "1." + leaf
        elif pre.endswith("conv_rm") and leaf == "weight":
            v = -v
        elif (pre.endswith("conv_f") or pre.endswith("residual.0")) and leaf == "weight":
            v = v.reshape(v.shape[0], v.shape[1])
        out[k] = v.detach().clone().contiguous()
    return out


def fast_model_a(p):
    """(model/dstdgcn_fast.py's DSTDGCN computing what model_a() computes, on
    the CPU; its state dict).  Built on the skeleton's first 5 joints like
    model_a, its private shadow (_make_shadow) cut alike."""
    from model import dstdgcn as base
    from model import dstdgcn_fast as F

    class SmallFast(F.DSTDGCN):
        def __init__(self, *args):
            super().__init__(*args)
            V = self.joints_to_consider
            for blk in self.modules():
                if isinstance(blk, F.DSTDGCB):
                    blk.A_s = torch.nn.Parameter(blk.A_s.data[:, :V, :V].clone())

        def _make_shadow(self):
            return cut_to(base.DSTDGCN(*self._ctor), self.joints_to_consider)

    a = model_a()
    fsd = fast_state(a.state_dict(), a.joints_to_consider)
    fm = SmallFast(6, a.input_time_frame, a.output_time_frame, p, a.joints_to_consider, a.num_feature, a.num_layers,
                   "h36m")
    fm.load_state_dict(fsd)
    return fm, fsd


# ---- one step through the oracle ----------------------------------------------------------
def oracle_step(sd0, num_layers, xs, dys, drops, dtype=torch.float64, device="cpu", fast=False, perms=None,
                record=False):
    """Train-mode forward and backward of loss = sum_i (y_i * dy_i).sum() over
    the batches ``xs`` (one, or the two halves of a pair: each its own
    BatchNorm batch and its own mask ``drops[i]`` [B, C, T, V], None for no
    dropout), through the oracle in ``dtype``.  ``perms[i]``: the sample order
    batch i is run in (its mask rows travel with the samples; outputs come
    back in the original order).  Returns {"y", "dx", parameter name: gradient}
    as float64 numpy, y and dx concatenated over the batches, and with
    ``record`` also "stats": per batch the oracle's BN_RECORD."""
    from oracle import dstdgcn_oracle as O
    P = O.train_params(sd0, dtype, device)
    if fast:
        for k, v in P.items():
            if k.endswith(".A_s"):
                v.requires_grad_(True)
    fn = O.fast_dstdgcn_fn if fast else O.dstdgcn_fn
    loss, ys, xg, stats = 0, [], [], []
    for i, (x, dy, drop) in enumerate(zip(xs, dys, drops)):
        perm = torch.arange(x.shape[0]) if perms is None else torch.as_tensor(perms[i])
        xi = x.to(device, dtype)[perm.to(device)].clone().requires_grad_(True)
        if drop is not None:
            drop = drop.permute(0, 2, 3, 1) if fast else drop
            drop = drop.to(device, dtype)[perm.to(device)]
        O.BN_RECORD = [] if record else None
        try:
            y = fn(xi, P, num_layers, training=True, drop=drop)
            stats.append(O.BN_RECORD)
        finally:
            O.BN_RECORD = None
        loss = loss + (y * dy.to(device, dtype)[perm.to(device)]).sum()
        ys.append((y, perm))
        xg.append((xi, perm))
    loss.backward()

    def back(t, perm):  # row perm[j] of the original order is row j of the run
        out = np.empty(tuple(t.shape), dtype=np.float64)
        out[perm.numpy()] = t.detach().double().cpu().numpy()
        return out

    res = {"y": np.concatenate([back(y, p) for y, p in ys]), "dx": np.concatenate([back(x.grad, p) for x, p in xg])}
    res.update({k: v.grad.double().cpu().numpy() for k, v in P.items() if v.grad is not None})
    if record:
        res["stats"] = stats
    return res
