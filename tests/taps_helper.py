"""References and cases for the tap tests (include/dstd_gcn_taps.h,
DSTDGCB.forward_taps / DSTDGCN.forward_taps).

The oracle (oracle/dstdgcn_oracle.py) forms a DSTDGC's adjacency inside
``dstdgc`` and contracts it at once; ``dynamic_adj`` restates those lines
(:50-55 spatial, :58-62 temporal) so that the matrices themselves can be
compared, and ``block_adjacencies`` applies it to a block's two spatial graphs
and its temporal graph.  ``oracle_taps`` walks a whole model (dstdgcn_fn,
:125-136) and keeps every block's x / h / adjacencies; ``spatial_half`` /
``temporal_half`` / ``after_block`` are the pieces of that walk, used to check
that a call's taps are consistent with each other.
"""
import functools

import numpy as np
import torch

from conftest import group, load_npz
from model import DSTDGCB, get_model
from oracle import dstdgcn_oracle as O

TAP_BAR = 1e-4  # the project's per-op / per-block bar (tests/test_gpu_parity.py)


def dynamic_adj(x, p, A, alpha, mode):
    """The ``adj`` of O.dstdgc: [n, T, V, V] (spatial) / [n, V, T, T] (temporal)."""
    p1 = O.conv1x1(x, p["conv_m1.weight"], p["conv_m1.bias"])
    q1 = O.conv1x1(x, p["conv_m2.weight"], p["conv_m2.bias"])
    n, r, t, v = p1.shape
    wrm = p["conv_rm.weight"].reshape(p["conv_rm.weight"].shape[0], -1)
    brm = p["conv_rm.bias"]
    if mode == "spatial":
        pk = p1.reshape(n, r * t, v)
        qk = q1.reshape(n, r * t, v)
        m = torch.tanh(pk[:, :, :, None] - qk[:, :, None, :])
        d = torch.einsum("tk,nkvw->ntvw", wrm, m) + brm.view(1, -1, 1, 1)
    else:
        pk = p1.permute(0, 1, 3, 2).reshape(n, r * v, t)
        qk = q1.permute(0, 1, 3, 2).reshape(n, r * v, t)
        m = torch.tanh(pk[:, :, :, None] - qk[:, :, None, :])
        d = torch.einsum("vk,nktu->nvtu", wrm, m) + brm.view(1, -1, 1, 1)
    return d * alpha + A


def cast_sd(sd, dtype):
    return {k: torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v).detach().cpu().to(dtype)
            for k, v in sd.items() if not k.endswith("num_batches_tracked")}


def spatial_adjs(x, p):
    """[n, 2, T, V, V]: the matrices conv_s[0], conv_s[1] contract (oracle :106-108)."""
    return torch.stack([dynamic_adj(x, O.sub(p, f"conv_s.{i}."),
                                    p["A_s"][i:i + 1] * p["W_s"][i:i + 1] + p["R_s"][i:i + 1], p["alpha_sm"], "spatial")
                        for i in range(p["A_s"].shape[0])], dim=1)


def temporal_adj(h, p):
    """[n, V, T, T]: the matrix conv_t[0] contracts (oracle :111-112)."""
    return dynamic_adj(h, O.sub(p, "conv_t.0."), p["A_t"][0:1] + p["R_t"][0:1], p["alpha_tm"], "temporal")


def block_adjacencies(x, h, p, dtype=torch.float64):
    """(adj_s [n, 2, T, V, V], adj_t [n, V, T, T]) of a DSTDGCB with state-dict
    entries ``p`` (no prefix) on block input ``x`` and temporal-GC input ``h``,
    computed in ``dtype``."""
    p = cast_sd(p, dtype)
    x, h = x.detach().cpu().to(dtype), h.detach().cpu().to(dtype)
    return spatial_adjs(x, p), temporal_adj(h, p)


def spatial_half(x, adj_s, p):
    """h of a block from its input and its spatial adjacencies (oracle :100-110)."""
    if x.shape[1] != p["conv_s.0.conv_f.weight"].shape[0]:
        r = O.batchnorm(O.conv1x1(x, p["residual.0.weight"], p["residual.0.bias"]), O.sub(p, "residual.1.bn."))
    else:
        r = x
    y = 0
    for i in range(adj_s.shape[1]):
        xf = O.conv1x1(x, p[f"conv_s.{i}.conv_f.weight"], p[f"conv_s.{i}.conv_f.bias"])
        y = y + torch.einsum("nctv,ntvw->nctw", xf, adj_s[:, i])
    return O.prelu(O.batchnorm(y, O.sub(p, "bn.bn.")) + r, p["prelu.weight"])


def temporal_half(h, adj_t, p):
    """A block's output from h and its temporal adjacency (oracle :63, :112)."""
    xf = O.conv1x1(h, p["conv_t.0.conv_f.weight"], p["conv_t.0.conv_f.bias"])
    return torch.einsum("nctv,nvtu->ncuv", xf, adj_t)


def block_prefixes(num_layers):
    return (["conv_st_in.stgcn.0.0."] + [f"encoders.{i}.0.stgcn.0.0." for i in range(num_layers)]
            + ["conv_st_out.stgcn.0.0."])


def after_block(b, out, x_blk, x_model, sd, num_layers):
    """What follows block b's raw output in O.dstdgcn_fn (:130-136): the next
    block's input, or for the last block the model output [n, T, V, 3]."""
    if b == 0:
        return O.prelu(O.batchnorm(out, O.sub(sd, "bn_in.bn.")), sd["prelu.weight"])
    if b <= num_layers:
        e = f"encoders.{b - 1}."
        return O.prelu(O.batchnorm(out + x_blk, O.sub(sd, e + "1.bn.")), sd[e + "2.weight"])
    return out.permute(0, 2, 3, 1) + x_model[:, -1:]


def model_input6(x):
    """cat(x, x - x[:, -1:]) as NCTV (oracle :127-128)."""
    return torch.cat((x, x - x[:, -1:]), dim=-1).permute(0, 3, 1, 2)


def oracle_taps(x, sd, num_layers, dtype=torch.float64):
    """(y, [per block {"x", "h", "adj_s", "adj_t"}]) of the oracle's forward."""
    sd = cast_sd(sd, dtype)
    x = x.detach().cpu().to(dtype)
    cur, taps = model_input6(x), []
    for b, pre in enumerate(block_prefixes(num_layers)):
        p = O.sub(sd, pre)
        adj_s = spatial_adjs(cur, p)
        h = spatial_half(cur, adj_s, p)
        adj_t = temporal_adj(h, p)
        taps.append({"x": cur, "h": h, "adj_s": adj_s, "adj_t": adj_t})
        cur = after_block(b, temporal_half(h, adj_t, p), cur, x, sd, num_layers)
    return cur, taps


def oracle_block_taps(x, p, dtype=torch.float64):
    p = cast_sd(p, dtype)
    x = x.detach().cpu().to(dtype)
    adj_s = spatial_adjs(x, p)
    h = spatial_half(x, adj_s, p)
    adj_t = temporal_adj(h, p)
    return temporal_half(h, adj_t, p), [{"x": x, "h": h, "adj_s": adj_s, "adj_t": adj_t}]


def randomise_dynamic(module, seed):
    """A freshly constructed model has alpha_* = 0, W_s = 0, R_t = 0 and
    conv_rm = 0, i.e. no dynamic graph at all.  Draw them (and R_s, the
    conv biases and the BatchNorm statistics) so that every term of the
    adjacencies is alive."""
    g = torch.Generator().manual_seed(seed)

    def rn(t, s):
        return s * torch.randn(t.shape, generator=g)

    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, DSTDGCB):
                m.alpha_sm.fill_(0.6 + 0.3 * float(torch.rand((), generator=g)))
                m.alpha_tm.fill_(-0.4 - 0.3 * float(torch.rand((), generator=g)))
                m.W_s.copy_(rn(m.W_s, 0.3))
                m.R_s.copy_(rn(m.R_s, 0.2))  # (A_s shares its storage, as in the reference)
                m.R_t.copy_(rn(m.R_t, 0.1))
                for gc in list(m.conv_s) + list(m.conv_t):
                    k = gc.conv_rm.weight.shape[1]
                    gc.conv_rm.weight.copy_(rn(gc.conv_rm.weight, k ** -0.5))
                    gc.conv_rm.bias.copy_(rn(gc.conv_rm.bias, 0.1))
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(rn(m.running_mean, 0.1))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(m.running_var.shape, generator=g))
                m.weight.copy_(0.8 + 0.4 * torch.rand(m.weight.shape, generator=g))
    return module


def calibrate_bn(model, x):
    """Running statistics as training would have left them: every BatchNorm's
    running mean / variance := the statistics of its own input on ``x`` (the
    oracle's train-mode walk, BN_RECORD in call order).  Without it a randomly
    drawn model multiplies its activations 20-50x per block, and at |h| ~ 1e5
    the P - Q of a tanh is no longer an fp32 quantity worth comparing."""
    L = model.num_layers
    sd = cast_sd(model.state_dict(), torch.float64)
    O.BN_RECORD = rec = []
    try:
        O.dstdgcn_fn(x.double(), sd, L, training=True)
    finally:
        O.BN_RECORD = None
    order = ["conv_st_in.stgcn.0.0.residual.1.bn", "conv_st_in.stgcn.0.0.bn.bn", "bn_in.bn"]
    for i in range(L):
        order += [f"encoders.{i}.0.stgcn.0.0.bn.bn", f"encoders.{i}.1.bn"]
    order += ["conv_st_out.stgcn.0.0.residual.1.bn", "conv_st_out.stgcn.0.0.bn.bn"]
    assert len(order) == len(rec)
    mods = dict(model.named_modules())
    with torch.no_grad():
        for name, (mean, var) in zip(order, rec):
            mods[name].running_mean.copy_(mean)
            mods[name].running_var.copy_(var)
    return model


# ---- the cases ---------------------------------------------------------------
FIXTURES = ("h36m", "cmu", "3dpw", "h36m75")
SYNTH = ((5, 1), (5, 3), (12, 1), (12, 3), (128, 1), (128, 3))  # (T, B), h36m layout, num_layers = 1
RANGE_ALPHA = 3e4
CASES = ([f"fix-{t}" for t in FIXTURES] + [f"syn-T{T}-B{B}" for T, B in SYNTH] + ["blk-range"])
SYN_SPLIT = {5: (2, 3), 12: (5, 7), 128: (50, 78)}  # T -> (input frames, output frames)


def synth_input(B, T, V, Tin, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, 3, generator=g)
    x[:, Tin:] = x[:, Tin - 1:Tin]
    return x


class Case:
    """module (CPU, eval), x, kind "model" / "block", sd (fp32 tensors, what
    the module holds), num_layers, and the fp64 oracle's y / taps on x."""

    def __init__(self, name, module, x, kind):
        self.name, self.module, self.x, self.kind = name, module.eval(), x, kind
        self.sd = {k: v.detach().clone() for k, v in module.state_dict().items()}
        self.num_layers = module.num_layers if kind == "model" else 0
        if kind == "model":
            self.y64, self.taps64 = oracle_taps(x, self.sd, self.num_layers)
        else:
            self.y64, self.taps64 = oracle_block_taps(x, self.sd)

    def block_sd(self, b, dtype=torch.float64):
        sd = cast_sd(self.sd, dtype)
        return sd if self.kind == "block" else O.sub(sd, block_prefixes(self.num_layers)[b])


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, rest = name.partition("-")
    if kind == "fix":
        d = load_npz(f"model_{rest}.npz")
        opts = {k[4:]: d[k].item() for k in d.files if k.startswith("opt/")}
        m = get_model("dstdgcn", dstdgcn=opts)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in group(d, "sd/").items()})
        return Case(name, m, torch.from_numpy(d["x"].copy()), "model")
    if kind == "syn":
        T, B = (int(s[1:]) for s in rest.split("-"))
        tin, tout = SYN_SPLIT[T]
        torch.manual_seed(100 + T)
        m = get_model("dstdgcn", dstdgcn=dict(input_channels=6, input_time_frame=tin, output_time_frame=tout,
                                              st_gcnn_dropout=0.1, joints_to_consider=22, num_feature=64,
                                              num_layers=1, layout="h36m"))
        randomise_dynamic(m, 200 + T)
        calibrate_bn(m, synth_input(4, T, 22, tin, 250 + T))  # one model per T, whatever the case's B
        return Case(name, m, synth_input(B, T, 22, tin, 300 + 7 * T + B), "model")
    if name == "blk-range":
        torch.manual_seed(17)
        blk = randomise_dynamic(DSTDGCB(64, 64, 35, 22, "h36m"), 18)
        with torch.no_grad():
            blk.alpha_sm.fill_(RANGE_ALPHA)
            blk.alpha_tm.fill_(RANGE_ALPHA)
            # the spatial GCs' sum grows with alpha_sm; the BatchNorm scale takes it back to O(1), so
            # that h -- and with it the P - Q the temporal tanh sees -- stays well conditioned in
            # fp32 (at |P - Q| ~ 1e5 one fp32 rounding of P moves a tanh near its zero by 1e-2)
            blk.bn.bn.weight.mul_(1.0 / RANGE_ALPHA)
        g = torch.Generator().manual_seed(19)
        return Case(name, blk, torch.randn(2, 64, 35, 22, generator=g), "block")
    raise KeyError(name)


def rel(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def plane_bound(p, which):
    """The bound the split kernels derive a plane range shift from
    (dstd_hilo.h "range scaling"): |alpha| max_r(sum_k |W_rm| + |b_rm|) +
    max|Astat| of a block's spatial graph i (which = 0, 1) or its temporal
    graph (which = "t"), from the block's state-dict entries."""
    p = cast_sd(p, torch.float64)
    if which == "t":
        gc, alpha, astat = "conv_t.0.", p["alpha_tm"], p["A_t"][0] + p["R_t"][0]
    else:
        gc, alpha = f"conv_s.{which}.", p["alpha_sm"]
        astat = p["A_s"][which] * p["W_s"][which] + p["R_s"][which]
    w = p[gc + "conv_rm.weight"].reshape(p[gc + "conv_rm.weight"].shape[0], -1)
    rb = (w.abs().sum(dim=1) + p[gc + "conv_rm.bias"].abs()).max()
    return float(alpha.abs().reshape(()) * rb + astat.abs().max())
