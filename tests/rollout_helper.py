"""The backward of the rollout contract (include/ext/dstd_gcn_rollout.h)
restated, and the loop a caller writes without ``DSTDGCN.rollout``
(tests/test_rollout_host.py, tests/test_gpu_rollout.py).

With Tin observed frames, T-frame windows, Tout = T - Tin, K = ceil(H / Tout)
and m(s) = min(s, Tin - 1), for k = K-1 .. 0 (G_K: no term):

    dy_k[:, s]  = 0                                                         s <  Tin
    dy_k[:, s]  = sum over s' with Tout + m(s') == s of G_{k+1}[:, s']
                  + (dout[:, k*Tout + s - Tin] while that frame is < H)     s >= Tin
    dx_k        = vjp_k(dy_k)
    G_k[:, t]   = (G_{k+1}[:, t - Tout] if Tout <= t < Tin) + dx_k[:, t]
    dobs[:, i]  = G_0[:, i] (i < Tin - 1),  dobs[:, Tin-1] = G_0[:, Tin-1] + ... + G_0[:, T-1]

Every sum runs in ascending s' by sequential adds from its first term, the
dout / dx term last.  ``glue_dy`` / ``glue_fold`` / ``glue_obs`` are the three
steps on numpy arrays in the arrays' own dtype: on float64 the closed form,
on float32 the exact restatement of the kernels (numpy adds two fp32 arrays
with one IEEE rounding per element, as the kernels' chains do).

``rollout_loop`` is the window loop over ``model(x)`` under autograd, the way
it can be written without the feature; its glue between two forwards is a
small autograd Function whose backward does the sums above slice by slice
with fp32 tensor adds, so its gradients have one order on any device.
"""
import numpy as np
import torch


def windows(T, Tin, H):
    return -(-H // (T - Tin))


def glue_dy(dout, Gn, T, Tin, k):
    """dy_k [N, T, ...] from dout [N, H, ...] and Gn = G_{k+1} (None: no term)."""
    Tout, H = T - Tin, dout.shape[1]
    dy = np.zeros((dout.shape[0], T) + dout.shape[2:], dtype=dout.dtype)
    for s in range(Tin, T):
        acc = None
        if Gn is not None:
            for sp in range(T):  # ascending s'
                if Tout + min(sp, Tin - 1) == s:
                    acc = Gn[:, sp].copy() if acc is None else acc + Gn[:, sp]
        f = k * Tout + s - Tin
        if f < H:
            acc = dout[:, f].copy() if acc is None else acc + dout[:, f]
        if acc is not None:
            dy[:, s] = acc
    return dy


def glue_fold(dx, Gn, T, Tin):
    """G_k from dx_k and Gn = G_{k+1} (None: G_k = dx_k)."""
    Tout = T - Tin
    G = dx.copy()
    if Gn is not None:
        for t in range(Tout, Tin):
            G[:, t] = Gn[:, t - Tout] + dx[:, t]
    return G


def glue_obs(G0, T, Tin):
    dobs = G0[:, :Tin].copy()
    acc = G0[:, Tin - 1].copy()
    for s in range(Tin, T):
        acc = acc + G0[:, s]
    dobs[:, Tin - 1] = acc
    return dobs


def rollout_backward(dout, T, Tin, vjp):
    """dobs [N, Tin, ...] for dout [N, H, ...]; ``vjp(k, dy)`` is window k's
    input gradient for the output gradient dy (both [N, T, ...])."""
    K = windows(T, Tin, dout.shape[1])
    G = None
    for k in range(K - 1, -1, -1):
        G = glue_fold(vjp(k, glue_dy(dout, G, T, Tin, k)), G, T, Tin)
    return glue_obs(G, T, Tin)


# ---- the loop under autograd -------------------------------------------------
class _Pad(torch.autograd.Function):
    """x_0[:, s] = obs[:, m(s)]; backward: the padding copies summed ascending."""

    @staticmethod
    def forward(ctx, obs, T):
        ctx.T, ctx.Tin = T, obs.shape[1]
        return obs[:, [min(s, ctx.Tin - 1) for s in range(T)]].contiguous()

    @staticmethod
    def backward(ctx, G0):
        T, Tin = ctx.T, ctx.Tin
        dobs = G0[:, :Tin].clone()
        acc = G0[:, Tin - 1].clone()
        for s in range(Tin, T):
            acc = acc + G0[:, s]
        dobs[:, Tin - 1] = acc
        return dobs, None


class _Roll(torch.autograd.Function):
    """(x_k, y_k) -> (y_k[:, Tin:Tin + take], x_{k+1}) with
    x_{k+1}[:, s] = seq_k[:, Tout + m(s)], seq_k = x_k below Tin, y_k from Tin on.
    ``last``: no next window (x_{k+1} is returned empty)."""

    @staticmethod
    def forward(ctx, x, y, Tin, take, last):
        T = x.shape[1]
        ctx.dims = (T, Tin, take, last)
        seq = torch.cat([x[:, :Tin], y[:, Tin:]], 1)
        xn = x.new_empty(0) if last else seq[:, [T - Tin + min(s, Tin - 1) for s in range(T)]].contiguous()
        return y[:, Tin:Tin + take].contiguous(), xn

    @staticmethod
    def backward(ctx, dout, Gn):
        T, Tin, take, last = ctx.dims
        Tout = T - Tin
        dy = torch.zeros((dout.shape[0], T) + tuple(dout.shape[2:]), dtype=dout.dtype, device=dout.device)
        dx = torch.zeros_like(dy)
        for s in range(Tin, T):
            acc = None
            if not last:
                for sp in range(T):
                    if Tout + min(sp, Tin - 1) == s:
                        acc = Gn[:, sp].clone() if acc is None else acc + Gn[:, sp]
            if s - Tin < take:
                acc = dout[:, s - Tin].clone() if acc is None else acc + dout[:, s - Tin]
            if acc is not None:
                dy[:, s] = acc
        if not last:
            for t in range(Tout, Tin):  # the frames window k + 1 took from x_k; autograd adds dx_k to them
                dx[:, t] = Gn[:, t - Tout]
        return dx, dy, None, None, None


def rollout_loop(model, obs, H, forward=None, T=None):
    """The ``H`` frames after ``obs`` by a loop of ``model(x_k)`` under
    autograd (or of ``forward(x_k)`` over windows of ``T`` frames)."""
    T = model.input_time_frame + model.output_time_frame if forward is None else T
    f = forward if forward is not None else (lambda w: model(w))
    Tin = obs.shape[1]
    Tout, K = T - Tin, windows(T, Tin, H)
    x, outs = _Pad.apply(obs, T), []
    for k in range(K):
        y = f(x)
        o, x = _Roll.apply(x, y, Tin, min(Tout, H - k * Tout), k == K - 1)
        outs.append(o)
    return torch.cat(outs, 1)


def rollout_loop_pair(model, obs1, obs2, H):
    """The same for a batch and its time reversal: ``model.forward_pair`` per
    window, each half rolled on its own."""
    T = model.input_time_frame + model.output_time_frame
    Tin = obs1.shape[1]
    Tout, K = T - Tin, windows(T, Tin, H)
    xs, outs = [_Pad.apply(obs1, T), _Pad.apply(obs2, T)], ([], [])
    for k in range(K):
        ys = model.forward_pair(xs[0], xs[1])
        for h in range(2):
            o, xs[h] = _Roll.apply(xs[h], ys[h], Tin, min(Tout, H - k * Tout), k == K - 1)
            outs[h].append(o)
    return torch.cat(outs[0], 1), torch.cat(outs[1], 1)
