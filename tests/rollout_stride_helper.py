"""Training through a strided rollout (include/ext/dstd_gcn_stride_train.h)
restated, and the loop a caller writes without ``DSTDGCN.rollout(stride=)``
(tests/test_rollout_stride_host.py, tests/test_gpu_rollout_stride.py).

With Tin observed frames, T-frame windows, Tout = T - Tin, S = stride
(1 <= S <= Tout), H = horizon, K = ceil(H / S), m(s) = min(s, Tin - 1), the known
sequence h = cat(obs, out), an optional mask [K, N] (row k: the boundary into
window k; row 0 is not read) and a truth read through one frame map (t0, step)
per half:

    x_k[b, s]        = h[b, k*S + m(s)]                                   free
    x_k[b, s]        = truth[b mod Nt, t0_h + step_h * (k*S + m(s))]      k >= 1 and mask[k, b]
    h[b, k*S + i]    = x_k[b, i]     i < Tin     (a forced sample knows the truth's frames from then on)
    y_k              = forward(k, x_k)
    out[:, k*S + j]  = h[:, Tin + k*S + j] = y_k[:, Tin + j]     j = 0..S-1 while k*S + j < H

and, with a gradient history Gh [N, Tin + H, ...] that starts at zero, for
k = K-1 .. 0:

    dy_k[:, s]  = Gh[:, k*S + s] + dout[:, k*S + s - Tin]    Tin <= s < Tin + S while that frame is < H
    dy_k[:, s]  = 0                                          elsewhere
    dx_k        = vjp_k(dy_k)
    where (k >= 1 and mask[k, b]):
      Gh[b, k*S + i]        = 0                              i < Tin
    elsewhere:
      Gh[b, k*S + i]       += dx_k[b, i]                     i < Tin - 1
      Gh[b, k*S + Tin - 1]  = ((Gh[b, k*S + Tin - 1] + dx_k[b, Tin - 1]) + ...) + dx_k[b, T - 1]
    dobs        = Gh[:, :Tin]                                after window 0

``glue_dy`` / ``glue_acc`` are the two glue steps on numpy arrays in the
arrays' own dtype: on float32 the exact restatement of the kernels (numpy adds
two fp32 arrays with one IEEE rounding per element, as the kernels' chains do).

``strided_reference`` is the forward in torch, indexing, concatenation and one
torch.where per forced boundary alone (autograd differentiates it; without a
mask it is ``stride_helper.predict_strided_reference``).

``StridedLoop`` is the loop a user can write today, with the backward composed
by hand in that order: every x_k is built with torch indexing (torch.where for a
mask) as a detached leaf that requires grad, y_k = forward(k, x_k), and the
backward calls torch.autograd.backward per window, K-1 first, and folds
x_k.grad into Gh slice by slice with tensor adds -- so its gradients have one
order on any device and in any dtype.
"""
import numpy as np
import torch


def windows(H, S):
    return -(-H // S)


def _rows(mrow, like):
    if isinstance(like, np.ndarray):
        return np.asarray(mrow).astype(bool).reshape((-1,) + (1,) * (like.ndim - 1))
    return mrow.bool().reshape((-1,) + (1,) * (like.dim() - 1))


def truth_frames(T, Tin, S, k, fmap):
    """The truth frames of window k's T rows under the map (t0, step)."""
    t0, step = fmap
    return [t0 + step * (k * S + min(s, Tin - 1)) for s in range(T)]


def truth_window(truth, T, Tin, S, k, maps):
    """[halves * Nt, T, ...]: what window k is for a forced sample; truth is
    [Nt, frames, ...] (a torch tensor), maps one (t0, step) per half."""
    return torch.cat([truth[:, truth_frames(T, Tin, S, k, fm)] for fm in maps])


# ---- the backward glue on numpy arrays -------------------------------------------
def glue_dy(Gh, dout, T, Tin, S, k):
    """dy_k [N, T, ...] from Gh [N, Tin + H, ...] and dout [N, H, ...]."""
    H = dout.shape[1]
    dy = np.zeros((dout.shape[0], T) + dout.shape[2:], dtype=dout.dtype)
    for s in range(Tin, Tin + S):
        f = k * S + s - Tin
        if f < H:
            dy[:, s] = Gh[:, k * S + s] + dout[:, f]
    return dy


def glue_acc(Gh, dx, mrow, T, Tin, S, k):
    """Gh after window k's dx [N, T, ...] is handed back; mrow [N]: row k of the
    mask (None, or k == 0: nobody is forced); a forced sample's Tin rows become zero."""
    new = Gh.copy()
    f0 = k * S
    for i in range(Tin - 1):
        new[:, f0 + i] = Gh[:, f0 + i] + dx[:, i]
    acc = Gh[:, f0 + Tin - 1]
    for s in range(Tin - 1, T):
        acc = acc + dx[:, s]
    new[:, f0 + Tin - 1] = acc
    if mrow is not None and k >= 1:
        forced = Gh.copy()
        forced[:, f0:f0 + Tin] = 0
        new = np.where(_rows(mrow, Gh), forced, new)
    return new


# ---- the forward under autograd ------------------------------------------------------
def strided_reference(forward, obs, T, H, S, truth=None, mask=None, maps=((0, 1),)):
    """out [N, H, ...] of the contract above; ``forward(k, x)`` is window k's forward."""
    Tin = obs.shape[1]
    assert 1 <= Tin < T and H >= 1 and 1 <= S <= T - Tin and (truth is None) == (mask is None)
    m = [min(s, Tin - 1) for s in range(T)]
    h, outs = obs, []
    for k in range(windows(H, S)):
        x = h[:, [k * S + i for i in m]]
        if k >= 1 and mask is not None:
            x = torch.where(_rows(mask[k], x), truth_window(truth, T, Tin, S, k, maps), x)
        y = forward(k, x)
        outs.append(y[:, Tin:Tin + min(S, H - k * S)])
        h = torch.cat([h[:, :k * S], x[:, :Tin], outs[-1]], 1)
    return torch.cat(outs, 1)


# ---- the loop ----------------------------------------------------------------------
class StridedLoop:
    """The forward of the strided chain by a window loop, keeping every (x_k, y_k)
    for ``backward``.  ``forward(k, x)`` is window k's forward under autograd;
    ``obs`` [N, Tin, ...]; ``truth`` [Nt, frames, ...], ``mask`` [K, N] (torch,
    any integer or bool dtype) and ``maps`` (one (t0, step) per half of N) come
    together or not at all.  ``out`` [N, H, ...] is detached."""

    def __init__(self, forward, obs, T, H, S, truth=None, mask=None, maps=((0, 1),)):
        Tin = obs.shape[1]
        assert 1 <= Tin < T and H >= 1 and 1 <= S <= T - Tin
        assert (truth is None) == (mask is None)
        self.dims, self.mask = (T, Tin, S, H), mask
        K = windows(H, S)
        m = [min(s, Tin - 1) for s in range(T)]
        h, outs = obs.detach(), []
        self.xs, self.ys = [], []
        for k in range(K):
            x = h[:, [k * S + i for i in m]]
            if k >= 1 and mask is not None:
                x = torch.where(_rows(mask[k], x), truth_window(truth, T, Tin, S, k, maps), x)
            x = x.detach().contiguous().requires_grad_()
            y = forward(k, x)
            self.xs.append(x)
            self.ys.append(y)
            outs.append(y.detach()[:, Tin:Tin + min(S, H - k * S)])
            h = torch.cat([h[:, :k * S], x.detach()[:, :Tin], outs[-1]], 1)
        self.out = torch.cat(outs, 1).contiguous()

    def backward(self, dout, params=()):
        """dobs [N, Tin, ...] for dout [N, H, ...]; the gradients of ``params``
        accumulate into their .grad, window K-1 first (those that require grad)."""
        T, Tin, S, H = self.dims
        assert dout.shape[1] == H
        params = [p for p in params if p.requires_grad]
        Gh = torch.zeros((dout.shape[0], Tin + H) + tuple(dout.shape[2:]), dtype=dout.dtype, device=dout.device)
        for k in range(len(self.xs) - 1, -1, -1):
            f0 = k * S
            dy = torch.zeros((dout.shape[0], T) + tuple(dout.shape[2:]), dtype=dout.dtype, device=dout.device)
            for s in range(Tin, Tin + S):
                if f0 + s - Tin < H:
                    dy[:, s] = Gh[:, f0 + s] + dout[:, f0 + s - Tin]
            x = self.xs[k]
            torch.autograd.backward([self.ys[k]], [dy], inputs=[x, *params])
            dx = x.grad
            old = Gh[:, f0:f0 + Tin].clone()
            new = old.clone()
            for i in range(Tin - 1):
                new[:, i] = old[:, i] + dx[:, i]
            acc = old[:, Tin - 1]
            for s in range(Tin - 1, T):
                acc = acc + dx[:, s]
            new[:, Tin - 1] = acc
            if k >= 1 and self.mask is not None:
                new = torch.where(_rows(self.mask[k], new), torch.zeros_like(new), new)
            Gh[:, f0:f0 + Tin] = new
        self.xs = self.ys = None
        return Gh[:, :Tin].clone()


def model_loop(model, obs, H, S, truth=None, mask=None, fmap=(0, 1)):
    """StridedLoop over ``model(x_k)``."""
    T = obs.shape[1] + model.output_time_frame
    return StridedLoop(lambda k, x: model(x), obs, T, H, S, truth, mask, (fmap,))


def model_loop_pair(model, obs1, obs2, H, S, truth=None, mask=None):
    """StridedLoop over ``model.forward_pair`` on a batch and its time reversal
    (obs [2 N, ...], obs1's samples first): the second half reads ``truth``
    [N, Ttot, ...] backwards from its last frame; ``mask`` is [K, 2 N]."""
    n = obs1.shape[0]
    T = obs1.shape[1] + model.output_time_frame
    maps = ((0, 1), (truth.shape[1] - 1, -1)) if truth is not None else ((0, 1),)
    return StridedLoop(lambda k, x: torch.cat(model.forward_pair(x[:n], x[n:])), torch.cat([obs1, obs2]), T, H, S,
                       truth, mask, maps)
