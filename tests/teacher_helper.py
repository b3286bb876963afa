"""Scheduled sampling over the rollout (include/ext/dstd_gcn_teacher.h)
restated, and the loop a caller writes without the feature
(tests/test_teacher_host.py, tests/test_gpu_teacher.py).

With the symbols of tests/rollout_helper.py, a mask [K, N] (row k: the boundary
into window k) and a truth read through one frame map (t0, step) per half:

    x_{k+1}[b, s] = seq_k[b, Tout + m(s)]                                   mask[k+1, b] == 0
    x_{k+1}[b, s] = truth[b mod Nt, t0_h + step_h * ((k+1) * Tout + m(s))]  otherwise, h = b // Nt

and in the backward the G_{k+1} terms of dy_k[b] and of G_k[b] are absent for
the b that mask[k+1] forces.  ``glue_dy_tf`` / ``glue_fold_tf`` are
rollout_helper's steps with a mask row: per sample the step with G_{k+1} or the
step without it, selected, so no arithmetic is added to either (float64: the
closed form; float32: the kernels' sums exactly).

``teacher_reference`` is the forward written with torch indexing and
torch.where alone (autograd differentiates it); ``teacher_loop`` /
``teacher_loop_pair`` are the window loops over ``model(x_k)`` with
rollout_helper's glue Functions and a torch.where between two windows.  The
where's backward hands a forced sample zeros for G_{k+1}: the glue adds them
(x + 0 == x in every bit but the sign of a zero, which torch.equal does not
see), so the loop's gradients are those of the contract.
"""
import numpy as np
import torch

from rollout_helper import _Pad, _Roll, glue_dy, glue_fold, glue_obs, windows


def _rows(mrow, like):
    return np.asarray(mrow).astype(bool).reshape((-1,) + (1,) * (like.ndim - 1))


def glue_dy_tf(dout, Gn, mrow, T, Tin, k):
    """dy_k; mrow [N]: row k + 1 of the mask (None or Gn None: glue_dy)."""
    if Gn is None or mrow is None:
        return glue_dy(dout, Gn, T, Tin, k)
    free, forced = glue_dy(dout, Gn, T, Tin, k), glue_dy(dout, None, T, Tin, k)
    return np.where(_rows(mrow, free), forced, free)


def glue_fold_tf(dx, Gn, mrow, T, Tin):
    """G_k from dx_k; mrow as above: a forced sample's G_k is its dx_k."""
    if Gn is None or mrow is None:
        return glue_fold(dx, Gn, T, Tin)
    return np.where(_rows(mrow, dx), dx, glue_fold(dx, Gn, T, Tin))


def truth_frames(T, Tin, k, fmap):
    """The truth frames of window k's T rows under the map (t0, step)."""
    t0, step = fmap
    return [t0 + step * (k * (T - Tin) + min(s, Tin - 1)) for s in range(T)]


def truth_window(truth, T, Tin, k, maps):
    """[halves * Nt, T, ...]: what window k is for a forced sample.  truth is
    [Nt, frames, ...] (numpy or torch), maps one (t0, step) per half."""
    parts = [truth[:, truth_frames(T, Tin, k, fm)] for fm in maps]
    return np.concatenate(parts) if isinstance(truth, np.ndarray) else torch.cat(parts)


def teacher_forward(obs, truth, maps, mask, T, H, f):
    """numpy: out [N, H, ...] and the windows [x_0 .. x_{K-1}]; ``f(k, x)`` is window k's forward."""
    Tin = obs.shape[1]
    Tout, K = T - Tin, windows(T, Tin, H)
    x = obs[:, [min(s, Tin - 1) for s in range(T)]]
    outs, xs = [], []
    for k in range(K):
        xs.append(x)
        y = f(k, x)
        outs.append(y[:, Tin:Tin + min(Tout, H - k * Tout)])
        if k + 1 < K:
            seq = np.concatenate([x[:, :Tin], y[:, Tin:]], 1)
            free = seq[:, [Tout + min(s, Tin - 1) for s in range(T)]]
            x = np.where(_rows(mask[k + 1], free), truth_window(truth, T, Tin, k + 1, maps), free)
    return np.concatenate(outs, 1), xs


def teacher_backward(dout, mask, T, Tin, vjp):
    """dobs for dout [N, H, ...] under ``mask`` [K, N]; ``vjp(k, dy)`` as rollout_helper.rollout_backward's."""
    K = windows(T, Tin, dout.shape[1])
    G = None
    for k in range(K - 1, -1, -1):
        mrow = mask[k + 1] if k + 1 < K else None
        G = glue_fold_tf(vjp(k, glue_dy_tf(dout, G, mrow, T, Tin, k)), G, mrow, T, Tin)
    return glue_obs(G, T, Tin)


def teacher_reference(forward, obs, truth, maps, mask, T, H):
    """The forward contract in torch, indexing and torch.where alone."""
    Tin = obs.shape[1]
    Tout, K = T - Tin, windows(T, Tin, H)
    pad = [min(s, Tin - 1) for s in range(T)]
    x, outs = obs[:, pad], []
    for k in range(K):
        y = forward(x)
        outs.append(y[:, Tin:Tin + min(Tout, H - k * Tout)])
        if k + 1 < K:
            free = torch.cat([x[:, :Tin], y[:, Tin:]], 1)[:, [Tout + i for i in pad]]
            forced = mask[k + 1].bool().reshape((-1,) + (1,) * (free.dim() - 1))
            x = torch.where(forced, truth_window(truth, T, Tin, k + 1, maps), free)
    return torch.cat(outs, 1)


# ---- the loop under autograd -------------------------------------------------
def _force(xn, truth, mrow, T, Tin, k, maps):
    return torch.where(mrow.bool()[:, None, None, None], truth_window(truth, T, Tin, k, maps), xn)


def teacher_loop(model, obs, H, truth, mask, fmap=(0, 1)):
    """rollout_helper.rollout_loop with ``mask`` [K, N] and ``truth`` [N, frames, V, 3]."""
    Tin = obs.shape[1]
    T = Tin + model.output_time_frame
    Tout, K = T - Tin, windows(T, Tin, H)
    x, outs = _Pad.apply(obs, T), []
    for k in range(K):
        y = model(x)
        o, x = _Roll.apply(x, y, Tin, min(Tout, H - k * Tout), k == K - 1)
        outs.append(o)
        if k + 1 < K:
            x = _force(x, truth, mask[k + 1], T, Tin, k + 1, [fmap])
    return torch.cat(outs, 1)


def teacher_loop_pair(model, obs1, obs2, H, truth, mask):
    """rollout_helper.rollout_loop_pair with ``mask`` [K, 2 N]; the second half
    reads ``truth`` [N, Ttot, V, 3] backwards from its last frame."""
    Tin, n = obs1.shape[1], obs1.shape[0]
    T = Tin + model.output_time_frame
    Tout, K = T - Tin, windows(T, Tin, H)
    maps = [(0, 1), (truth.shape[1] - 1, -1)]
    xs, outs = [_Pad.apply(obs1, T), _Pad.apply(obs2, T)], ([], [])
    for k in range(K):
        ys = model.forward_pair(xs[0], xs[1])
        for h in range(2):
            o, xs[h] = _Roll.apply(xs[h], ys[h], Tin, min(Tout, H - k * Tout), k == K - 1)
            outs[h].append(o)
            if k + 1 < K:
                xs[h] = _force(xs[h], truth, mask[k + 1, h * n:(h + 1) * n], T, Tin, k + 1, [maps[h]])
    return torch.cat(outs[0], 1), torch.cat(outs[1], 1)


def mixed_mask(K, N, half=None):
    """A fixed [K, N] uint8 pattern in which every boundary (row >= 1) has forced
    and free samples, consecutive rows differ, and -- with ``half`` = N / 2 --
    the two halves of a pair differ on every row."""
    m = np.zeros((K, N), dtype=np.uint8)
    for k in range(K):
        for b in range(N):
            m[k, b] = (b + k + (1 if half and b >= half and half % 2 == 0 else 0)) % 2
    if half:
        for k in range(K):
            assert (m[k, :half] != m[k, half:]).any()
    for k in range(1, K):
        assert 0 < m[k].sum() < N
    return m
