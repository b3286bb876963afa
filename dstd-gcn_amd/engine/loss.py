"""Training loss and loss bookkeeping (reference engine/utils/loss.py).

``mpjpe_error_3d`` without joint weights runs forward and backward as HIP
kernels (dstd_mpjpe_fwd / dstd_mpjpe_bwd): a deterministic two-stage mean of
per-joint L2 distances, and its gradient (p - q) / ||p - q|| / K written
straight into the output-gradient buffer of the model's backward.

Joint weights (``use_weight: True``) and the other terms of the reference's
loss table -- ``tl2`` (transition_error_3d), ``cl1`` (mae_error_3d), ``cl2``
(mse_error_3d) -- go through include/dstd_gcn_loss.h: ``weighted_losses``
evaluates every configured term, for the batch and its time reversal
together, in one native forward (two launches) and one native backward (one
launch), reading the targets in place through a frame mapping.
"""
import ctypes

import numpy as np
import torch

import dstd_native as native


class AccumLoss(object):
    """Running sum / count / average of host floats (loss.py:7-21)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val_his = []
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val_his.append(val)
        self.sum += val
        self.count += n
        self.avg = self.sum / self.count


class DeviceAccum(object):
    """AccumLoss whose running sum stays on the GPU: ``update`` takes a 0-d
    device tensor and never synchronises; ``avg`` synchronises once."""

    def __init__(self, device):
        self.sum = torch.zeros((), dtype=torch.float64, device=device)
        self.count = 0

    def update(self, val, n=1):
        self.sum += val.detach().to(torch.float64)
        self.count += n

    @property
    def avg(self):
        return float(self.sum.item()) / self.count if self.count else 0.0


class _MPJPE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, targ):
        L = native.lib()
        dev = pred.device
        out = torch.empty((), dtype=torch.float32, device=dev)
        npts = pred.numel() // 3
        ws = native.workspace(dev, L.dstd_loss_workspace_bytes())
        code = L.dstd_mpjpe_fwd(native.ptr(pred, "pred"), native.ptr(targ, "targ"), npts, out.data_ptr(),
                                ws.data_ptr(), ws.numel(), native.stream_handle(dev))
        native.check(code, "dstd_mpjpe_fwd")
        ctx.save_for_backward(pred, targ)
        return out

    @staticmethod
    def backward(ctx, g):
        L = native.lib()
        pred, targ = ctx.saved_tensors
        dev = pred.device
        g = g.contiguous()
        dp = torch.empty_like(pred)
        code = L.dstd_mpjpe_bwd(native.ptr(pred, "pred"), native.ptr(targ, "targ"), pred.numel() // 3,
                                native.ptr(g, "grad"), 1.0, dp.data_ptr(), native.stream_handle(dev))
        native.check(code, "dstd_mpjpe_bwd")
        return dp, None


TERM_BITS = {"jl2": native.LOSS_JL2, "tl2": native.LOSS_TL2, "cl1": native.LOSS_CL1, "cl2": native.LOSS_CL2}


class JointWeights(object):
    """Validated joint weights on the device (``prepare_joint_weights``): what
    the training loop uploads once and hands to every step."""

    def __init__(self, dev_tensor):
        self.dev = dev_tensor

    def __len__(self):
        return self.dev.numel()


def prepare_joint_weights(joint_weights, device, n_joints=None, into=None):
    """numpy array / tensor of per-joint weights -> JointWeights on ``device``
    (fp32; the reference keeps the dtype of the numpy array).  Checked on the
    host first: 1-D, finite, non-negative, of length ``n_joints`` when that is
    given.  ``into``: an earlier result to overwrite in place when it fits (a
    captured training step keeps reading that buffer)."""
    if isinstance(joint_weights, JointWeights):
        w = joint_weights
        if n_joints is not None and len(w) != n_joints:
            raise ValueError(f"joint_weights: {len(w)} weights for {n_joints} joints")
        return w
    if torch.is_tensor(joint_weights):
        joint_weights = joint_weights.detach().cpu().numpy()
    host = torch.from_numpy(np.array(joint_weights, dtype=np.float32))  # (a copy: the caller's array stays its own)
    if host.dim() != 1 or (n_joints is not None and host.numel() != n_joints):
        raise ValueError(f"joint_weights: shape {tuple(host.shape)} for {n_joints} joints")
    if not bool(torch.isfinite(host).all()) or bool((host < 0).any()):
        raise ValueError("joint_weights: weights must be finite and non-negative")
    if into is not None and len(into) == host.numel() and into.dev.device == torch.device(device):
        into.dev.copy_(host)
        return into
    return JointWeights(host.to(device))


class LossSpec(object):
    """The configured loss lines in config order: ``pairs`` = [(term name,
    config weight), ...].  ``terms`` is the native bitmask; ``matrix(device)``
    the [n_lines][LOSS_NTERMS] table holding line i's weight in the column of
    its term, uploaded once per device."""

    def __init__(self, pairs):
        self.pairs = [(name, float(w)) for name, w in pairs]
        for name, _ in self.pairs:
            if name not in TERM_BITS:
                raise NotImplementedError(f"loss '{name}' is not built")
        self.terms = 0
        for name, _ in self.pairs:
            self.terms |= TERM_BITS[name]
        self._matrix = {}

    def matrix(self, device):
        key = str(device)
        if key not in self._matrix:
            m = torch.zeros(len(self.pairs), native.LOSS_NTERMS, dtype=torch.float32)
            for i, (name, w) in enumerate(self.pairs):
                m[i, TERM_BITS[name].bit_length() - 1] = w
            self._matrix[key] = m.to(device)
        return self._matrix[key]


def _problems(preds, targets, maps):
    arr = (native.LossProblem * len(preds))()
    for q, p, (t0, step) in zip(arr, preds, maps):
        n, t, vc = p.shape
        q.pred, q.targ = native.ptr(p, "outputs"), native.ptr(targets, "targets")
        q.B, q.T, q.V = n, t, vc // 3
        q.targ_T, q.targ_t0, q.targ_step = targets.shape[1], t0, step
    return arr


class _Losses(torch.autograd.Function):
    """out[p][i] = config weight i x its term on problem p (prediction p against
    ``targets`` through frame map p), all from one dstd_losses_fwd; backward is
    one dstd_losses_bwd writing every prediction's gradient."""

    @staticmethod
    def forward(ctx, spec, targets, maps, w, *preds):
        L = native.lib()
        dev = preds[0].device
        values = torch.empty((len(preds), native.LOSS_NTERMS), dtype=torch.float32, device=dev)
        ws = native.workspace(dev, L.dstd_losses_workspace_bytes())
        code = L.dstd_losses_fwd(_problems(preds, targets, maps), len(preds), spec.terms,
                                 w.data_ptr() if w is not None else None, values.data_ptr(), ws.data_ptr(),
                                 ws.numel(), native.stream_handle(dev))
        native.check(code, "dstd_losses_fwd")
        ctx.spec, ctx.maps, ctx.n = spec, maps, len(preds)
        ctx.save_for_backward(targets, *([w] if w is not None else []), *preds)
        return (values.unsqueeze(1) * spec.matrix(dev)).sum(-1)

    @staticmethod
    def backward(ctx, g):
        L = native.lib()
        saved = ctx.saved_tensors
        targets, preds = saved[0], saved[len(saved) - ctx.n:]
        w = saved[1] if len(saved) - ctx.n == 2 else None
        dev = targets.device
        # coef[p][k] = sum over the lines of term k of upstream gradient x config weight
        coef = (g.unsqueeze(-1) * ctx.spec.matrix(dev)).sum(1).contiguous()
        dps = [torch.empty_like(p) for p in preds]
        ptrs = (ctypes.c_void_p * ctx.n)(*[d.data_ptr() for d in dps])
        code = L.dstd_losses_bwd(_problems(preds, targets, ctx.maps), ctx.n, ctx.spec.terms,
                                 w.data_ptr() if w is not None else None, coef.data_ptr(), 1.0, ptrs,
                                 native.stream_handle(dev))
        native.check(code, "dstd_losses_bwd")
        return (None, None, None, None, *dps)


def weighted_losses(spec, preds, targets, maps=None, joint_weights=None):
    """Every line of ``spec`` on every prediction in ``preds`` (one, or the
    batch's and its time reversal's) against ``targets`` [n][targ_T][V*3]:
    a [len(preds)][n_lines] fp32 device tensor of config weight x term.

    ``maps[p]`` = (targ_t0, targ_step) pairs prediction p's frame s with target
    frame targ_t0 + targ_step * s; the default pairs the last frames of
    ``targets`` in order (``targets[:, -t:]``)."""
    preds = list(preds)
    if not 1 <= len(preds) <= 2:
        raise ValueError(f"weighted_losses: {len(preds)} predictions (1 or 2)")
    n, t_all, vc = targets.shape
    if maps is None:
        maps = [(t_all - p.shape[1], 1) for p in preds]
    for p, (t0, step) in zip(preds, maps):
        if p.dim() != 3 or p.shape[0] != n or p.shape[2] != vc or vc % 3 or step not in (1, -1) or not (
                0 <= t0 < t_all and 0 <= t0 + step * (p.shape[1] - 1) < t_all):
            raise ValueError(f"weighted_losses: outputs {tuple(p.shape)} at frames ({t0}, {step}) of targets "
                             f"{tuple(targets.shape)}")
        if spec.terms & native.LOSS_TL2 and p.shape[1] < 2:
            raise ValueError("tl2 needs at least two frames")
    w = None
    if joint_weights is not None:
        w = prepare_joint_weights(joint_weights, preds[0].device, vc // 3).dev
    for p in preds:
        native.require_device(p, "outputs")
    native.require_device(targets, "targets")
    return _Losses.apply(spec, targets.contiguous(), tuple(maps), w, *(p.contiguous() for p in preds))


_SINGLE = {name: LossSpec([(name, 1.0)]) for name in TERM_BITS}


def _single(name, outputs, targets, joint_weights):
    if outputs.dim() != 3 or targets.shape != outputs.shape or outputs.shape[2] % 3:
        raise ValueError(f"{name}: shapes {tuple(outputs.shape)} vs {tuple(targets.shape)}")
    return weighted_losses(_SINGLE[name], [outputs], targets, None, joint_weights)[0, 0]


def mpjpe_error_3d(outputs, targets, joint_weights=None):
    """Mean per-joint position error (loss.py:52-65).

    With ``joint_weights=None`` (every shipped config: ``use_weight: False``)
    the reference's all-ones weight broadcast makes this the plain mean of the
    per-joint L2 distances over (n, t, joint).  With weights w it is
    mean(w) * mean(w_j ||p - q||): the reference multiplies the flattened norms
    by the [1][V][1] weights once more, which broadcasts to a mean over w."""
    if joint_weights is not None:
        return _single("jl2", outputs, targets, joint_weights)
    n, t, vc = outputs.shape
    if targets.shape != outputs.shape or vc % 3:
        raise ValueError(f"mpjpe_error_3d: shapes {tuple(outputs.shape)} vs {tuple(targets.shape)}")
    native.require_device(outputs, "outputs")
    native.require_device(targets, "targets")
    return _MPJPE.apply(outputs.contiguous(), targets.contiguous())


def transition_error_3d(outputs, targets, joint_weights=None):
    """Weighted mean L2 error of the frame-to-frame differences
    (loss.py:129-146), with the same mean(w) factor as mpjpe_error_3d."""
    return _single("tl2", outputs, targets, joint_weights)


def mae_error_3d(outputs, targets, joint_weights=None):
    """Weighted mean absolute coordinate error (loss.py:24-35)."""
    return _single("cl1", outputs, targets, joint_weights)


def mse_error_3d(outputs, targets, joint_weights=None):
    """The reference's ``cl2`` (loss.py:38-49): mean of sqrt((w d)^2), the value
    of mae_error_3d.  Its gradient is mae_error_3d's too -- 0 where w d == 0,
    where the reference's autograd returns NaN."""
    return _single("cl2", outputs, targets, joint_weights)


LOSSES = {"jl2": mpjpe_error_3d, "tl2": transition_error_3d, "cl1": mae_error_3d, "cl2": mse_error_3d}
