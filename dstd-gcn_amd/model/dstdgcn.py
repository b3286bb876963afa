"""DSTD-GCN modules backed by the MI355X kernels.

Drop-in replacements for the reference's ``model/dstdgcn.py``: the same class
names, constructor signatures, sub-module names, parameter names / shapes /
registration order (so ``state_dict`` keys and optimizer state line up with
checkpoints of the reference), the same initialisation and the same A_s/R_s
storage alias (reference :107-109).  Forward passes run through the C ABI in
include/dstd_gcn.h:

  DSTDGC.forward   -> dstd_dstdgc_fwd   (reference :80-94)
  DSTDGCB.forward  -> dstd_block_fwd    (reference :141-163)
  DSTDGCN.forward  -> dstd_model_fwd    (reference :293-317)

Training runs through include/dstd_gcn_train.h:

  DSTDGC  with autograd       -> dstd_dstdgc_train_fwd / _bwd
  DSTDGCB in train mode       -> dstd_block_train_fwd / _bwd (batch-stat BN)
  DSTDGCN in train mode       -> dstd_model_train_fwd / _bwd

each wrapped in a torch.autograd.Function whose backward is the native
backward, with the reference's gradient semantics (A_s / A_t constant, R_s
aliasing A_s's storage, alpha_sm shared by both spatial convs).

There is no CPU / eager fallback: a tensor off the GPU or a missing library
raises.  An eval-mode DSTDGCB / DSTDGCN forward that autograd will
differentiate (grad enabled and an input or parameter requiring grad) runs
the native training path with BatchNorm on its running statistics
(include/dstd_gcn_train.h DSTD_TRAIN_RUNNING_STATS), as the reference
back-propagates through its eval-mode modules; under torch.no_grad() (or
with frozen parameters and input) eval runs the fused inference kernels.
"""
import collections
import itertools
import numbers
import operator
import math
import weakref
from typing import List, Tuple

import numpy as np
import torch
import torch.nn as nn

import dstd_native as native

from .layers.graph import Graph
from .layers.time import Time


def conv_init(conv):
    """kaiming-normal fan_out weights, zero bias (reference :14-18)."""
    if conv.weight is not None:
        nn.init.kaiming_normal_(conv.weight, mode="fan_out")
    if conv.bias is not None:
        nn.init.constant_(conv.bias, 0)


def bn_init(bn, scale):
    nn.init.constant_(bn.weight, scale)
    nn.init.constant_(bn.bias, 0)


def weights_init(m):
    """Applied by ST_GCNN_layer to every Conv* module (reference :26-32)."""
    if "Conv" in type(m).__name__ and isinstance(getattr(m, "weight", None), torch.Tensor):
        nn.init.kaiming_normal_(m.weight, mode="fan_out")
        if isinstance(getattr(m, "bias", None), torch.Tensor):
            nn.init.constant_(m.bias, 0)


class _ForwardOnly(torch.autograd.Function):
    """Empty-batch outputs: forward is identity, backward gives the zero
    gradients torch's own ops would (nothing flows through an empty batch)."""

    @staticmethod
    def forward(ctx, y, *deps):
        ctx.shapes = [(d.shape, d.dtype, d.device) for d in deps]
        return y

    @staticmethod
    def backward(ctx, dy, *rest):
        return (dy, *[torch.zeros(sh, dtype=dt, device=dev) for sh, dt, dev in ctx.shapes])


# Native modules carry an instance token that is never reused (unlike id()):
# part of the constant-reuse tag of DSTDGCN, and the key under which the
# torch.library ops below find the module that lays out their C parameter
# struct.  Copies (deepcopy / unpickling) get a token of their own.
_UIDS = itertools.count(1)
_INSTANCES = weakref.WeakValueDictionary()


def _register(mod):
    mod._dstd_uid = next(_UIDS)
    _INSTANCES[mod._dstd_uid] = mod


class _NativeModule(nn.Module):
    # extra per-call launch-schedule flags of the eval forwards (include/dstd_gcn.h
    # DSTD_FWD_SEPARATE_ADJ / DSTD_FWD_FUSED_TEMPORAL: same results, for tests and A/B)
    _dstd_fwd_flags = 0

    def __setstate__(self, state):
        super().__setstate__(state)
        _register(self)

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        _bump_epoch()  # may have put new Parameter objects into _parameters
        return out


def invalidate_native_cache(module):
    """Force the next eval forward of every native module in ``module``'s tree
    to refold its constants.  Needed after writes the version counters do not
    see: through ``.data``, by collectives (dstd_dist.broadcast_module calls
    it), or by foreign kernels.  In-place torch ops, optimizer steps,
    ``load_state_dict`` and ``.to()`` are detected without it."""
    for m in module.modules():
        if hasattr(m, "_dstd_gen"):
            m._dstd_gen += 1


def _mark(y, *deps):
    if torch.is_grad_enabled():
        req = [d for d in deps if isinstance(d, torch.Tensor) and d.requires_grad]
        if req:
            return _ForwardOnly.apply(y, *req)
    return y


# Structure epoch: bumped by torch's global registration hooks whenever ANY
# module registers (or replaces) a parameter, buffer or submodule -- the
# assignments nn.Module.__setattr__ / register_* make -- and by
# _NativeModule._apply (.to(), .cuda(), .float() may put new Parameter objects
# straight into _parameters).  A cached walk of a native module tree is valid
# while the epoch it was taken at is current: an O(1) check per call instead
# of one identity check per (module, name, tensor) entry.
_STRUCT_EPOCH = [0]


def _bump_epoch(*args, **kwargs):
    _STRUCT_EPOCH[0] += 1


for _reg in ("register_module_parameter_registration_hook", "register_module_buffer_registration_hook",
             "register_module_module_registration_hook"):
    getattr(torch.nn.modules.module, _reg)(_bump_epoch)


def _hook_swap_tensor():
    """torch.func.functional_call and torch.nn.utils.stateless swap tensors
    into ``module._parameters`` / ``_buffers`` directly (the accessor's
    swap_tensor), past the registration hooks: bump the epoch there too, so a
    cached walk never hands the native kernels the module's own tensors in
    place of the swapped-in ones."""
    import torch.nn.utils._named_member_accessor as acc
    orig = acc.swap_tensor
    if getattr(orig, "_dstd_epoch", False):
        return

    def swap_tensor(*args, **kwargs):
        _STRUCT_EPOCH[0] += 1
        return orig(*args, **kwargs)

    swap_tensor._dstd_epoch = True
    acc.swap_tensor = swap_tensor


_hook_swap_tensor()


class _TensorTree:
    """``list(root.parameters())`` and ``list(root.buffers())`` without
    torch's generator walk of the module tree (~1.3 ms for DSTDGCN's ~350
    modules, paid per forward and per backward).  The walk is reused while the
    structure epoch it was taken at is current (no module anywhere registered
    or replaced a parameter, buffer or submodule since); a stale epoch falls
    back to checking every (parent, name, child) edge and (module, name,
    tensor) entry the walk saw, and walks again only if one of them changed."""

    def __init__(self):
        self.edges = self.pents = self.bents = None
        self.params = self.buffers = None
        self.epoch = -1

    def _walk(self, root):
        mods, edges, seen = [], [], set()

        def rec(mod):
            seen.add(id(mod))
            mods.append(mod)
            for name, child in mod._modules.items():
                edges.append((mod, name, child))
                if child is not None and id(child) not in seen:
                    rec(child)

        rec(root)
        pents, bents, params, buffers, ps, bs = [], [], [], [], set(), set()
        for md in mods:  # Module.parameters() order: modules pre-order, then insertion order
            for name, t in md._parameters.items():
                pents.append((md, name, t))
                if t is not None and id(t) not in ps:
                    ps.add(id(t))
                    params.append(t)
        for md in mods:
            for name, t in md._buffers.items():
                bents.append((md, name, t))
                if t is not None and id(t) not in bs:
                    bs.add(id(t))
                    buffers.append(t)
        self.edges, self.pents, self.bents, self.params, self.buffers = edges, pents, bents, params, buffers
        self.mods = mods
        self.counts = [(m, len(m._modules), len(m._parameters), len(m._buffers)) for m in mods]

    def _valid(self, root):
        return (self.edges is not None and self.mods[0] is root
                and all(len(m._modules) == a and len(m._parameters) == b and len(m._buffers) == c
                        for m, a, b, c in self.counts)
                and all(m._modules[n] is c for m, n, c in self.edges)
                and all(m._parameters[n] is t for m, n, t in self.pents)
                and all(m._buffers[n] is t for m, n, t in self.bents))

    def get(self, root):
        if self.epoch == _STRUCT_EPOCH[0] and self.mods[0] is root:
            return self.params, self.buffers
        if not self._valid(root):
            self._walk(root)
        self.epoch = _STRUCT_EPOCH[0]
        return self.params, self.buffers


_DATA_PTR = torch.Tensor.data_ptr
_VERSION = operator.attrgetter("_version")


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in ts)


def _bn_modules(module):
    """The BatchNorm1d modules of ``module``'s tree; the walk (~1.4 ms on
    DSTDGCN) is cached on the module for the current structure epoch."""
    c = module.__dict__.get("_dstd_bn_cache")
    if c is not None and c[0] == _STRUCT_EPOCH[0]:
        return c[1]
    bns = [m for m in module.modules() if isinstance(m, nn.BatchNorm1d)]
    module.__dict__["_dstd_bn_cache"] = (_STRUCT_EPOCH[0], bns)
    return bns


def _bn_momentum(module):
    moms = {m.momentum for m in _bn_modules(module)}
    if len(moms) != 1 or None in moms:
        raise NotImplementedError(f"native train-mode BN needs one fixed momentum for every BatchNorm, got {moms}")
    return float(moms.pop())


def _count_batch(module, calls=1):
    """nn.BatchNorm1d bumps num_batches_tracked once per train forward
    (``calls``: a forward pair counts as two)."""
    t = [m.num_batches_tracked for m in _bn_modules(module) if m.num_batches_tracked is not None]
    if t:
        torch._foreach_add_(t, calls)


def _op_train_fwd_native(mod, mode, x, A, alpha):
    L = native.lib()
    B, cin, T, V = x.shape
    dev = x.device
    cout, red = mod.out_channels, mod.red_channels
    y = torch.empty(B, cout, T, V, dtype=torch.float32, device=dev)
    nbytes = L.dstd_dstdgc_train_saved_bytes_r(mode, B, cin, cout, T, V, red)
    saved = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    code = L.dstd_dstdgc_train_fwd_r(mode, native.ptr(x, "x"), B, cin, cout, T, V, red, native.gc_weights(mod),
                                     native.ptr(A, "A"), native.ptr(alpha, "alpha_m"), native.ptr(y, "y"),
                                     saved.data_ptr(), nbytes, native.stream_handle(dev))
    native.check(code, "dstd_dstdgc_train_fwd_r")
    return y, saved


class _OpTrain(torch.autograd.Function):
    """DSTDGC forward + native backward (reference :80-94 under autograd);
    both directions are torch.library ops (dstd::dstdgc_train_forward /
    dstdgc_train_backward, below)."""

    @staticmethod
    def forward(ctx, mod, mode, x, A, alpha, *params):
        y, saved = torch.ops.dstd.dstdgc_train_forward(x, A, alpha, list(params), mod._dstd_uid)
        ctx.mod, ctx.saved_buf = mod, saved
        ctx.params = list(params)
        ctx.save_for_backward(x, A, alpha)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, A, alpha = ctx.saved_tensors
        need_dx = bool(ctx.needs_input_grad[2])
        dx, dA, dalpha, flat = torch.ops.dstd.dstdgc_train_backward(x, A, alpha, ctx.saved_buf, dy.contiguous(),
                                                                    ctx.params, ctx.mod._dstd_uid, need_dx)
        ctx.saved_buf = None
        arena = native.GradArena(ctx.params, x.device, buf=flat)
        return (None, None, dx if need_dx else None, dA, dalpha, *arena.views())


def _bn_flags(module):
    """Batch statistics in train mode; the running statistics, not updated,
    under .eval() (an eval-mode forward that autograd differentiates)."""
    return 0 if module.training else native.TRAIN_RUNNING_STATS


def _block_train_fwd_native(blk, x, flags, momentum):
    L = native.lib()
    B, cin, T, V = x.shape
    dev = x.device
    y = torch.empty(B, blk.out_channels, T, V, dtype=torch.float32, device=dev)
    nbytes = L.dstd_block_train_saved_bytes(B, cin, blk.out_channels, T, V)
    saved = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    code = L.dstd_block_train_fwd_ex(native.block_struct(blk), native.ptr(x, "x"), B, T, V, momentum,
                                     native.ptr(y, "y"), saved.data_ptr(), nbytes, native.stream_handle(dev), flags)
    native.check(code, "dstd_block_train_fwd_ex")
    return y, saved


def _block_train_bwd_native(blk, x, saved, dy, flags, arena, need_dx):
    L = native.lib()
    B, cin, T, V = x.shape
    dev = x.device
    dx = torch.zeros_like(x) if need_dx else None
    ws = native.workspace(dev, L.dstd_block_train_workspace_bytes(B, cin, blk.out_channels, T, V))
    code = L.dstd_block_train_bwd_ex(native.block_struct(blk), native.ptr(x, "x"), B, T, V, saved.data_ptr(),
                                     saved.numel(), native.ptr(dy, "dy"), dx.data_ptr() if dx is not None else None,
                                     native.block_grads(blk, arena), ws.data_ptr(), ws.numel(),
                                     native.stream_handle(dev), flags)
    native.check(code, "dstd_block_train_bwd_ex")
    return dx


def _model_train_fwd_native(model, x, flags, momentum, drop, seed):
    L = native.lib()
    n, t, v, c = x.shape
    dev = x.device
    y = torch.empty_like(x)
    nbytes = L.dstd_model_train_saved_bytes(n, t, v, model.num_feature, model.num_layers)
    saved = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    args = (model._native_params(), native.ptr(x, "x"), n, momentum, drop, seed, native.ptr(y, "y"),
            saved.data_ptr(), nbytes, native.stream_handle(dev), flags)
    sync = _bn_sync(model, flags)
    if sync is not None:  # cross-rank BatchNorm (dstd_dist.convert_sync_batchnorm)
        native.check(L.dstd_model_train_fwd_sync(*args, sync), "dstd_model_train_fwd_sync")
    else:
        native.check(L.dstd_model_train_fwd_ex(*args), "dstd_model_train_fwd_ex")
    return y, saved


def _bn_sync(model, flags):
    """The model's dstd_bn_sync (dstd_dist.BnSync) when its BatchNorms run on
    batch statistics; None for per-rank BatchNorm or running statistics."""
    s = model.__dict__.get("_dstd_bn_sync")
    if s is None or flags & native.TRAIN_RUNNING_STATS:
        return None
    return s.struct_ref()


def _model_train_bwd_native(model, x, saved, dy, flags, drop, seed, g, need_dx):
    L = native.lib()
    n, t, v, c = x.shape
    dev = x.device
    ws = native.workspace(dev, L.dstd_model_train_workspace_bytes(n, t, v, model.num_feature, model.num_layers))
    dx = torch.empty_like(x) if need_dx else None
    args = (model._native_params(), native.ptr(x, "x"), n, drop, seed, saved.data_ptr(), saved.numel(),
            native.ptr(dy, "dy"), g, dx.data_ptr() if dx is not None else None, ws.data_ptr(), ws.numel(),
            native.stream_handle(dev), flags)
    sync = _bn_sync(model, flags)
    if sync is not None:
        native.check(L.dstd_model_train_bwd_sync(*args, sync), "dstd_model_train_bwd_sync")
    else:
        native.check(L.dstd_model_train_bwd_ex(*args), "dstd_model_train_bwd_ex")
    return dx


class _BlockTrain(torch.autograd.Function):
    """DSTDGCB forward + native backward (reference :141-163): train-mode BN,
    or running-statistics BN for an eval-mode block under autograd.  Both
    directions are torch.library ops (dstd::dstdgcb_train_forward /
    dstdgcb_train_backward, below) over the C ABI."""

    @staticmethod
    def forward(ctx, blk, x, *params):
        flags = _bn_flags(blk)
        y, saved = torch.ops.dstd.dstdgcb_train_forward(x, list(params), list(blk.buffers()), blk._dstd_uid, flags,
                                                        _bn_momentum(blk))
        if not flags:
            _count_batch(blk)
        ctx.blk, ctx.saved_buf, ctx.flags = blk, saved, flags
        ctx.params = list(params)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        need_dx = bool(ctx.needs_input_grad[1])
        dx, flat = torch.ops.dstd.dstdgcb_train_backward(x, ctx.saved_buf, dy.contiguous(), ctx.params,
                                                         ctx.blk._dstd_uid, ctx.flags, need_dx)
        ctx.saved_buf = None
        arena = native.GradArena(ctx.params, x.device, buf=flat)
        return (None, dx if need_dx else None, *arena.views())


@torch._dynamo.disable
def _host_seed(model):
    """A dropout seed for the op branch of _ModelTrain: an integer drawn on
    the host at run time (under torch.compile this is a graph break, not a
    traced random value -- dynamo would turn one into a tensor, which the ops'
    integer `seed` cannot take).  Taken from the model device's generator --
    the one the eager branch draws its device seed from -- as its (seed,
    philox offset) pair, whose offset it then advances as one device draw
    would: torch.manual_seed makes compiled training with dropout
    reproducible, compiled and eager steps consume the same stream, and the
    global CPU stream (samplers, DataLoader base seeds) is not touched
    (ADVICE r05)."""
    dev = next(model.parameters()).device
    g = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    seed, off = g.initial_seed(), g.get_offset()
    g.set_offset(off + 4)
    return (seed * 0x9E3779B97F4A7C15 + (off + 1) * 0xBF58476D1CE4E5B9) % (2 ** 62)


class _ModelTrain(torch.autograd.Function):
    """DSTDGCN forward + native backward (reference :293-317): train mode, or
    an eval-mode model under autograd (running-statistics BN, no dropout).
    Both directions are torch.library ops (dstd::dstdgcn_train_forward /
    dstdgcn_train_backward, below) over the C ABI; eager forwards call the
    forward op's implementation directly (as the eval forward does), and the
    opt-in in-place gradient arena calls the C ABI directly (it writes .grad
    as a side effect, which an op cannot)."""

    @staticmethod
    def forward(ctx, model, paired, x, *params):
        # paired: x is two train-mode batches of B/2 (DSTDGCN.forward_pair)
        flags = _bn_flags(model) | (native.TRAIN_PAIRED if paired else 0)
        if getattr(model, "_dstd_one_stream", False):  # the backward's launches all on the caller's stream
            flags |= native.TRAIN_ONE_STREAM
        drop = float(model.do_in.p) if model.do_in.training else 0.0
        seed, ctx.seed_t = 0, None
        eager = type(x) is torch.Tensor and not torch.compiler.is_compiling()
        if drop > 0 and eager:
            # the dropout seed is drawn on the device and read there
            # (DSTD_TRAIN_SEED_DEVICE): no host round trip, and a captured HIP
            # graph (engine.GraphedStep) draws a fresh mask per replay; the
            # tensor lives in ctx until the backward has regenerated the mask
            ctx.seed_t = torch.randint(0, 2 ** 62, (1,), device=x.device, dtype=torch.int64)
            seed = ctx.seed_t.data_ptr()
            flags |= native.TRAIN_SEED_DEVICE
        elif drop > 0:
            # the op branch (torch.compile, subclass inputs): the ops' schema
            # carries the seed as an integer, so it is drawn on the host -- a
            # device tensor read by pointer would be invisible to the tracer
            # (and a FakeTensor has no data pointer).  Drawn outside the traced
            # region (_host_seed), so it stays an integer and every compiled call
            # gets a new mask
            seed = _host_seed(model)
        buffers = model._tree.get(model)[1]
        if eager:
            # eager: the op's implementation without the dispatcher's boxing
            # of ~300 tensor arguments (~0.3 ms of host time per step); the
            # running statistics it updates get the version bump the op's
            # mutates_args declares (the eval forward's constant cache keys
            # on versions)
            y, saved = _model_train_fwd_native(model, x, flags, _bn_momentum(model), drop, seed)
            if not flags & native.TRAIN_RUNNING_STATS:
                torch.autograd.graph.increment_version(buffers)
        else:
            y, saved = torch.ops.dstd.dstdgcn_train_forward(x, list(params), buffers, model._dstd_uid,
                                                            flags, _bn_momentum(model), drop, seed)
        if not flags & native.TRAIN_RUNNING_STATS:
            _count_batch(model, 2 if paired else 1)
        ctx.model, ctx.saved_buf, ctx.drop, ctx.seed, ctx.flags = model, saved, drop, seed, flags
        # anchored (_anchor_of): the parameters are not the Function's inputs
        ctx.anchored = len(params) == 1 and params[0] is getattr(model, "_dstd_anchor_t", None)
        # the backward reuses them (a module walk costs ~0.7 ms)
        ctx.params = model._tree.get(model)[0] if ctx.anchored else list(params)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        model = ctx.model
        dev = x.device
        dy = dy.contiguous()
        need_dx = bool(ctx.needs_input_grad[2])
        # gradients accumulate straight into the parameters' .grad (one arena,
        # native +=) when the caller opted in (engine.PredictionEngine.train
        # sets model._dstd_inplace_grads) and no parameter carries hooks; else
        # the backward op fills a fresh arena whose views autograd accumulates
        # (hooks, DDP and torch.autograd.grad see ordinary gradients)
        if ctx.anchored or (getattr(model, "_dstd_inplace_grads", False) and not any(
                p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None) for p in ctx.params)):
            arena, direct = native.grad_sink(model, ctx.params, dev)
            if direct:
                g = getattr(arena, "model_grads", None)
                if g is None:  # the persistent arena: its pointer table is reused
                    g = arena.model_grads = model._native_grads(arena)
                dx = _model_train_bwd_native(model, x, ctx.saved_buf, dy, ctx.flags, ctx.drop, ctx.seed, g, need_dx)
                ctx.saved_buf = ctx.seed_t = None
                return (None, None, dx, *([None] * (1 if ctx.anchored else len(arena.params))))
        dx, flat = torch.ops.dstd.dstdgcn_train_backward(x, ctx.saved_buf, dy, ctx.params, model._dstd_uid, ctx.flags,
                                                         ctx.drop, ctx.seed, need_dx)
        ctx.saved_buf = ctx.seed_t = None
        arena = native.GradArena(ctx.params, dev, buf=flat)
        if ctx.anchored:
            # .grad was set by someone else since the forward: accumulate as
            # autograd's AccumulateGrad would (no hooks: _anchor_of checked)
            for p, v in zip(arena.params, arena.views()):
                if v is not None and p.requires_grad:
                    if p.grad is None:
                        p.grad = v.clone()
                    else:
                        p.grad.add_(v)
            return (None, None, dx if need_dx else None, None)
        return (None, None, dx if need_dx else None, *arena.views())


def _anchor_of(model, x, params):
    """The Function's parameter inputs for a train-mode call: ``params``, or
    -- in the opt-in in-place gradient mode (model._dstd_inplace_grads, set by
    engine.PredictionEngine.train), eager, no parameter hooks -- one empty
    leaf that requires grad standing in for all of them.  The backward writes
    the parameters' .grad itself in that mode (native.grad_sink) and returns
    None for each of them, so autograd needs no edge per parameter: ~300
    inputs cost the host ~1 ms per step in Function.apply and the engine's
    walk of the backward graph (measured on this container's CPU: 1.9 ms
    against 0.1 ms for a 2-output Function with 300 vs 1 input)."""
    if not (getattr(model, "_dstd_inplace_grads", False) and torch.is_grad_enabled()
            and type(x) is torch.Tensor and not torch.compiler.is_compiling()):
        return params
    if not any(p.requires_grad for p in params) or any(
            p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None) for p in params):
        return params
    a = getattr(model, "_dstd_anchor_t", None)
    if a is None:
        a = model._dstd_anchor_t = torch.empty(0, requires_grad=True)
    return [a]


class _ModelTrainPair(torch.autograd.Function):
    """DSTDGCN.forward_pair's Function: _ModelTrain over the concatenated
    pair (DSTD_TRAIN_PAIRED) with the two halves as two outputs.  The backward
    joins their gradients with one copy; slicing one output instead left it to
    autograd's slice backward -- a zero-filled pair-sized buffer and a copy per
    half, then their sum (five launches and their host time per step)."""

    @staticmethod
    def forward(ctx, model, n, x, *params):
        y = _ModelTrain.forward(ctx, model, True, x, *params)
        return y[:n], y[n:]

    @staticmethod
    def backward(ctx, d1, d2):
        (x,) = ctx.saved_tensors
        n = x.shape[0] // 2
        if d1 is None:
            d1 = x.new_zeros((n,) + tuple(x.shape[1:]))
        if d2 is None:
            d2 = x.new_zeros((x.shape[0] - n,) + tuple(x.shape[1:]))
        # (argument positions: model, n, x, params -- as _ModelTrain's model, paired, x, params)
        return _ModelTrain.backward(ctx, torch.cat([d1, d2]))


def _param_hooks(params):
    return any(p._backward_hooks or getattr(p, "_post_accumulate_grad_hooks", None) for p in params)


# The three families of chain entry points (include/ext/dstd_gcn_rollout.h,
# dstd_gcn_teacher.h, dstd_gcn_stride_train.h), keyed by (stride is None,
# mask is None): the stem of _fwd / _bwd / _bwd_window, whether ``stride``
# follows ``horizon`` in their arguments (and the workspace is the strided
# one, sized by input_n and horizon too), and whether they take the teacher's
# five arguments -- NULL in a free-running strided chain.
_Chain = collections.namedtuple("_Chain", "stem strided teacher")
_CHAINS = {(True, True): _Chain("dstd_model_rollout", False, False),
           (True, False): _Chain("dstd_model_rollout_tf", False, True),
           (False, True): _Chain("dstd_model_rollout_strided", True, True),
           (False, False): _Chain("dstd_model_rollout_strided", True, True)}


class _RolloutChain(torch.autograd.Function):
    """DSTDGCN.rollout under autograd: the whole chain of train forwards as one
    native call and its backward as another (include/ext/dstd_gcn_rollout.h).
    Built like _ModelTrain -- flags, device seeds, the anchored parameters and
    the in-place gradient arena -- but eager only: there is no custom op for
    the chain, so both directions call the C ABI directly.

    One Function for every chain.  ``stride`` None: whole windows; else every
    window hands on its first ``stride`` frames (a stride below
    ``output_time_frame``: include/ext/dstd_gcn_stride_train.h), and the chain
    has ``ceil(horizon / stride)`` windows.  ``mask`` None: free running
    (``teacher`` and ``maps`` are None too); else scheduled sampling
    (include/ext/dstd_gcn_teacher.h) with the teacher's frames, one (t0, step)
    frame map per half and the mask, which stays in ctx, since the backward
    reads it again; the teacher and the mask get no gradient.  Which entry
    points that makes, and how their arguments differ, is _CHAINS'."""

    @staticmethod
    def forward(ctx, model, paired, horizon, stride, obs, teacher, mask, maps, *params):
        L = native.lib()
        n, tin, v, c = obs.shape
        dev = obs.device
        t = tin + model.output_time_frame
        windows = -(-horizon // (stride or model.output_time_frame))
        chain = ctx.chain = _CHAINS[stride is None, mask is None]
        flags = _bn_flags(model) | (native.TRAIN_PAIRED if paired else 0)
        if getattr(model, "_dstd_one_stream", False):
            flags |= native.TRAIN_ONE_STREAM
        drop = float(model.do_in.p) if model.do_in.training else 0.0
        seeds, ctx.seed_t = None, None
        if drop > 0:
            # one device seed per window, drawn in one launch and read there
            # (DSTD_TRAIN_SEED_DEVICE); kept until the backward has regenerated the masks
            ctx.seed_t = torch.randint(0, 2 ** 62, (windows,), device=dev, dtype=torch.int64)
            seeds = ctx.seed_t.data_ptr()
            flags |= native.TRAIN_SEED_DEVICE
        params_all, buffers = model._tree.get(model)
        out = obs.new_empty(n, horizon, v, c)
        nbytes = L.dstd_model_rollout_saved_bytes(n, t, v, model.num_feature, model.num_layers, windows)
        saved = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ctx.mask = mask  # the backward reads it again
        ctx.tf = ()
        if mask is not None:
            ctx.tf = (native.ptr(teacher, "teacher"), teacher.shape[1], *native.ext.frame_maps(maps), mask.data_ptr())
        elif chain.teacher:
            ctx.tf = (None, 0, None, None, None)
        # (horizon[, stride]) as every entry point of the family takes them
        ctx.span = (horizon, stride) if chain.strided else (horizon,)
        code = getattr(L, chain.stem + "_fwd")(native.ext.model_params_ref(model._native_params()),
                                               native.ptr(obs, "observed"), n, tin, *ctx.span, _bn_momentum(model),
                                               drop, seeds, native.ptr(out, "out"), saved.data_ptr(), nbytes, *ctx.tf,
                                               native.stream_handle(dev), flags)
        native.check(code, chain.stem + "_fwd")
        if not flags & native.TRAIN_RUNNING_STATS:
            # the running statistics were updated once per window (twice when paired)
            torch.autograd.graph.increment_version(buffers)
            _count_batch(model, windows * (2 if paired else 1))
        ctx.model, ctx.saved_buf, ctx.drop, ctx.flags, ctx.shape = model, saved, drop, flags, (n, tin, v, c)
        ctx.horizon, ctx.windows = horizon, windows
        ctx.anchored = len(params) == 1 and params[0] is getattr(model, "_dstd_anchor_t", None)
        ctx.params = params_all if ctx.anchored else list(params)
        return out

    @staticmethod
    def backward(ctx, dout):
        L = native.lib()
        model, chain, windows = ctx.model, ctx.chain, ctx.windows
        n, tin, v, c = ctx.shape
        dev = dout.device
        dout = dout.contiguous()
        need_dx = bool(ctx.needs_input_grad[4])
        if ctx.saved_buf is None:
            raise RuntimeError("DSTDGCN.rollout: backward through the chain a second time "
                               "(its saved windows were freed by the first)")
        arena, direct = None, False
        if ctx.anchored or (getattr(model, "_dstd_inplace_grads", False) and not _param_hooks(ctx.params)):
            arena, direct = native.grad_sink(model, ctx.params, dev)
        size = (n, tin + model.output_time_frame, v, model.num_feature, model.num_layers)
        if chain.strided:
            ws = native.workspace(dev, L.dstd_model_rollout_strided_workspace_bytes(*size, tin, ctx.horizon))
        else:
            ws = native.workspace(dev, L.dstd_model_rollout_workspace_bytes(*size))
        dobs = dout.new_empty(n, tin, v, c) if need_dx else None
        pref = native.ext.model_params_ref(model._native_params())
        tail = (ctx.drop, ctx.seed_t.data_ptr() if ctx.seed_t is not None else None, ctx.saved_buf.data_ptr(),
                ctx.saved_buf.numel(), native.ptr(dout, "dout"))
        tail2 = (dobs.data_ptr() if need_dx else None, ws.data_ptr(), ws.numel(), *ctx.tf, native.stream_handle(dev),
                 ctx.flags)
        if direct:
            # every window accumulates (+=) into the parameters' .grad, as the K
            # backwards of a loop do in this mode: one native call
            g = getattr(arena, "model_grads", None)
            if g is None:
                g = arena.model_grads = model._native_grads(arena)
            code = getattr(L, chain.stem + "_bwd")(pref, n, tin, *ctx.span, *tail, native.ext.model_grads_ref(g),
                                                   *tail2)
            native.check(code, chain.stem + "_bwd")
        else:
            # gradients for autograd: a zeroed arena per window, summed in backward
            # order (window K-1 first) -- what autograd makes of the K backwards of
            # a loop, each of which returns an arena of its own.  One (+=) chain
            # into a single arena would round alpha_sm, which both spatial
            # operators of a block add into, differently from that.
            numel = native.arena_numel(ctx.params)
            bufs = torch.zeros(windows, numel, dtype=torch.float32, device=dev)
            bwd_window = getattr(L, chain.stem + "_bwd_window")
            for k in range(windows - 1, -1, -1):
                g = model._native_grads(native.GradArena(ctx.params, dev, buf=bufs[k]))
                code = bwd_window(pref, n, tin, *ctx.span, k, *tail, native.ext.model_grads_ref(g), *tail2)
                native.check(code, chain.stem + "_bwd_window")
            total = bufs[windows - 1]
            for k in range(windows - 2, -1, -1):
                total += bufs[k]
            arena = native.GradArena(ctx.params, dev, buf=total)
        ctx.saved_buf = ctx.seed_t = ctx.mask = ctx.tf = None
        # model, paired, horizon, stride, obs, teacher, mask, maps
        head = (None, None, None, None, dobs, None, None, None)
        if direct:
            return (*head, *([None] * (1 if ctx.anchored else len(arena.params))))
        if ctx.anchored:
            # .grad was set by someone else since the forward (_ModelTrain.backward)
            for p, gv in zip(arena.params, arena.views()):
                if gv is not None and p.requires_grad:
                    if p.grad is None:
                        p.grad = gv.clone()
                    else:
                        p.grad.add_(gv)
            return (*head, None)
        return (*head, *arena.views())


class _RolloutChainPair(torch.autograd.Function):
    """DSTDGCN.rollout_pair's Function: _RolloutChain over the concatenated
    pair (DSTD_TRAIN_PAIRED) with the two halves as two outputs, as
    _ModelTrainPair."""

    @staticmethod
    def forward(ctx, model, n, horizon, stride, obs, teacher, mask, maps, *params):
        out = _RolloutChain.forward(ctx, model, True, horizon, stride, obs, teacher, mask, maps, *params)
        ctx.half = n
        return out[:n], out[n:]

    @staticmethod
    def backward(ctx, d1, d2):
        n2, tin, v, c = ctx.shape
        n = ctx.half
        ref = d1 if d1 is not None else d2
        if d1 is None:
            d1 = ref.new_zeros((n, ctx.horizon, v, c))
        if d2 is None:
            d2 = ref.new_zeros((n2 - n, ctx.horizon, v, c))
        # (argument positions: model, n, ... -- as _RolloutChain's model, paired, ...)
        return _RolloutChain.backward(ctx, torch.cat([d1, d2]))


class BatchNorm(nn.Module):
    """BN1d over C*V channels of an NCTV tensor (reference :35-50).  Glue only:
    on the hot path every BatchNorm is folded into a kernel epilogue."""

    def __init__(self, feature_channels, joint_dim, time_dim):
        super().__init__()
        self.c = feature_channels
        self.v = joint_dim
        self.t = time_dim
        self.bn = nn.BatchNorm1d(feature_channels * joint_dim)

    def forward(self, x):
        n, c, t, v = x.shape
        assert (c, t, v) == (self.c, self.t, self.v)
        y = self.bn(x.transpose(2, 3).reshape(n, c * v, t))
        return y.reshape(n, c, v, t).transpose(2, 3).contiguous()


class DSTDGC(_NativeModule):
    """Dynamic graph convolution (reference :53-94); ``mode`` spatial or temporal."""

    def __init__(self, in_channels, out_channels, ref_channels, kpt_channels, red_channels=2, mode="spatial"):
        super().__init__()
        if mode not in ("spatial", "temporal"):
            raise AssertionError(f"mode must be spatial or temporal, got {mode}")
        if not 1 <= red_channels <= 8:
            raise NotImplementedError(f"red_channels={red_channels}: this build covers 1..8 (every shipped config uses 2)")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.ref_channels = ref_channels
        self.kpt_channels = kpt_channels
        self.red_channels = red_channels
        self.mode = mode
        self.conv_m1 = nn.Conv2d(in_channels, red_channels, 1)
        self.conv_m2 = nn.Conv2d(in_channels, red_channels, 1)
        self.conv_rm = nn.Conv2d(red_channels * ref_channels, ref_channels, 1)
        self.tanh = nn.Tanh()
        self.conv_f = nn.Conv2d(in_channels, out_channels, 1)
        self.init_parameter()
        _register(self)

    def init_parameter(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                conv_init(m)

    def forward(self, x, A=None, alpha_m=1):
        L = native.lib()
        B, cin, T, V = x.shape
        if cin != self.in_channels:
            raise ValueError(f"DSTDGC: expected {self.in_channels} input channels, got {cin}")
        x = x.contiguous()
        native.require_device(x, "x")
        dev = x.device
        if B == 0:  # empty batch: empty output, as the reference's torch ops give
            return _mark(x.new_empty(0, self.out_channels, T, V), x)
        A = A.reshape(A.shape[-2], A.shape[-1]).contiguous()
        if not torch.is_tensor(alpha_m):
            alpha_m = torch.full((1,), float(alpha_m), dtype=torch.float32, device=dev)
        alpha = alpha_m.reshape(1).contiguous()
        mode = native.MODE_SPATIAL if self.mode == "spatial" else native.MODE_TEMPORAL
        params = list(self.parameters())
        if _needs_grad(x, A, alpha, *params):
            return _OpTrain.apply(self, mode, x, A, alpha, *params)
        return torch.ops.dstd.dstdgc_forward(x, A, alpha, params, self._dstd_uid)

    def _eval_native(self, x, A, alpha):
        """dstd_dstdgc_fwd on prepared operands (torch.ops.dstd.dstdgc_forward)."""
        L = native.lib()
        B, cin, T, V = x.shape
        dev = x.device
        mode = native.MODE_SPATIAL if self.mode == "spatial" else native.MODE_TEMPORAL
        if self.red_channels != 2:
            # the inference kernels carry exactly two P / Q channels; any other
            # red_channels runs the training forward (generic in it, exact fp32,
            # and the same function: DSTDGC has no BN or dropout)
            return _op_train_fwd_native(self, mode, x, A, alpha)[0]
        y = torch.empty(B, self.out_channels, T, V, dtype=torch.float32, device=dev)
        nbytes = L.dstd_dstdgc_workspace_bytes(mode, B, cin, self.out_channels, T, V)
        ws = native.workspace(dev, nbytes)
        w = native.gc_weights(self)
        code = L.dstd_dstdgc_fwd(mode, native.ptr(x, "x"), B, cin, self.out_channels, T, V, w,
                                 native.ptr(A, "A"), native.ptr(alpha, "alpha_m"), native.ptr(y, "y"),
                                 ws.data_ptr(), ws.numel(), native.stream_handle(dev))
        native.check(code, "dstd_dstdgc_fwd")
        return y


class DSTDGCB(_NativeModule):
    """DSTD-GC block: two spatial DSTDGCs on the skeleton priors, BN + residual
    + PReLU, one temporal DSTDGC (reference :97-163)."""

    def __init__(self, in_channels, out_channels, time_dim, joint_dim, layout="h36m"):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        A_s = Graph(layout).get_all_adjacency()
        A_t = Time(time_dim).get_all_adjacency()
        # registration order and the A_s/R_s alias follow the reference (:107-112)
        self.A_s = nn.Parameter(torch.tensor(A_s, dtype=torch.float32), False)
        self.W_s = nn.Parameter(torch.zeros_like(self.A_s))
        self.R_s = nn.Parameter(self.A_s.data)  # same storage as A_s
        self.A_t = nn.Parameter(torch.tensor(A_t, dtype=torch.float32), False)
        self.R_t = nn.Parameter(torch.zeros_like(self.A_t))
        self.conv_s = nn.ModuleList()
        self.conv_t = nn.ModuleList()
        if in_channels != out_channels:
            self.residual = nn.Sequential(nn.Conv2d(in_channels, out_channels, 1),
                                          BatchNorm(out_channels, joint_dim, time_dim))
        else:
            self.residual = lambda x: x
        for _ in range(A_s.shape[0]):
            self.conv_s.append(DSTDGC(in_channels, out_channels, time_dim, joint_dim, mode="spatial"))
        self.alpha_sm = nn.Parameter(torch.zeros(1))
        self.bn = BatchNorm(out_channels, joint_dim, time_dim)
        for _ in range(A_t.shape[0]):
            self.conv_t.append(DSTDGC(out_channels, out_channels, joint_dim, time_dim, mode="temporal"))
        self.alpha_tm = nn.Parameter(torch.zeros(1))
        self.prelu = nn.PReLU()
        self.do = nn.Dropout(0.1)  # constructed but never applied (reference :133)
        # arithmetic of the eval forward's graph convolutions, per call
        # (include/dstd_gcn.h DSTD_FWD_EXACT_FP32): "split" or "fp32"
        self.gc_arithmetic = "split"
        _register(self)

    def init_parameter(self):
        stdt = 1.0 / math.sqrt(self.R_t.size(1))
        self.R_t.data.uniform_(-stdt, stdt)
        stdt = 1.0 / math.sqrt(self.R_s.size(1))
        self.R_s.data.uniform_(-stdt, stdt)

    def forward(self, x):
        L = native.lib()
        B, cin, T, V = x.shape
        x = x.contiguous()
        native.require_device(x, "x")
        if B == 0 and not self.training:  # empty batch: empty output (reference torch semantics)
            return _mark(x.new_empty(0, self.out_channels, T, V), x, *self.parameters())
        params = list(self.parameters())
        if self.training or _needs_grad(x, *params):
            # train mode, or an eval-mode output autograd differentiates: the
            # native training path (running-statistics BN in eval mode)
            return _BlockTrain.apply(self, x, *params)
        tensors = params + list(self.buffers())
        # _dstd_fwd_flags: extra per-call schedule flags (tests / A-B: include/dstd_gcn.h DSTD_FWD_*)
        return torch.ops.dstd.dstdgcb_forward(x, tensors, self._dstd_uid, self.out_channels,
                                              native.arith_flags(self.gc_arithmetic) | self._dstd_fwd_flags)

    def _eval_native(self, x, flags):
        """dstd_block_fwd_ex (torch.ops.dstd.dstdgcb_forward)."""
        L = native.lib()
        B, cin, T, V = x.shape
        dev = x.device
        y = torch.empty(B, self.out_channels, T, V, dtype=torch.float32, device=dev)
        nbytes = L.dstd_block_workspace_bytes(B, cin, self.out_channels, T, V)
        ws = native.workspace(dev, nbytes)
        p = native.block_struct(self)
        code = L.dstd_block_fwd_ex(p, native.ptr(x, "x"), B, T, V, native.ptr(y, "y"), ws.data_ptr(), ws.numel(),
                                   native.stream_handle(dev), flags)
        native.check(code, "dstd_block_fwd_ex")
        return y

    def forward_taps(self, x, what=native.TAP_NAMES):
        """``(y, taps)``: the eval forward of ``x`` [N, cin, T, V] and what it
        computed on the way (include/dstd_gcn_taps.h) -- ``taps.adj_s``
        [N, 2, T, V, V] and ``taps.adj_t`` [N, V, T, T], the sample-wise
        graphs the graph convolutions contracted, ``taps.x`` the block's
        input and ``taps.h`` [N, cout, T, V] the temporal GC's input.
        ``what`` names the ones wanted; the others are None.  Eval mode only,
        no autograd; honours ``gc_arithmetic``.  Runs the unit-parallel launch
        schedule (one launch per adjacency and per GC); y equals ``self(x)``."""
        what = _tap_names(what)
        _taps_eval_only(self)
        L = native.lib()
        x = x.detach().contiguous()
        native.require_device(x, "x")
        B, cin, T, V = x.shape
        dev = x.device
        with torch.no_grad():
            y = torch.empty(B, self.out_channels, T, V, dtype=torch.float32, device=dev)
            taps, st = _alloc_taps(what, B, cin, self.out_channels, T, V, dev)
            if B == 0:
                return y, taps
            nbytes = L.dstd_block_taps_workspace_bytes(B, cin, self.out_channels, T, V)
            ws = native.workspace(dev, nbytes)
            code = L.dstd_block_fwd_taps(native.block_struct(self), native.ptr(x, "x"), B, T, V, native.ptr(y, "y"),
                                         st, ws.data_ptr(), ws.numel(), native.stream_handle(dev),
                                         native.arith_flags(self.gc_arithmetic))
        native.check(code, "dstd_block_fwd_taps")
        return y, taps


class Taps:
    """What ``forward_taps`` returns for one DSTDGCB: ``adj_s``, ``adj_t``,
    ``x``, ``h`` (detached tensors; None where not requested)."""
    __slots__ = native.TAP_NAMES

    def __init__(self):
        for n in native.TAP_NAMES:
            setattr(self, n, None)

    def __repr__(self):
        return "Taps(" + ", ".join(f"{n}={None if getattr(self, n) is None else list(getattr(self, n).shape)}"
                                   for n in native.TAP_NAMES) + ")"


def _tap_names(what):
    what = (what,) if isinstance(what, str) else tuple(what)
    for n in what:
        if n not in native.TAP_NAMES:
            raise ValueError(f"forward_taps: unknown tap {n!r} (one of {native.TAP_NAMES})")
    return what


def _taps_eval_only(module):
    if module.training:
        raise RuntimeError("forward_taps returns the eval forward's adjacencies and activations: call .eval() first")


def _alloc_taps(what, B, cin, cout, T, V, dev):
    """A Taps with a fresh output tensor per requested name and the C struct
    that points at them (native.BlockTaps)."""
    shapes = {"adj_s": (B, 2, T, V, V), "adj_t": (B, V, T, T), "x": (B, cin, T, V), "h": (B, cout, T, V)}
    taps, st = Taps(), native.BlockTaps()
    for n in what:
        t = torch.empty(shapes[n], dtype=torch.float32, device=dev)
        setattr(taps, n, t)
        setattr(st, n, t.data_ptr() if t.numel() else None)
    return taps, st


def _ptr_or_none(t):
    return t.data_ptr() if t is not None else None


class _CTGFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, Tm, A, A_fixed):
        L = native.lib()
        B, C, T, V = x.shape
        dev = x.device
        y = torch.empty_like(x)
        ws = native.workspace(dev, L.dstd_ctg_workspace_bytes(B, C, T, V))
        code = L.dstd_ctg_fwd(native.ptr(x, "x"), B, C, T, V, native.ptr(Tm, "T"), native.ptr(A, "A"),
                              native.ptr(A_fixed, "A_fixed"), native.ptr(y, "y"), ws.data_ptr(), ws.numel(),
                              native.stream_handle(dev))
        native.check(code, "dstd_ctg_fwd")
        ctx.save_for_backward(x, Tm, A, A_fixed)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = native.lib()
        x, Tm, A, A_fixed = ctx.saved_tensors
        B, C, T, V = x.shape
        dev = x.device
        dy = dy.contiguous()
        dx = torch.zeros_like(x) if ctx.needs_input_grad[0] else None
        dTm, dA = torch.zeros_like(Tm), torch.zeros_like(A)
        ws = native.workspace(dev, L.dstd_ctg_workspace_bytes(B, C, T, V))
        code = L.dstd_ctg_bwd(native.ptr(x, "x"), B, C, T, V, native.ptr(Tm, "T"), native.ptr(A, "A"),
                              native.ptr(A_fixed, "A_fixed"), native.ptr(dy, "dy"), _ptr_or_none(dx), dTm.data_ptr(),
                              dA.data_ptr(), ws.data_ptr(), ws.numel(), native.stream_handle(dev))
        native.check(code, "dstd_ctg_bwd")
        return dx, dTm, dA, None


class ConvTemporalGraphical(nn.Module):
    """Learnable temporal (T [V,T,T]) then spatial (A [T,V,V] + fixed skeleton)
    graph mixing (reference :166-188).  Only reachable through
    ST_GCNN_layer(refine=False), which no shipped config builds."""

    def __init__(self, time_dim, joints_dim, layout="h36m"):
        super().__init__()
        self.A = nn.Parameter(torch.FloatTensor(time_dim, joints_dim, joints_dim))
        stdv = 1.0 / math.sqrt(self.A.size(1))
        self.A.data.uniform_(-stdv, stdv)
        self.T = nn.Parameter(torch.FloatTensor(joints_dim, time_dim, time_dim))
        stdv = 1.0 / math.sqrt(self.T.size(1))
        self.T.data.uniform_(-stdv, stdv)
        adj = Graph(layout).get_adjacency()[np.newaxis, :]
        self.A_fixed = nn.Parameter(torch.FloatTensor(adj), requires_grad=False)

    def forward(self, x):
        x = x.contiguous()
        native.require_device(x, "x")
        return _CTGFn.apply(x, self.T.contiguous(), self.A.contiguous(), self.A_fixed.contiguous())


class _Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, geom):
        L = native.lib()
        B, cin, H, W = x.shape
        cout, kh, kw, sh, sw, ph, pw = geom
        Ho, Wo = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        dev = x.device
        y = torch.empty(B, cout, Ho, Wo, dtype=torch.float32, device=dev)
        nbytes = L.dstd_conv2d_workspace_bytes(B, cin, cout, H, W, kh, kw, sh, sw, ph, pw)
        ws = native.workspace(dev, nbytes)
        code = L.dstd_conv2d_fwd(native.ptr(x, "x"), B, cin, H, W, native.ptr(weight, "weight"), _ptr_or_none(bias),
                                 cout, kh, kw, sh, sw, ph, pw, native.ptr(y, "y"), ws.data_ptr(), ws.numel(),
                                 native.stream_handle(dev))
        native.check(code, "dstd_conv2d_fwd")
        ctx.geom = geom
        ctx.save_for_backward(x, weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        L = native.lib()
        x, weight, bias = ctx.saved_tensors
        B, cin, H, W = x.shape
        cout, kh, kw, sh, sw, ph, pw = ctx.geom
        dev = x.device
        dy = dy.contiguous()
        dx = torch.zeros_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.zeros_like(weight)
        db = torch.zeros_like(bias) if bias is not None else None
        nbytes = L.dstd_conv2d_workspace_bytes(B, cin, cout, H, W, kh, kw, sh, sw, ph, pw)
        ws = native.workspace(dev, nbytes)
        code = L.dstd_conv2d_bwd(native.ptr(x, "x"), B, cin, H, W, native.ptr(weight, "weight"), cout, kh, kw, sh, sw,
                                 ph, pw, native.ptr(dy, "dy"), _ptr_or_none(dx), dw.data_ptr(), _ptr_or_none(db),
                                 ws.data_ptr(), ws.numel(), native.stream_handle(dev))
        native.check(code, "dstd_conv2d_bwd")
        return dx, dw, db, None


class Conv2d(nn.Conv2d):
    """nn.Conv2d (same parameters / state_dict) computed by the native kernels
    (include/dstd_gcn_aux.h); groups = dilation = 1, zero padding."""

    def forward(self, x):
        if self.groups != 1 or self.dilation != (1, 1) or self.padding_mode != "zeros" or isinstance(self.padding,
                                                                                                       str):
            raise NotImplementedError("native Conv2d: groups=1, dilation=1, numeric zero padding only")
        x = x.contiguous()
        native.require_device(x, "x")
        geom = (self.out_channels, *self.kernel_size, *self.stride, *self.padding)
        return _Conv2dFn.apply(x, self.weight.contiguous(), None if self.bias is None else self.bias.contiguous(),
                               geom)


class ST_GCNN_layer(nn.Module):
    """Wrapper of one DSTDGCB plus an optional residual (reference :191-249).
    Every shipped config builds ``refine=True``; the STS-GCN style
    ``refine=False`` branch (ConvTemporalGraphical + a k_t x k_v Conv2d,
    :218-223) runs on the native kernels of include/dstd_gcn_aux.h."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, time_dim, joints_dim, bias=True,
                 refine=False, residual=True, layout="h36m"):
        super().__init__()
        self.kernel_size = kernel_size
        self.refine = refine
        assert self.kernel_size[0] % 2 == 1
        assert self.kernel_size[1] % 2 == 1
        padding = ((self.kernel_size[0] - 1) // 2, (self.kernel_size[1] - 1) // 2)
        if refine:
            self.stgcn = nn.ModuleList(
                [nn.Sequential(DSTDGCB(in_channels, out_channels, time_dim, joints_dim, layout))])
        else:
            self.stgcn = nn.Sequential(ConvTemporalGraphical(time_dim, joints_dim, layout),
                                       Conv2d(in_channels, out_channels, (self.kernel_size[0], self.kernel_size[1]),
                                              (stride, stride), padding))
        if not residual:
            self.residual = None
        elif stride != 1 or in_channels != out_channels:
            self.residual = Conv2d(in_channels, out_channels, kernel_size=1, stride=1)
        else:
            self.residual = nn.Identity()
        self.apply(weights_init)

    def forward(self, x):
        if self.refine:
            y = None
            for stb in self.stgcn:
                z = stb(x)
                y = z if y is None else y + z
        else:
            y = self.stgcn(x)
        if self.residual is not None:
            y = y + self.residual(x)
        return y


class DSTDGCN(_NativeModule):
    """The whole network (reference :252-317)."""

    def __init__(self, input_channels, input_time_frame, output_time_frame, st_gcnn_dropout, joints_to_consider,
                 num_feature=64, num_layers=7, layout="h36m"):
        super().__init__()
        self.input_time_frame = input_time_frame
        self.output_time_frame = output_time_frame
        self.joints_to_consider = joints_to_consider
        self.input_channels = input_channels
        self.num_feature = num_feature
        self.num_layers = num_layers
        self.encoders = nn.ModuleList()
        T = input_time_frame + output_time_frame
        self.conv_st_in = ST_GCNN_layer(input_channels, num_feature, [1, 1], 1, T, joints_to_consider, True, True,
                                        False, layout)
        self.bn_in = BatchNorm(num_feature, joints_to_consider, T)
        self.do_in = nn.Dropout(st_gcnn_dropout)
        for _ in range(num_layers):
            self.encoders.append(
                nn.Sequential(ST_GCNN_layer(num_feature, num_feature, [1, 1], 1, T, joints_to_consider, False, True,
                                            True, layout),
                              BatchNorm(num_feature, joints_to_consider, T),
                              nn.PReLU()))
        self.conv_st_out = ST_GCNN_layer(num_feature, input_channels // 2, [1, 1], 1, T, joints_to_consider, True,
                                         True, False, layout)
        self.prelu = nn.PReLU()
        self._native = None
        self._tree = _TensorTree()
        self.gc_arithmetic = "split"  # see DSTDGCB; set_gc_arithmetic() sets the whole tree
        self._dstd_gen = 0
        _register(self)
        self.register_load_state_dict_post_hook(lambda mod, incompatible: invalidate_native_cache(mod))

    def set_gc_arithmetic(self, mode):
        """"split" (default) or "fp32" for this model's eval forward and every
        DSTDGCB in it (include/dstd_gcn.h DSTD_FWD_EXACT_FP32)."""
        native.arith_flags(mode)  # validates
        for m in self.modules():
            if isinstance(m, (DSTDGCN, DSTDGCB)):
                m.gc_arithmetic = mode
        return self

    # -- native parameter block ---------------------------------------------
    def _native_params(self):
        params, buffers = self._tree.get(self)
        if self._native is not None and self._native[2] is params:
            tensors = self._native_tensors
        else:
            tensors = self._native_tensors = params + buffers
        ptrs = tuple(map(_DATA_PTR, tensors))
        if self._native is not None and self._native[0] == ptrs:
            return self._native[1]
        p = native.ModelParams()
        p.T = self.input_time_frame + self.output_time_frame
        p.V = self.joints_to_consider
        p.num_layers = self.num_layers
        p.num_feature = self.num_feature
        p.in_channels = self.input_channels
        if self.num_layers > native.MAX_LAYERS:
            raise ValueError(f"num_layers {self.num_layers} > {native.MAX_LAYERS}")
        p.st_in = native.block_struct(self.conv_st_in.stgcn[0][0])
        p.bn_in = native.bn_struct(self.bn_in)
        p.prelu = native.ptr(self.prelu.weight, "prelu.weight")
        for i, enc in enumerate(self.encoders):
            p.enc[i] = native.block_struct(enc[0].stgcn[0][0])
            p.enc_bn[i] = native.bn_struct(enc[1])
            p.enc_prelu[i] = native.ptr(enc[2].weight, f"encoders.{i}.2.weight")
        p.st_out = native.block_struct(self.conv_st_out.stgcn[0][0])
        self._native = (ptrs, p, params)
        return p

    def _native_grads(self, arena):
        g = native.ModelGrads()
        g.st_in = native.block_grads(self.conv_st_in.stgcn[0][0], arena)
        g.bn_in = native.bn_grads(self.bn_in, arena)
        g.prelu = arena.ptr(self.prelu.weight)
        for i, enc in enumerate(self.encoders):
            g.enc[i] = native.block_grads(enc[0].stgcn[0][0], arena)
            g.enc_bn[i] = native.bn_grads(enc[1], arena)
            g.enc_prelu[i] = arena.ptr(enc[2].weight)
        g.st_out = native.block_grads(self.conv_st_out.stgcn[0][0], arena)
        return g

    def forward(self, x):
        n, t, v, c = x.shape
        assert t == self.input_time_frame + self.output_time_frame
        if c != self.input_channels // 2 or v != self.joints_to_consider:
            raise ValueError(f"DSTDGCN: expected [N, {t}, {self.joints_to_consider}, {self.input_channels // 2}], "
                             f"got {list(x.shape)}")
        L = native.lib()
        x = x.contiguous()
        native.require_device(x, "x")
        if n == 0 and not self.training:  # empty batch: empty output (reference torch semantics)
            return _mark(torch.empty_like(x), x, *self._tree.get(self)[0])
        params, buffers = self._tree.get(self)
        if self.training or _needs_grad(x, *params):
            # train mode, or an eval-mode forward autograd differentiates (the
            # reference back-propagates through running-statistics BN there)
            return _ModelTrain.apply(self, False, x, *_anchor_of(self, x, params))
        flags = native.arith_flags(self.gc_arithmetic)
        if type(x) is not torch.Tensor or torch.compiler.is_compiling():
            # tracing (torch.compile, FakeTensor): the custom op, whose inputs
            # name every tensor the forward reads
            return torch.ops.dstd.dstdgcn_forward(x, params + buffers, self._dstd_uid, flags)
        # eager: the op's implementation without the dispatcher's per-call
        # boxing of ~400 tensor arguments
        y = torch.empty_like(x)
        self._forward_native(x, y, arith=flags)
        return y

    def forward_taps(self, x, blocks=None, what=native.TAP_NAMES):
        """``(y, {block index: taps})``: the eval forward of ``x`` [N, T, V, 3]
        and, per DSTDGCB, the sample-wise graphs and activations it computed
        (include/dstd_gcn_taps.h; ``DSTDGCB.forward_taps`` describes a block's
        ``taps``).  Blocks count in forward order: 0 is conv_st_in, 1..L the
        encoders, L + 1 conv_st_out; ``blocks=None`` taps all of them.  Block
        0's ``x`` is ``cat(x, x - x[:, -1:])`` as [N, 6, T, V]; an encoder's
        ``x`` is the previous block's output after its BatchNorm / residual /
        PReLU.  This is the counterpart of forward hooks on the reference's
        sub-modules, which cannot fire here (the forward is one native call).
        Eval mode only, no autograd; honours ``gc_arithmetic``.  Runs the
        unit-parallel launch schedule at any batch size (one launch per
        adjacency and per GC) and refolds the constants; y equals ``self(x)``."""
        what = _tap_names(what)
        _taps_eval_only(self)
        n, t, v, c = x.shape
        assert t == self.input_time_frame + self.output_time_frame
        if c != self.input_channels // 2 or v != self.joints_to_consider:
            raise ValueError(f"DSTDGCN: expected [N, {t}, {self.joints_to_consider}, {self.input_channels // 2}], "
                             f"got {list(x.shape)}")
        nb = self.num_layers + 2
        blocks = list(range(nb)) if blocks is None else sorted(set(int(b) for b in blocks))
        for b in blocks:
            if not 0 <= b < nb:
                raise ValueError(f"forward_taps: block {b} outside 0..{nb - 1}")
        L = native.lib()
        x = x.detach().contiguous()
        native.require_device(x, "x")
        dev = x.device
        C = self.num_feature
        with torch.no_grad():
            y = torch.empty_like(x)
            out, arr = {}, (native.BlockTaps * nb)()
            for b in blocks:
                cin = self.input_channels if b == 0 else C
                cout = self.input_channels // 2 if b == nb - 1 else C
                out[b], arr[b] = _alloc_taps(what, n, cin, cout, t, v, dev)
            if n == 0:
                return y, out
            p = self._native_params()
            nbytes = L.dstd_model_taps_workspace_bytes(n, t, v, C, self.num_layers)
            # (an untagged claim: the next plain forward folds its constants again)
            ws = native.workspace(dev, nbytes)
            code = L.dstd_model_fwd_taps(p, native.ptr(x, "x"), n, native.ptr(y, "y"), arr, ws.data_ptr(), ws.numel(),
                                         native.stream_handle(dev), native.arith_flags(self.gc_arithmetic))
        native.check(code, "dstd_model_fwd_taps")
        return y, out

    def predict(self, observed, horizon=None, stride=None):
        """The ``horizon`` frames (default ``output_time_frame``) that follow
        ``observed`` [N, input_time_frame, V, 3], as [N, horizon, V, 3]: one
        native call (include/dstd_gcn_predict.h) that pads the observed frames
        into a window with copies of the last one, as the reference's datasets
        do, runs the eval forward, and for a horizon beyond
        ``output_time_frame`` feeds the last ``input_time_frame`` frames of
        what is known so far -- observations as given, predictions appended --
        into the next window, without leaving the device.  What a loop of
        ``self(x)`` over windows built with torch indexing returns, bit for
        bit.  Eval mode only, detached, no autograd; honours ``gc_arithmetic``.
        The folded constants are shared with ``self(x)`` of the same batch
        size (``_forward_native``).

        ``stride`` (an integer in 1..``output_time_frame``; None or
        ``output_time_frame``: the chain above, unchanged): every window
        contributes only its first ``stride`` frames and the next window
        observes the last ``input_time_frame`` frames known by then, again in
        one native call (include/ext/dstd_gcn_stride.h) and equal in bits to
        the window loop.  At most ``PREDICT_MAX_WINDOWS`` windows:
        ``ceil(horizon / stride) <= 64``.  Eager only: under tracing a stride
        below ``output_time_frame`` is a NotImplementedError."""
        if self.training:
            raise RuntimeError("DSTDGCN.predict rolls the eval forward out: call .eval() first")
        n, tin, v, c = observed.shape
        assert tin == self.input_time_frame
        if c != self.input_channels // 2 or v != self.joints_to_consider:
            raise ValueError(f"DSTDGCN: expected [N, {tin}, {self.joints_to_consider}, {self.input_channels // 2}], "
                             f"got {list(observed.shape)}")
        stride = self._predict_stride(stride)
        horizon = self.output_time_frame if horizon is None else int(horizon)
        if horizon < 1:
            raise ValueError(f"DSTDGCN.predict: horizon {horizon} < 1")
        if -(-horizon // (stride or self.output_time_frame)) > native.PREDICT_MAX_WINDOWS:
            fits = -(-horizon // native.PREDICT_MAX_WINDOWS)  # the smallest stride with at most that many windows
            if stride is not None and fits <= self.output_time_frame:
                raise ValueError(f"DSTDGCN.predict: horizon {horizon} at stride {stride} needs more than "
                                 f"{native.PREDICT_MAX_WINDOWS} windows; it needs stride >= {fits}")
            raise ValueError(f"DSTDGCN.predict: horizon {horizon} needs more than {native.PREDICT_MAX_WINDOWS} "
                             f"windows of {self.output_time_frame} frames")
        native.lib()
        observed = observed.detach().contiguous()
        native.require_device(observed, "observed")
        flags = native.arith_flags(self.gc_arithmetic)
        if type(observed) is not torch.Tensor or torch.compiler.is_compiling():
            if stride is not None:
                raise NotImplementedError("DSTDGCN.predict: a stride below output_time_frame is eager only -- the "
                                          "custom op has no stride, so it cannot be traced (torch.compile, tensor "
                                          "subclasses)")
            # tracing: the custom op, whose inputs name every tensor the call reads
            params, buffers = self._tree.get(self)
            return torch.ops.dstd.dstdgcn_predict(observed, params + buffers, self._dstd_uid, horizon, flags)
        with torch.no_grad():
            out = observed.new_empty(n, horizon, v, c)
            if n:
                self._predict_native(observed, out, arith=flags, stride=stride)
        return out

    def _predict_stride(self, stride, what="predict"):
        """``predict``'s (and ``rollout``'s) ``stride`` as checked: None for
        today's chain (no stride, or one of a whole window), the integer
        otherwise."""
        if stride is None:
            return None
        if isinstance(stride, bool) or not isinstance(stride, numbers.Integral) \
                or not 1 <= stride <= self.output_time_frame:
            raise ValueError(f"DSTDGCN.{what}: stride must be an integer in 1..{self.output_time_frame} "
                             f"(output_time_frame), got {stride!r}")
        return None if stride == self.output_time_frame else int(stride)

    def _predict_native(self, obs, out, arith=None, stride=None):
        """One rollout through dstd_model_predict -- with a ``stride``,
        dstd_model_predict_strided -- on the forward's workspace and constants
        (``_claim_workspace``)."""
        L = native.lib()
        n, tin, v, _ = obs.shape
        dev = obs.device
        t = tin + self.output_time_frame
        p = self._native_params()
        flags = (native.arith_flags(self.gc_arithmetic) if arith is None else arith) | self._dstd_fwd_flags
        if stride is not None:
            nbytes = L.dstd_model_predict_strided_workspace_bytes(n, t, v, self.num_feature, self.num_layers)
            ws, flags = self._claim_workspace(dev, nbytes, n, flags)
            code = L.dstd_model_predict_strided(native.ext_stride.model_params_ref(p), native.ptr(obs, "observed"), n,
                                                tin, out.shape[1], stride, native.ptr(out, "out"), ws.data_ptr(),
                                                ws.numel(), native.stream_handle(dev), flags)
            native.check(code, "dstd_model_predict_strided")
            return
        nbytes = L.dstd_model_predict_workspace_bytes(n, t, v, self.num_feature, self.num_layers)
        ws, flags = self._claim_workspace(dev, nbytes, n, flags)
        code = L.dstd_model_predict(p, native.ptr(obs, "observed"), n, tin, out.shape[1], native.ptr(out, "out"),
                                    ws.data_ptr(), ws.numel(), native.stream_handle(dev), flags)
        native.check(code, "dstd_model_predict")

    def _rollout_args(self, observed, horizon, what, stride=None):
        """(observed's shape, horizon) of a rollout call, checked as ``predict``
        checks them; ``stride``: what ``_predict_stride`` returned."""
        n, tin, v, c = observed.shape
        assert tin == self.input_time_frame
        if c != self.input_channels // 2 or v != self.joints_to_consider:
            raise ValueError(f"DSTDGCN: expected [N, {tin}, {self.joints_to_consider}, {self.input_channels // 2}], "
                             f"got {list(observed.shape)}")
        horizon = self.output_time_frame if horizon is None else int(horizon)
        if horizon < 1:
            raise ValueError(f"DSTDGCN.{what}: horizon {horizon} < 1")
        if -(-horizon // (stride or self.output_time_frame)) > native.PREDICT_MAX_WINDOWS:
            fits = -(-horizon // native.PREDICT_MAX_WINDOWS)  # the smallest stride with at most that many windows
            if stride is not None and fits <= self.output_time_frame:
                raise ValueError(f"DSTDGCN.{what}: horizon {horizon} at stride {stride} needs more than "
                                 f"{native.PREDICT_MAX_WINDOWS} windows; it needs stride >= {fits}")
            raise ValueError(f"DSTDGCN.{what}: horizon {horizon} needs more than {native.PREDICT_MAX_WINDOWS} "
                             f"windows of {self.output_time_frame} frames")
        return (n, tin, v, c), horizon

    def _rollout_refusals(self, observed, what):
        """What the differentiable chain does not cover, said before anything runs."""
        if self.training and self.__dict__.get("_dstd_bn_sync") is not None:
            raise NotImplementedError(f"DSTDGCN.{what}: no cross-rank BatchNorm through a rollout "
                                      "(include/ext/dstd_gcn_rollout.h has no dstd_bn_sync variant)")
        if type(observed) is not torch.Tensor or torch.compiler.is_compiling():
            raise RuntimeError(f"DSTDGCN.{what}: eager only -- the chain has no custom op, so it cannot be traced "
                               "(torch.compile, tensor subclasses)")
        native.lib()
        native.require_device(observed, "observed")

    def _teacher_args(self, teacher, teacher_mask, observed, halves, horizon, what, stride=None):
        """(teacher, mask as uint8) of a rollout call with scheduled sampling,
        checked before anything runs: ``teacher`` [N, >= input_n + horizon, V, 3]
        float32 and ``teacher_mask`` [windows, halves * N] bool or uint8, both
        on the device of ``observed`` [N, input_n, V, 3]; ``windows`` is
        ``ceil(horizon / stride)`` with a ``stride``."""
        if (teacher is None) != (teacher_mask is None):
            raise ValueError(f"DSTDGCN.{what}: teacher and teacher_mask come together "
                             f"(got {'teacher' if teacher_mask is None else 'teacher_mask'} alone)")
        n, tin, v, c = observed.shape
        windows = -(-horizon // (stride or self.output_time_frame))
        for name, x in (("teacher", teacher), ("teacher_mask", teacher_mask)):
            if not torch.is_tensor(x):
                raise ValueError(f"DSTDGCN.{what}: {name} must be a tensor, got {type(x).__name__}")
            if x.device != observed.device:
                raise ValueError(f"DSTDGCN.{what}: {name} is on {x.device}, observed on {observed.device}")
        if teacher.dtype != torch.float32:
            raise ValueError(f"DSTDGCN.{what}: teacher must be float32, got {teacher.dtype}")
        if teacher.dim() != 4 or teacher.shape[0] != n or tuple(teacher.shape[2:]) != (v, c):
            raise ValueError(f"DSTDGCN.{what}: expected teacher [{n}, >= {tin + horizon}, {v}, {c}], "
                             f"got {list(teacher.shape)}")
        if teacher.shape[1] < tin + horizon:
            raise ValueError(f"DSTDGCN.{what}: horizon {horizon} after {tin} observed frames needs a teacher of "
                             f"{tin + horizon} frames, got {teacher.shape[1]}")
        if teacher_mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"DSTDGCN.{what}: teacher_mask must be bool or uint8, got {teacher_mask.dtype}")
        if tuple(teacher_mask.shape) != (windows, halves * n):
            raise ValueError(f"DSTDGCN.{what}: expected teacher_mask [{windows}, {halves * n}], "
                             f"got {list(teacher_mask.shape)}")
        mask = teacher_mask.contiguous()
        return teacher.detach().contiguous(), mask.view(torch.uint8) if mask.dtype == torch.bool else mask

    def rollout(self, observed, horizon=None, teacher=None, teacher_mask=None, stride=None):
        """``predict`` that autograd can differentiate and a train-mode model
        can run: the ``horizon`` frames (default ``output_time_frame``) after
        ``observed`` [N, input_time_frame, V, 3], as [N, horizon, V, 3].

        In ``eval()`` mode with nothing to differentiate it is
        ``self.predict(observed, horizon)``.  In ``train()`` mode every window
        is the train-mode forward -- batch statistics per window, the running
        statistics updated once per window in window order, a dropout mask per
        window -- and in ``eval()`` mode with grad enabled and ``observed`` or a
        parameter requiring grad it is the eval forward under autograd
        (BatchNorm on its running statistics, no dropout).  Either way the
        chain is ONE autograd Function over two native calls
        (include/ext/dstd_gcn_rollout.h): what a loop of ``self(x_k)`` over
        windows built under autograd computes -- outputs, buffers and
        gradients bit for bit (tests/test_gpu_rollout.py) -- without K
        Functions of ~300 inputs each, and with the gradient of the window
        shuffling summed in a fixed order.  Eager only; no cross-rank
        BatchNorm.

        Scheduled sampling: with ``teacher`` [N, >= input_time_frame + horizon,
        V, 3] (each sample's own frames from the first observed one) and
        ``teacher_mask`` [windows, N] (bool or uint8, on the device), sample b's
        window k is built from the teacher's frames instead of what is known
        so far wherever ``teacher_mask[k, b]`` is set, and no gradient crosses
        that boundary (include/ext/dstd_gcn_teacher.h; row 0 is not read).  The
        result is always the model's prediction.  Neither gets a gradient.

        ``stride`` is ``predict``'s (an integer in 1..``output_time_frame``;
        None or ``output_time_frame``: the chain above, call for call): every
        window hands on its first ``stride`` frames only, so the chain has
        ``ceil(horizon / stride)`` windows -- at most ``PREDICT_MAX_WINDOWS``,
        and that many rows of ``teacher_mask`` -- and a predicted frame is
        observed by up to ``ceil(input_time_frame / stride)`` later windows,
        whose gradients are summed in a fixed order
        (include/ext/dstd_gcn_stride_train.h).  What the window loop of
        ``predict(stride=)`` computes under autograd, bit for bit
        (tests/test_gpu_rollout_stride.py).  As without a stride, the frames
        a forced window took from the teacher are what that sample knows from
        then on: a later free window that still observes them sees the
        teacher's frames, and no gradient passes through them.  Its saved
        activations grow with the number of windows, not with ``horizon``."""
        stride = self._predict_stride(stride, "rollout")
        (n, tin, v, c), horizon = self._rollout_args(observed, horizon, "rollout", stride)
        params = self._tree.get(self)[0]
        tf = teacher is not None or teacher_mask is not None
        if tf:
            teacher, mask = self._teacher_args(teacher, teacher_mask, observed, 1, horizon, "rollout", stride)
        if not self.training and not _needs_grad(observed, *params):
            if tf:
                raise RuntimeError("DSTDGCN.rollout: a teacher needs train mode or something to differentiate "
                                   "(predict has no teacher)")
            return self.predict(observed, horizon, stride)
        self._rollout_refusals(observed, "rollout")
        observed = observed.contiguous()
        if n == 0:  # empty batch: empty output
            return _mark(observed.new_empty(0, horizon, v, c), observed, *params)
        return _RolloutChain.apply(self, False, horizon, stride, observed, teacher if tf else None,
                                   mask if tf else None, [(0, 1)] if tf else None, *_anchor_of(self, observed, params))

    def rollout_pair(self, obs1, obs2, horizon=None, teacher=None, teacher_mask=None, stride=None):
        """``(self.rollout(obs1, horizon), self.rollout(obs2, horizon))`` as one
        chain over the concatenated batch, as ``forward_pair`` is for one
        window: in train mode every window keeps each half's own batch
        statistics and the running statistics take obs1's update then obs2's
        (DSTD_TRAIN_PAIRED), window by window.  Elsewhere (eval, shapes that
        differ, an empty batch) it is the two calls.

        Scheduled sampling: one ``teacher`` [N, Ttot, V, 3] serves both halves,
        obs1's forwards in time and obs2's backwards from its last frame (the
        time reversal of PredictionEngine.train: frame maps (0, +1) and
        (Ttot - 1, -1)); ``teacher_mask`` is [windows, 2 N], obs1's samples
        first.  ``stride`` is ``rollout``'s."""
        stride = self._predict_stride(stride, "rollout_pair")
        tf = teacher is not None or teacher_mask is not None
        if tf:
            if obs1.shape != obs2.shape or obs1.device != obs2.device:
                raise ValueError("DSTDGCN.rollout_pair: one teacher serves two batches of one shape on one device, got "
                                 f"{list(obs1.shape)} on {obs1.device} and {list(obs2.shape)} on {obs2.device}")
            (n, tin, v, c), horizon = self._rollout_args(obs1, horizon, "rollout_pair", stride)
            teacher, mask = self._teacher_args(teacher, teacher_mask, obs1, 2, horizon, "rollout_pair", stride)
        if not self.training or obs1.shape != obs2.shape or obs1.shape[0] == 0 or obs1.device != obs2.device:
            if tf:  # the second call reads the teacher backwards as a tensor of its own
                return (self.rollout(obs1, horizon, teacher, mask[:, :n], stride=stride),
                        self.rollout(obs2, horizon, teacher.flip(1), mask[:, n:], stride=stride))
            return self.rollout(obs1, horizon, stride=stride), self.rollout(obs2, horizon, stride=stride)
        (n, tin, v, c), horizon = self._rollout_args(obs1, horizon, "rollout_pair", stride)
        self._rollout_refusals(obs1, "rollout_pair")
        if type(obs2) is not torch.Tensor:
            raise RuntimeError("DSTDGCN.rollout_pair: eager only (tensor subclasses cannot be traced through the chain)")
        obs = torch.cat([obs1, obs2]).contiguous()
        params = self._tree.get(self)[0]
        maps = [(0, 1), (teacher.shape[1] - 1, -1)] if tf else None
        return _RolloutChainPair.apply(self, n, horizon, stride, obs, teacher if tf else None, mask if tf else None,
                                       maps, *_anchor_of(self, obs, params))

    def forward_pair(self, x1, x2):
        """``(self(x1), self(x2))`` -- PredictionEngine.train's forward of a
        batch and of its time reversal (engine/prediction.py:231-287) -- as
        ONE native launch sequence over the concatenated batch.  In train mode
        every BatchNorm keeps each half's own batch statistics and the running
        statistics take x1's update then x2's (DSTD_TRAIN_PAIRED), so outputs,
        gradients and buffers are those of the two calls; elsewhere (eval, or
        shapes that differ) it is the two calls."""
        if not self.training or x1.shape != x2.shape or x1.shape[0] == 0 or x1.device != x2.device:
            return self(x1), self(x2)
        n, t, v, c = x1.shape
        assert t == self.input_time_frame + self.output_time_frame
        if c != self.input_channels // 2 or v != self.joints_to_consider:
            raise ValueError(f"DSTDGCN: expected [N, {t}, {self.joints_to_consider}, {self.input_channels // 2}], "
                             f"got {list(x1.shape)}")
        native.lib()
        x = torch.cat([x1, x2]).contiguous()
        native.require_device(x, "x")
        params = self._tree.get(self)[0]
        return _ModelTrainPair.apply(self, n, x, *_anchor_of(self, x, params))

    def graphed(self, x, frozen=False):
        """The eval forward for inputs shaped like ``x`` captured once into a
        HIP graph (no per-call launch or Python cost at small
        batch).  Returns ``run(x_new) -> y``: copies ``x_new`` into the graph's
        static input (skipped when it is that tensor, ``run.input``), replays
        the forward's launches and returns the graph's static output
        ``run.output`` (overwritten by the next replay).  By default every
        replay also re-runs the two launches that fold BatchNorm and prepare
        the split weight images, so in-place parameter updates are seen by the
        next replay.  ``frozen=True`` (serving fixed weights): the first call
        folds, later ones replay the GC launches alone; after an in-place
        parameter update call ``run.refresh()``.  New parameter storage (e.g.
        ``load_state_dict`` into fresh tensors, ``.to()``) needs a new capture."""
        if self.training:
            raise RuntimeError("DSTDGCN.graphed captures the eval forward: call .eval() first")
        dev = x.device
        native.require_device(x, "x")
        x_static = x.detach().clone().contiguous()
        y_static = torch.empty_like(x_static)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.no_grad(), torch.cuda.stream(side):
            for _ in range(2):  # library load, per-kernel attributes, workspace
                self(x_static)
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        cap = torch.cuda.Stream(device=dev)  # a stream of its own: its workspace is private to this graph
        with torch.no_grad(), torch.cuda.graph(g, stream=cap):
            self._forward_native(x_static, y_static)
        gf = None
        if frozen:
            # the same forward again on the same workspace: the claim finds the
            # constants graph g folds there (same tag), so this capture holds
            # only the GC launches
            gf = torch.cuda.CUDAGraph()
            with torch.no_grad(), torch.cuda.graph(gf, stream=cap):
                self._forward_native(x_static, y_static)
        # the capture's workspace lives in the graph's memory pool: keep it
        # with the graph and out of the eager cache
        ws = native._ws_cache.pop((str(dev), cap.cuda_stream), (None, None))[0]
        state = {"folded": False}

        def run(x_new):
            if x_new is not x_static:
                x_static.copy_(x_new)
            if gf is not None and state["folded"]:
                gf.replay()
            else:
                g.replay()
                state["folded"] = True
            return y_static

        def refresh():
            """(frozen) parameters changed in place: the next call refolds."""
            state["folded"] = False

        run.graph, run.graph_frozen, run.input, run.output, run._workspace = g, gf, x_static, y_static, ws
        run.refresh = refresh
        return run

    def _claim_workspace(self, dev, nbytes, n, flags):
        """(workspace, flags) of an eval call at batch size ``n``, after
        ``_native_params``: the flags carry DSTD_FWD_REUSE_CONSTANTS when the
        buffer still holds this model's constants (``_forward_native``).  The
        forward and ``predict`` lay the constants out alike at the start of the
        buffer and claim it under one tag, so either reuses the other's."""
        try:
            versions = tuple(map(_VERSION, self._native_tensors))
            tag = (self._dstd_uid, self._dstd_gen, self._native[0], n, flags, versions)
        except RuntimeError:  # "Inference tensors do not track version counter"
            tag = None
        ws, reuse = native.workspace_claim(dev, nbytes, tag)
        return ws, (flags | native.FWD_REUSE_CONSTANTS) if reuse else flags

    def _forward_native(self, x, y, prof=None, arith=None):
        """One eval forward through dstd_model_fwd_ex.  The folded constants
        and split-f16 weight images a forward leaves in the workspace are
        reused when nothing changed since: same model instance (a token never
        reused) and cache generation (invalidate_native_cache), same parameter
        storage, torch version counters unchanged (no in-place update), batch
        size, arithmetic, and no other user of the workspace in between.
        Tensors without version counters (inference tensors) never reuse."""
        L = native.lib()
        n, t, v, _ = x.shape
        dev = x.device
        if prof is None:  # event brackets requested through the module (bench.py probes model(x) itself)
            prof = getattr(self, "_dstd_profile", None)
        p = self._native_params()
        flags = (native.arith_flags(self.gc_arithmetic) if arith is None else arith) | self._dstd_fwd_flags
        nbytes = L.dstd_model_workspace_bytes(n, t, v, self.num_feature, self.num_layers)
        ws, flags = self._claim_workspace(dev, nbytes, n, flags)
        code = L.dstd_model_fwd_ex(p, native.ptr(x, "x"), n, native.ptr(y, "y"), ws.data_ptr(), ws.numel(),
                                   native.stream_handle(dev), flags, prof)
        native.check(code, "dstd_model_fwd_ex")


# ---------------------------------------------------------------------------
# torch.library ops: the eval forwards as custom operators with
# fake (meta) kernels, so torch.compile / FakeTensor tracing see them as single
# ops with known output shapes.  Each op receives every tensor of its module
# (the data dependencies) plus the module's instance token, under which the
# implementation finds the module that lays out the C parameter struct
# (include/dstd_gcn.h); underneath is the same C ABI call as before.
# ---------------------------------------------------------------------------
def _instance(uid):
    mod = _INSTANCES.get(uid)
    if mod is None:
        raise RuntimeError(f"dstd op: no live DSTD module with instance token {uid}")
    return mod


@torch.library.custom_op("dstd::dstdgc_forward", mutates_args=())
def _op_dstdgc_forward(x: torch.Tensor, A: torch.Tensor, alpha: torch.Tensor, weights: List[torch.Tensor],
                       uid: int) -> torch.Tensor:
    """DSTDGC.forward eval (reference :80-94) -> dstd_dstdgc_fwd."""
    return _instance(uid)._eval_native(x, A, alpha)


@_op_dstdgc_forward.register_fake
def _(x, A, alpha, weights, uid):
    # weights in DSTDGC.parameters() order: conv_m1, conv_m2, conv_rm, conv_f (weight, bias)
    return x.new_empty(x.shape[0], weights[6].shape[0], x.shape[2], x.shape[3])


@torch.library.custom_op("dstd::dstdgcb_forward", mutates_args=())
def _op_dstdgcb_forward(x: torch.Tensor, tensors: List[torch.Tensor], uid: int, cout: int,
                        flags: int) -> torch.Tensor:
    """DSTDGCB.forward eval (reference :141-163) -> dstd_block_fwd_ex."""
    return _instance(uid)._eval_native(x, flags)


@_op_dstdgcb_forward.register_fake
def _(x, tensors, uid, cout, flags):
    return x.new_empty(x.shape[0], cout, x.shape[2], x.shape[3])


@torch.library.custom_op("dstd::dstdgcn_forward", mutates_args=())
def _op_dstdgcn_forward(x: torch.Tensor, tensors: List[torch.Tensor], uid: int, flags: int) -> torch.Tensor:
    """DSTDGCN.forward eval (reference :293-317) -> dstd_model_fwd_ex."""
    y = torch.empty_like(x)
    _instance(uid)._forward_native(x, y, arith=flags)
    return y


@_op_dstdgcn_forward.register_fake
def _(x, tensors, uid, flags):
    return torch.empty_like(x)


@torch.library.custom_op("dstd::dstdgcn_predict", mutates_args=())
def _op_dstdgcn_predict(observed: torch.Tensor, tensors: List[torch.Tensor], uid: int, horizon: int,
                        flags: int) -> torch.Tensor:
    """DSTDGCN.predict -> dstd_model_predict (no counterpart in the reference:
    its callers loop over windows in Python)."""
    n, _, v, c = observed.shape
    out = observed.new_empty(n, horizon, v, c)
    if n:
        _instance(uid)._predict_native(observed.contiguous(), out, arith=flags)
    return out


@_op_dstdgcn_predict.register_fake
def _(observed, tensors, uid, horizon, flags):
    n, _, v, c = observed.shape
    return observed.new_empty(n, horizon, v, c)


# Training directions: forward ops return the
# output and the saved-state buffer the backward op consumes; backward ops
# return the input gradient (empty when not needed) and every parameter
# gradient in one flat arena (dstd_native.GradArena layout, in params order).
# The forward ops update the BN running statistics among `buffers` in train
# mode (declared mutated).
@torch.library.custom_op("dstd::dstdgcb_train_forward", mutates_args=("buffers",))
def _op_dstdgcb_train_forward(x: torch.Tensor, params: List[torch.Tensor], buffers: List[torch.Tensor], uid: int,
                              flags: int, momentum: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """DSTDGCB forward with train-mode (or running-stats) BN -> dstd_block_train_fwd_ex."""
    return _block_train_fwd_native(_instance(uid), x, flags, momentum)


@_op_dstdgcb_train_forward.register_fake
def _(x, params, buffers, uid, flags, momentum):
    blk = _instance(uid)
    B, cin, T, V = x.shape
    nbytes = native.lib().dstd_block_train_saved_bytes(B, cin, blk.out_channels, T, V)
    return x.new_empty(B, blk.out_channels, T, V), x.new_empty(nbytes, dtype=torch.uint8)


@torch.library.custom_op("dstd::dstdgcb_train_backward", mutates_args=())
def _op_dstdgcb_train_backward(x: torch.Tensor, saved: torch.Tensor, dy: torch.Tensor, params: List[torch.Tensor],
                               uid: int, flags: int, need_dx: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """DSTDGCB backward -> dstd_block_train_bwd_ex."""
    blk = _instance(uid)
    # the arena is laid out over the module's own parameters (the native
    # pointer table resolves them by identity); `params` -- the same tensors
    # in normal use, copies under opcheck -- match them slot for slot
    arena = native.GradArena(list(blk.parameters()), x.device)
    dx = _block_train_bwd_native(blk, x, saved, dy, flags, arena, need_dx)
    return (dx if dx is not None else x.new_empty(0)), arena.buf


@_op_dstdgcb_train_backward.register_fake
def _(x, saved, dy, params, uid, flags, need_dx):
    return (torch.empty_like(x) if need_dx else x.new_empty(0)), x.new_empty(native.arena_numel(params))


@torch.library.custom_op("dstd::dstdgcn_train_forward", mutates_args=("buffers",))
def _op_dstdgcn_train_forward(x: torch.Tensor, params: List[torch.Tensor], buffers: List[torch.Tensor], uid: int,
                              flags: int, momentum: float, drop: float, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """DSTDGCN forward with train-mode (or running-stats) BN -> dstd_model_train_fwd_ex."""
    return _model_train_fwd_native(_instance(uid), x, flags, momentum, drop, seed)


@_op_dstdgcn_train_forward.register_fake
def _(x, params, buffers, uid, flags, momentum, drop, seed):
    m = _instance(uid)
    n, t, v, c = x.shape
    nbytes = native.lib().dstd_model_train_saved_bytes(n, t, v, m.num_feature, m.num_layers)
    return torch.empty_like(x), x.new_empty(nbytes, dtype=torch.uint8)


@torch.library.custom_op("dstd::dstdgcn_train_backward", mutates_args=())
def _op_dstdgcn_train_backward(x: torch.Tensor, saved: torch.Tensor, dy: torch.Tensor, params: List[torch.Tensor],
                               uid: int, flags: int, drop: float, seed: int,
                               need_dx: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """DSTDGCN backward -> dstd_model_train_bwd_ex."""
    m = _instance(uid)
    arena = native.GradArena(m._tree.get(m)[0], x.device)  # (see dstdgcb_train_backward)
    dx = _model_train_bwd_native(m, x, saved, dy, flags, drop, seed, m._native_grads(arena), need_dx)
    return (dx if dx is not None else x.new_empty(0)), arena.buf


@_op_dstdgcn_train_backward.register_fake
def _(x, saved, dy, params, uid, flags, drop, seed, need_dx):
    return (torch.empty_like(x) if need_dx else x.new_empty(0)), x.new_empty(native.arena_numel(params))


@torch.library.custom_op("dstd::dstdgc_train_forward", mutates_args=())
def _op_dstdgc_train_forward(x: torch.Tensor, A: torch.Tensor, alpha: torch.Tensor, weights: List[torch.Tensor],
                             uid: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """DSTDGC forward keeping the backward's state -> dstd_dstdgc_train_fwd."""
    mod = _instance(uid)
    mode = native.MODE_SPATIAL if mod.mode == "spatial" else native.MODE_TEMPORAL
    return _op_train_fwd_native(mod, mode, x, A, alpha)


@_op_dstdgc_train_forward.register_fake
def _(x, A, alpha, weights, uid):
    mod = _instance(uid)
    mode = native.MODE_SPATIAL if mod.mode == "spatial" else native.MODE_TEMPORAL
    B, cin, T, V = x.shape
    nbytes = native.lib().dstd_dstdgc_train_saved_bytes_r(mode, B, cin, mod.out_channels, T, V, mod.red_channels)
    return x.new_empty(B, mod.out_channels, T, V), x.new_empty(nbytes, dtype=torch.uint8)


@torch.library.custom_op("dstd::dstdgc_train_backward", mutates_args=())
def _op_dstdgc_train_backward(x: torch.Tensor, A: torch.Tensor, alpha: torch.Tensor, saved: torch.Tensor,
                              dy: torch.Tensor, weights: List[torch.Tensor], uid: int,
                              need_dx: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """DSTDGC backward -> dstd_dstdgc_train_bwd: (dx, dA, dalpha, weight-gradient arena)."""
    L = native.lib()
    mod = _instance(uid)
    mode = native.MODE_SPATIAL if mod.mode == "spatial" else native.MODE_TEMPORAL
    B, cin, T, V = x.shape
    dev = x.device
    cout = mod.out_channels
    arena = native.GradArena(list(mod.parameters()), dev)  # (see dstdgcb_train_backward)
    dx = torch.zeros_like(x) if need_dx else x.new_empty(0)
    dA = torch.zeros_like(A)
    dalpha = torch.zeros_like(alpha)
    red = mod.red_channels
    ws = native.workspace(dev, L.dstd_dstdgc_train_workspace_bytes_r(mode, B, cin, cout, T, V, red))
    code = L.dstd_dstdgc_train_bwd_r(mode, native.ptr(x, "x"), B, cin, cout, T, V, red, native.gc_weights(mod),
                                     native.ptr(alpha, "alpha_m"), saved.data_ptr(), saved.numel(),
                                     native.ptr(dy, "dy"), dx.data_ptr() if need_dx else None,
                                     native.gc_grads(mod, arena), native.ptr(dA, "dA"), native.ptr(dalpha, "dalpha"),
                                     ws.data_ptr(), ws.numel(), native.stream_handle(dev))
    native.check(code, "dstd_dstdgc_train_bwd_r")
    return dx, dA, dalpha, arena.buf


@_op_dstdgc_train_backward.register_fake
def _(x, A, alpha, saved, dy, weights, uid, need_dx):
    return ((torch.empty_like(x) if need_dx else x.new_empty(0)), torch.empty_like(A), torch.empty_like(alpha),
            x.new_empty(native.arena_numel(weights)))
