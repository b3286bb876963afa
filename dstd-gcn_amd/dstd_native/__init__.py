"""ctypes binding of the MI355X C ABI (include/*.h, declared in abi.py; include/ext/*.h in ext.py,
ext_eval.py, ext_augment.py, ext_stride.py, ext_stride_train.py and ext_warp.py).

The shared library ``libdstd_gcn.so`` is built in-tree (``make -C dstd-gcn_amd``
or ``__graft_entry__.build()``).  There is no fallback: if the library is
missing or a tensor is not on a ROCm device, the call raises.
"""
import ctypes
import os

import torch

from .abi import *  # noqa: F401,F403 -- the constants, structs and export lists are this package's names
from . import ext  # include/ext/*.h: a table of its own, by name only (not star-imported)
from . import ext_eval  # include/ext/dstd_gcn_eval.h: likewise (ext.ALL and ext.ABI are pinned by their tests)
from . import ext_augment  # include/ext/dstd_gcn_augment.h: likewise
from . import ext_stride  # include/ext/dstd_gcn_stride.h: likewise
from . import ext_stride_train  # include/ext/dstd_gcn_stride_train.h: likewise
from . import ext_warp  # include/ext/dstd_gcn_warp.h: likewise

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSTD_LIB overrides the library (A/B experiments with variant builds)
LIB_PATH = os.environ.get("DSTD_LIB") or os.path.join(os.path.dirname(_HERE), "libdstd_gcn.so")


def model_schedule(B, T, V, num_feature, num_layers, flags=0, profiled=False, taps=0, cus=0):
    """dstd_model_fwd_schedule: the (kind, first_block, num_blocks) launches a
    forward of these arguments enqueues after its parameter preparation; cus=0:
    on the current device.  With cus > 0 no GPU is touched."""
    out = (Launch * (1 + 4 * (MAX_LAYERS + 2)))()
    n = lib().dstd_model_fwd_schedule(B, T, V, num_feature, num_layers, flags, int(profiled), taps, cus, out, len(out))
    if n < 0:
        raise RuntimeError(f"dstd_model_fwd_schedule failed ({n}): {lib().dstd_error_string(n).decode()}")
    return [(out[i].kind, out[i].first_block, out[i].num_blocks) for i in range(n)]

_lib = None


def source_hash():
    """sha256 (16 hex digits) of the sources the library is built from, in the
    order dstd-gcn_amd/Makefile hashes them (HASHED); None when the sources
    are not next to the package."""
    import glob
    import hashlib
    pkg = os.path.dirname(_HERE)
    rel = [os.path.relpath(p, pkg) for pat in ("csrc/*.hip", "csrc/*.h", "../include/*.h", "../include/ext/*.h")
           for p in glob.glob(os.path.join(pkg, pat))]
    files = sorted(rel) + ["Makefile"]
    h = hashlib.sha256()
    for f in files:
        path = os.path.join(pkg, f)
        if not os.path.exists(path):
            return None
        with open(path, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def lib():
    """Load libdstd_gcn.so once; raise loudly if it is not built, or if it was
    built from other sources than the tree it is loaded from (its embedded
    dstd_source_hash() against source_hash())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"DSTD native library not built: {LIB_PATH} (run `make -C dstd-gcn_amd`)")
        L = ctypes.CDLL(LIB_PATH)
        # DSTD_AB_FOREIGN_LIB=1: A/B tooling (scripts/ab_kernels.py) loading a
        # library built from an earlier revision on purpose
        foreign = os.environ.get("DSTD_AB_FOREIGN_LIB") == "1"
        declare(L, allow_missing=foreign, extra={**ext.ALL, **ext_eval.ABI, **ext_augment.ABI, **ext_stride.ABI,
                                                       **ext_stride_train.ABI, **ext_warp.ABI})
        built, tree = L.dstd_source_hash().decode(), source_hash()
        if tree is not None and built != tree and not foreign:
            raise RuntimeError(f"{LIB_PATH} was built from other sources (hash {built}, this tree {tree}): "
                               "rebuild with `make -C dstd-gcn_amd`")
        _lib = L
    return _lib


ARITHMETICS = ("split", "fp32")


def arith_flags(mode):
    """Per-call flag of the graph-convolution arithmetic (include/dstd_gcn.h
    DSTD_FWD_EXACT_FP32): "split" (split-f16 MFMA where the shape has kernels,
    the default) or "fp32" (exact-fp32 MFMA everywhere)."""
    if mode not in ARITHMETICS:
        raise ValueError(f"gc arithmetic must be one of {ARITHMETICS}, got {mode!r}")
    return FWD_EXACT_FP32 if mode == "fp32" else 0


def check(code, what):
    if code != 0:
        msg = lib().dstd_error_string(code).decode()
        raise RuntimeError(f"{what} failed ({code}): {msg}")


# ---------------------------------------------------------------------------
# tensor helpers
# ---------------------------------------------------------------------------
def require_device(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the DSTD path runs on the MI355X only (tensor is on {t.device}); "
                           "there is no CPU fallback")
    if t.dtype != torch.float32:
        raise ValueError(f"{name}: expected float32, got {t.dtype}")


def ptr(t, name="tensor"):
    require_device(t, name)
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")
    return t.data_ptr()


def stream_handle(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_ws_cache = {}


def workspace(device, nbytes):
    """Caller-owned scratch (torch caching allocator), grown on demand and kept
    per (device, stream) so graph capture and steady state reuse one buffer."""
    return workspace_claim(device, nbytes, None)[0]


def workspace_claim(device, nbytes, tag):
    """workspace() for a caller that can reuse what its previous call left in
    the buffer: returns (buf, reused), reused = True iff the last claim of this
    buffer carried the same (non-None) tag and nothing else used it since."""
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    buf, last = _ws_cache.get(key, (None, None))
    reused = buf is not None and buf.numel() >= nbytes and tag is not None and last == tag
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    _ws_cache[key] = (buf, tag)
    return buf, reused


def gc_weights(dstdgc):
    """GCWeights from a DSTDGC module (conv weights [O, I, 1, 1] are read as [O, I])."""
    w = GCWeights()
    for f, conv in (("f", dstdgc.conv_f), ("m1", dstdgc.conv_m1), ("m2", dstdgc.conv_m2), ("rm", dstdgc.conv_rm)):
        setattr(w, "w" + f, ptr(conv.weight, f"conv_{f}.weight"))
        setattr(w, "b" + f, ptr(conv.bias, f"conv_{f}.bias"))
    return w


def bn_struct(bnw):
    """BN from the reference BatchNorm wrapper (.bn = BatchNorm1d(C*V))."""
    b = bnw.bn
    return BN(ptr(b.weight, "bn.weight"), ptr(b.bias, "bn.bias"), ptr(b.running_mean, "bn.running_mean"),
              ptr(b.running_var, "bn.running_var"), float(b.eps))


def block_struct(blk):
    p = BlockParams()
    p.cin, p.cout = blk.in_channels, blk.out_channels
    p.A_s, p.W_s, p.R_s = ptr(blk.A_s, "A_s"), ptr(blk.W_s, "W_s"), ptr(blk.R_s, "R_s")
    p.A_t, p.R_t = ptr(blk.A_t, "A_t"), ptr(blk.R_t, "R_t")
    p.alpha_sm, p.alpha_tm = ptr(blk.alpha_sm, "alpha_sm"), ptr(blk.alpha_tm, "alpha_tm")
    p.conv_s[0] = gc_weights(blk.conv_s[0])
    p.conv_s[1] = gc_weights(blk.conv_s[1])
    p.conv_t = gc_weights(blk.conv_t[0])
    p.bn = bn_struct(blk.bn)
    p.prelu = ptr(blk.prelu.weight, "prelu.weight")
    if blk.in_channels != blk.out_channels:
        conv, bnw = blk.residual[0], blk.residual[1]
        p.res_w, p.res_b = ptr(conv.weight, "residual.0.weight"), ptr(conv.bias, "residual.0.bias")
        p.res_bn = bn_struct(bnw)
    return p


# ---------------------------------------------------------------------------
# gradient structs (training path)
# ---------------------------------------------------------------------------
class GradArena:
    """One zeroed fp32 buffer with a slice per parameter (the backward kernels
    accumulate into it); ``ptr(p)`` is p's slice, ``views()`` the gradients in
    the order given, None for parameters that do not require grad (A_s, A_t
    and anything frozen)."""

    def __init__(self, params, device, buf=None):
        self.params = list(params)
        self.offsets = {}
        n = 0
        for p in self.params:
            if id(p) not in self.offsets:
                self.offsets[id(p)] = n
                n += (p.numel() + 63) // 64 * 64
        if buf is not None:  # an arena a backward op returned (same params, same layout)
            if buf.numel() != max(n, 1):
                raise ValueError(f"gradient arena of {buf.numel()} floats for a layout of {max(n, 1)}")
            self.buf = buf
        else:
            self.buf = torch.zeros(max(n, 1), dtype=torch.float32, device=device)

    def ptr(self, p):
        return self.buf.data_ptr() + 4 * self.offsets[id(p)]

    def views(self):
        out = []
        for p in self.params:
            off = self.offsets[id(p)]
            out.append(self.buf[off:off + p.numel()].view(p.shape) if p.requires_grad else None)
        return out


def arena_numel(params):
    """Floats of a GradArena over ``params`` (64-float aligned slices, shared
    tensors once)."""
    seen, n = set(), 0
    for p in params:
        if id(p) not in seen:
            seen.add(id(p))
            n += (p.numel() + 63) // 64 * 64
    return max(n, 1)


def grad_sink(owner, params, device):
    """Where a native backward writes the parameters' gradients.

    Returns (arena, direct).  direct=True: the parameters' ``.grad`` ARE
    slices of ``owner``'s persistent arena and the backward kernels, which
    always accumulate (+=), add into them in place -- the caller returns None
    to autograd for the parameters.  That is torch's accumulate semantics
    without a per-parameter clone / add kernel per backward (a training step
    with the inverse pass runs two backwards into the same gradients:
    engine/prediction.py:267-287).  It holds when every trainable parameter's
    ``.grad`` is None (the arena is zeroed and the views installed) or is
    still the view installed earlier.  Otherwise (gradients set by someone
    else) a fresh zeroed arena is returned with direct=False and the caller
    hands its views to autograd as before."""
    params = params if isinstance(params, list) else list(params)
    dev = torch.device(device)
    arena = getattr(owner, "_dstd_grad_arena", None)
    if (arena is None or len(arena.params) != len(params) or arena.buf.device != dev
            or any(a is not b for a, b in zip(arena.params, params))):
        arena = GradArena(params, device)
        # (parameter, its slice) for every trainable parameter, built once
        arena.pairs = [(q, v) for q, v in zip(arena.params, arena.views()) if v is not None]
        owner._dstd_grad_arena = arena
    pairs = arena.pairs
    grads = [q.grad for q, _ in pairs]
    if all(g is None for g in grads):
        arena.buf.zero_()
        for q, v in pairs:
            q.grad = v
        return arena, True
    if all(g is v for g, (_, v) in zip(grads, pairs)):
        return arena, True
    return GradArena(params, device), False


def gc_grads(dstdgc, arena):
    g = GCGrads()
    for f, conv in (("f", dstdgc.conv_f), ("m1", dstdgc.conv_m1), ("m2", dstdgc.conv_m2), ("rm", dstdgc.conv_rm)):
        setattr(g, "w" + f, arena.ptr(conv.weight))
        setattr(g, "b" + f, arena.ptr(conv.bias))
    return g


def bn_grads(bnw, arena):
    return BNGrads(arena.ptr(bnw.bn.weight), arena.ptr(bnw.bn.bias))


def block_grads(blk, arena):
    g = BlockGrads()
    g.W_s, g.R_s, g.R_t = arena.ptr(blk.W_s), arena.ptr(blk.R_s), arena.ptr(blk.R_t)
    g.alpha_sm, g.alpha_tm = arena.ptr(blk.alpha_sm), arena.ptr(blk.alpha_tm)
    g.conv_s[0] = gc_grads(blk.conv_s[0], arena)
    g.conv_s[1] = gc_grads(blk.conv_s[1], arena)
    g.conv_t = gc_grads(blk.conv_t[0], arena)
    g.bn = bn_grads(blk.bn, arena)
    g.prelu = arena.ptr(blk.prelu.weight)
    if blk.in_channels != blk.out_channels:
        g.res_w, g.res_b = arena.ptr(blk.residual[0].weight), arena.ptr(blk.residual[0].bias)
        g.res_bn = bn_grads(blk.residual[1], arena)
    return g
