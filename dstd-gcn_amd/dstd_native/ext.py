"""The C ABI of include/ext/*.h, declared once as abi.py declares include/*.h.

A table of its own: tests/test_abi_host.py pins the key set and the sizes of
abi.ABI / abi.C_TYPES, so this module adds nothing to either and is not
star-imported into dstd_native (``dstd_native.ext`` names it).  lib() hands
ALL below to abi.declare with abi.ABI: one loop, one rule for a missing symbol.

The extension headers bring no typedef, so C_TYPES is empty, and this
namespace holds no Structure class: the reader that compares a header with its
binding (tests/abi_reader.py) resolves struct names through the C_TYPES of the
binding it is given.  A pointer to a struct of include/*.h is therefore
declared as void* here; callers pass the abi.py Structure itself (the
wrappers below take it by reference), whose layout tests/test_abi_host.py
settles.
"""
import ctypes
import types

from . import abi

C_TYPES = {}

_i, _u, _f, _z, _p = ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p

ABI = {
    "ext/dstd_gcn_rollout.h": {
        "dstd_model_rollout_saved_bytes": (_z, [_i, _i, _i, _i, _i, _i]),
        "dstd_model_rollout_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
        # (p, obs, B, input_n, horizon, momentum, dropout_p, seeds, out, saved, saved_bytes, stream, flags)
        "dstd_model_rollout_fwd": (_i, [_p, _p, _i, _i, _i, _f, _f, _p, _p, _p, _z, _p, _u]),
        # (p, B, input_n, horizon, dropout_p, seeds, saved, saved_bytes, dout, g, dobs, workspace,
        #  workspace_bytes, stream, flags)
        "dstd_model_rollout_bwd": (_i, [_p, _i, _i, _i, _f, _p, _p, _z, _p, _p, _p, _p, _z, _p, _u]),
        # (p, B, input_n, horizon, k, ... as dstd_model_rollout_bwd)
        "dstd_model_rollout_bwd_window": (_i, [_p, _i, _i, _i, _i, _f, _p, _p, _z, _p, _p, _p, _p, _z, _p, _u]),
        # (step, dout, Gn, dst, B, T, input_n, V, horizon, k, stream)
        "dstd_model_rollout_glue_bwd": (_i, [_i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    },
}

ROLLOUT_EXPORTS = tuple(ABI["ext/dstd_gcn_rollout.h"])

# include/ext/dstd_gcn_teacher.h, in a table of its own: tests/test_rollout_host.py
# pins ABI above to the rollout header alone.  `teacher` is the namespace the
# header reader compares it through (ABI, C_TYPES), and lib() declares both.
_tf = [_p, _i, _p, _p, _p]  # (truth, truth_T, t0, step, mask)
TEACHER_ABI = {
    "ext/dstd_gcn_teacher.h": {
        # (p, obs, B, input_n, horizon, momentum, dropout_p, seeds, out, saved, saved_bytes, <teacher>, stream, flags)
        "dstd_model_rollout_tf_fwd": (_i, [_p, _p, _i, _i, _i, _f, _f, _p, _p, _p, _z, *_tf, _p, _u]),
        # (p, B, input_n, horizon, dropout_p, seeds, saved, saved_bytes, dout, g, dobs, workspace,
        #  workspace_bytes, <teacher>, stream, flags)
        "dstd_model_rollout_tf_bwd": (_i, [_p, _i, _i, _i, _f, _p, _p, _z, _p, _p, _p, _p, _z, *_tf, _p, _u]),
        # (p, B, input_n, horizon, k, ... as dstd_model_rollout_tf_bwd)
        "dstd_model_rollout_tf_bwd_window": (_i, [_p, _i, _i, _i, _i, _f, _p, _p, _z, _p, _p, _p, _p, _z, *_tf, _p, _u]),
        # (step, dout, Gn, dst, mask_row, B, T, input_n, V, horizon, k, stream)
        "dstd_model_rollout_tf_glue_bwd": (_i, [_i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    },
}

TEACHER_EXPORTS = tuple(TEACHER_ABI["ext/dstd_gcn_teacher.h"])
teacher = types.SimpleNamespace(ABI=TEACHER_ABI, C_TYPES={})
ALL = {**ABI, **TEACHER_ABI}  # what lib() declares


def frame_maps(maps):
    """[(t0, step)] of one or two halves as the (t0, step) host arrays of the
    teacher entry points (two ints each; a missing second half is zeros)."""
    maps = list(maps) + [(0, 0)] * (2 - len(maps))
    return (ctypes.c_int * 2)(*(int(m[0]) for m in maps)), (ctypes.c_int * 2)(*(int(m[1]) for m in maps))


def struct_ref(s, cls):
    """``s`` (an abi.py Structure of class ``cls``) as the void* argument of an
    entry point above; anything else is a TypeError here, not a crash there."""
    if not isinstance(s, cls):
        raise TypeError(f"expected {cls.__name__}, got {type(s).__name__}")
    return ctypes.byref(s)


def model_params_ref(p):
    return struct_ref(p, abi.ModelParams)


def model_grads_ref(g):
    return struct_ref(g, abi.ModelGrads)
