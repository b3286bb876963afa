"""The C ABI of include/ext/dstd_gcn_stride_train.h (train through a strided
rollout, with scheduled sampling), declared as ext_stride.py declares its
header.

A module of its own, for the reason ext_stride.py gives: the host tests pin the
key sets and sizes of abi.ABI, abi.C_TYPES, ext.ALL, ext.ABI, ext_eval.ABI,
ext_augment.ABI and ext_stride.ABI, so this table adds nothing to any of them.
lib() hands ABI below to abi.declare together with the others: one loop, one
rule for a missing symbol.  The module is the namespace the header reader
(tests/abi_reader.py) compares the header through.

The header brings no typedef and no constant (C_TYPES is empty); the
dstd_model_params / dstd_model_grads of include/*.h are declared as void* and
passed by reference through ext.model_params_ref / ext.model_grads_ref, and the
teacher's frame maps are built by ext.frame_maps.
"""
import ctypes

from .ext import frame_maps, model_grads_ref, model_params_ref  # noqa: F401 -- the same helpers

C_TYPES = {}

_i, _u, _f, _z, _p = ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p
_tf = [_p, _i, _p, _p, _p]  # (truth, truth_T, t0, step, mask)

ABI = {
    "ext/dstd_gcn_stride_train.h": {
        # (B, T, V, num_feature, num_layers, input_n, horizon)
        "dstd_model_rollout_strided_workspace_bytes": (_z, [_i, _i, _i, _i, _i, _i, _i]),
        # (p, obs, B, input_n, horizon, stride, momentum, dropout_p, seeds, out, saved, saved_bytes, <teacher>,
        #  stream, flags)
        "dstd_model_rollout_strided_fwd": (_i, [_p, _p, _i, _i, _i, _i, _f, _f, _p, _p, _p, _z, *_tf, _p, _u]),
        # (p, B, input_n, horizon, stride, dropout_p, seeds, saved, saved_bytes, dout, g, dobs, workspace,
        #  workspace_bytes, <teacher>, stream, flags)
        "dstd_model_rollout_strided_bwd": (_i, [_p, _i, _i, _i, _i, _f, _p, _p, _z, _p, _p, _p, _p, _z, *_tf, _p, _u]),
        # (p, B, input_n, horizon, stride, k, ... as dstd_model_rollout_strided_bwd)
        "dstd_model_rollout_strided_bwd_window": (_i, [_p, _i, _i, _i, _i, _i, _f, _p, _p, _z, _p, _p, _p, _p, _z, *_tf,
                                                       _p, _u]),
        # (step, dout, dx, Gh, dst, mask_row, B, T, input_n, V, horizon, stride, k, stream)
        "dstd_model_rollout_strided_glue_bwd": (_i, [_i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p]),
    },
}

STRIDE_TRAIN_EXPORTS = tuple(ABI["ext/dstd_gcn_stride_train.h"])
