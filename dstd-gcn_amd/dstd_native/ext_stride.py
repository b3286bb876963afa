"""The C ABI of include/ext/dstd_gcn_stride.h (predict with a stride), declared
as ext_eval.py and ext_augment.py declare their headers.

A module of its own, for the reason they give: the host tests pin the key sets
and sizes of abi.ABI, abi.C_TYPES, ext.ALL, ext.ABI, ext_eval.ABI and
ext_augment.ABI, so this table adds nothing to any of them.  lib() hands ABI
below to abi.declare together with the others: one loop, one rule for a missing
symbol.  The module is the namespace the header reader (tests/abi_reader.py)
compares the header through.

The header brings no typedef and no constant (C_TYPES is empty;
DSTD_PREDICT_MAX_WINDOWS is include/dstd_gcn_predict.h's, abi.PREDICT_MAX_WINDOWS);
the dstd_model_params of include/dstd_gcn.h is declared as void* and passed by
reference through ext.model_params_ref.
"""
import ctypes

from .ext import model_params_ref  # noqa: F401 -- the parameters go through the same helper

C_TYPES = {}

_i, _u, _z, _p = ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.c_void_p

ABI = {
    "ext/dstd_gcn_stride.h": {
        "dstd_model_predict_strided_workspace_bytes": (_z, [_i, _i, _i, _i, _i]),
        # (p, obs, B, input_n, horizon, stride, out, workspace, workspace_bytes, stream, flags)
        "dstd_model_predict_strided": (_i, [_p, _p, _i, _i, _i, _i, _p, _p, _z, _p, _u]),
    },
}

STRIDE_EXPORTS = tuple(ABI["ext/dstd_gcn_stride.h"])
