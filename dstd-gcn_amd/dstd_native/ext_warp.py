"""The C ABI of include/ext/dstd_gcn_warp.h (the warping gather of a resident
set: windows resampled in time inside the gather), declared as ext_augment.py
declares its header.

A module of its own, for the reason ext_eval.py gives: the host tests pin the
key sets and sizes of abi.ABI, abi.C_TYPES, ext.ALL, ext.ABI, ext_eval.ABI,
ext_augment.ABI, ext_stride.ABI and ext_stride_train.ABI, so this table adds
nothing to any of them.  lib() hands ABI below to abi.declare together with the
others: one loop, one rule for a missing symbol.  The module is the namespace
the header reader (tests/abi_reader.py) compares the header through.

The header brings no typedef and no constant (C_TYPES is empty); the
dstd_seq_store of include/dstd_gcn_data.h is declared as void* and passed by
reference through ext_eval.seq_store_ref.
"""
import ctypes

from .ext_eval import seq_store_ref  # noqa: F401 -- the store goes through the same helper

C_TYPES = {}

_i, _f, _u64, _p = ctypes.c_int, ctypes.c_float, ctypes.c_ulonglong, ctypes.c_void_p

ABI = {
    "ext/dstd_gcn_warp.h": {
        # (store, room, index, B, rate, xf, noise_amp, seed, inputs, inputs_inv, targets, all_seqs, stream)
        "dstd_batch_gather_warp": (_i, [_p, _p, _p, _i, _p, _p, _f, _u64, _p, _p, _p, _p, _p]),
    },
}

WARP_EXPORTS = tuple(ABI["ext/dstd_gcn_warp.h"])
