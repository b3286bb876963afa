"""The C ABI of include/ext/dstd_gcn_eval.h (grouped evaluation of a resident
set), declared as ext.py declares its headers.

A module of its own: tests/test_teacher_host.py pins the key set of ext.ALL and
tests/test_rollout_host.py pins ext.ABI, so this table adds nothing to ext.*,
abi.ABI or abi.C_TYPES.  lib() hands ABI below to abi.declare together with
ext.ALL: one loop, one rule for a missing symbol.  The module is the namespace
the header reader (tests/abi_reader.py) compares the header through: ABI,
C_TYPES and the header's one constant.

The header brings no typedef (C_TYPES is empty) and this namespace holds no
Structure class; the dstd_seq_store of include/dstd_gcn_data.h is declared as
void* and passed by reference through seq_store_ref.
"""
import ctypes

from . import abi
from .ext import struct_ref

C_TYPES = {}
EVAL_MAX_GROUPS = 1024

_i, _p = ctypes.c_int, ctypes.c_void_p

ABI = {
    "ext/dstd_gcn_eval.h": {
        # (store, index, B, outputs, t_out0, used_pos, n_used, joint_src, frames, n_frames, group, n_groups,
        #  sums, counts, stream)
        "dstd_store_group_mpjpe": (_i, [_p, _p, _i, _p, _i, _p, _i, _p, _p, _i, _p, _i, _p, _p, _p]),
    },
}

EVAL_EXPORTS = tuple(ABI["ext/dstd_gcn_eval.h"])


def seq_store_ref(s):
    return struct_ref(s, abi.SeqStore)
