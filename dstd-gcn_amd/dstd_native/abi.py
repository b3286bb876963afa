"""The C ABI of include/*.h, declared once: constants, structs, entry points.

A constant is its define without the DSTD_ prefix; C_TYPES maps every struct and
callback typedef to its class; ABI holds, per header, each prototype once as
name: (restype, argtypes).  Nothing here reads the headers: tests/test_abi_host.py
does, and compares every value, field and signature below with them.
"""
import ctypes
from ctypes import POINTER, c_char_p, c_longlong as ll, c_ulonglong as u64

i, u, f, z, p = ctypes.c_int, ctypes.c_uint, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p

# ---- constants --------------------------------------------------------------
OK, EINVAL, EWORKSPACE, ELIMIT, ECOLLECTIVE = 0, -1, -2, -3, -5
MODE_SPATIAL, MODE_TEMPORAL = 0, 1
MAX_LAYERS = 16
# kernel families of a profile (Profile.kind_mask bits, Profile.kinds entries)
KIND_FOLD, KIND_PREP, KIND_ADJ_S, KIND_SPATIAL, KIND_ADJ_T, KIND_TEMPORAL, KIND_BLOCK, KIND_COUNT = range(8)
KIND_NAMES = ("fold", "prep", "adj_spatial", "spatial_gc", "adj_temporal", "temporal_gc", "block")
FWD_REUSE_CONSTANTS = 1
FWD_EXACT_FP32 = 2
FWD_SEPARATE_ADJ = 4
FWD_FUSED_TEMPORAL = 8
FWD_SEPARATE_BLOCK = 16
FWD_SEPARATE_ENCODERS = 32
FWD_SEPARATE_ENDS = 64
# the kinds of a launch schedule's entries (Launch.kind)
(LAUNCH_PREP, LAUNCH_ADJ_S, LAUNCH_SPATIAL, LAUNCH_ADJ_T, LAUNCH_TEMPORAL, LAUNCH_TEMPORAL_FUSED, LAUNCH_BLOCK,
 LAUNCH_ENC_RUN, LAUNCH_MODEL) = range(9)
TRAIN_RUNNING_STATS = 1
TRAIN_PAIRED = 2  # two BatchNorm batches of B/2 (a forward pair)
TRAIN_SEED_DEVICE = 4  # the dropout seed is read from device memory
TRAIN_ONE_STREAM = 8  # no weight-gradient stream in the model backward
COLL_ALLGATHER, COLL_ALLREDUCE_SUM = 0, 1
# term bits; slot k of a values / coef row is bit 1 << k
LOSS_JL2, LOSS_TL2, LOSS_CL1, LOSS_CL2 = 1, 2, 4, 8
LOSS_NTERMS = 4
PREDICT_MAX_WINDOWS = 64


# ---- structs (C_TYPES below names the typedef each one mirrors) ---------------
class GCWeights(ctypes.Structure):
    _fields_ = [(n, p) for n in ("wf", "bf", "wm1", "bm1", "wm2", "bm2", "wrm", "brm")]


class BN(ctypes.Structure):
    _fields_ = [("weight", p), ("bias", p), ("running_mean", p), ("running_var", p), ("eps", f)]


class BlockParams(ctypes.Structure):
    _fields_ = [("cin", i), ("cout", i), ("A_s", p), ("W_s", p), ("R_s", p), ("A_t", p), ("R_t", p),
                ("alpha_sm", p), ("alpha_tm", p), ("conv_s", GCWeights * 2), ("conv_t", GCWeights), ("bn", BN),
                ("prelu", p), ("res_w", p), ("res_b", p), ("res_bn", BN)]


class ModelParams(ctypes.Structure):
    _fields_ = [("T", i), ("V", i), ("num_layers", i), ("num_feature", i), ("in_channels", i),
                ("st_in", BlockParams), ("bn_in", BN), ("prelu", p), ("enc", BlockParams * MAX_LAYERS),
                ("enc_bn", BN * MAX_LAYERS), ("enc_prelu", p * MAX_LAYERS), ("st_out", BlockParams)]


class Profile(ctypes.Structure):
    _fields_ = [("kind_mask", u), ("capacity", i), ("count", i), ("events", POINTER(p)), ("kinds", POINTER(i)),
                ("block", POINTER(i)), ("only_block", i)]


class Launch(ctypes.Structure):
    """One entry of a forward's launch schedule."""
    _fields_ = [("kind", i), ("first_block", i), ("num_blocks", i)]


class BlockTaps(ctypes.Structure):
    """Where one DSTDGCB's taps go (device pointers to dense fp32; None: not
    wanted, not written)."""
    _fields_ = [(n, p) for n in ("adj_s", "adj_t", "x", "h")]


TAP_NAMES = ("adj_s", "adj_t", "x", "h")


class GCGrads(ctypes.Structure):
    _fields_ = [(n, p) for n in ("wf", "bf", "wm1", "bm1", "wm2", "bm2", "wrm", "brm")]


class BNGrads(ctypes.Structure):
    _fields_ = [("weight", p), ("bias", p)]


class BlockGrads(ctypes.Structure):
    _fields_ = [("W_s", p), ("R_s", p), ("R_t", p), ("alpha_sm", p), ("alpha_tm", p), ("conv_s", GCGrads * 2),
                ("conv_t", GCGrads), ("bn", BNGrads), ("prelu", p), ("res_w", p), ("res_b", p), ("res_bn", BNGrads)]


class ModelGrads(ctypes.Structure):
    _fields_ = [("st_in", BlockGrads), ("bn_in", BNGrads), ("prelu", p), ("enc", BlockGrads * MAX_LAYERS),
                ("enc_bn", BNGrads * MAX_LAYERS), ("enc_prelu", p * MAX_LAYERS), ("st_out", BlockGrads)]


COLLECTIVE_FN = ctypes.CFUNCTYPE(i, p, i, p, ll, p)


class BnSyncStruct(ctypes.Structure):
    """Cross-rank BatchNorm (dstd_dist.BnSync)."""
    _fields_ = [("world", i), ("rank", i), ("fn", COLLECTIVE_FN), ("ctx", p), ("buf", p), ("buf_floats", ll)]


class LossProblem(ctypes.Structure):
    """pred [B][T][V][3] against targ [B][targ_T][V][3], pred frame s <-> targ
    frame targ_t0 + targ_step * s."""
    _fields_ = [("pred", p), ("targ", p), ("B", i), ("T", i), ("V", i), ("targ_T", i), ("targ_t0", i),
                ("targ_step", i)]


class SeqStore(ctypes.Structure):
    """Frames [F][D] resident on the device, windows as start rows, and the
    tables a batch is gathered through."""
    _fields_ = [("frames", p), ("used", p), ("starts", p), ("F", ll), ("N", ll), ("T", i), ("D", i), ("Du", i),
                ("dim_used", p), ("frame_in", p), ("frame_inv", p), ("mirror_src", p)]


C_TYPES = {"dstd_gc_weights": GCWeights, "dstd_bn": BN, "dstd_block_params": BlockParams,
           "dstd_model_params": ModelParams, "dstd_profile": Profile, "dstd_launch": Launch,
           "dstd_block_taps": BlockTaps, "dstd_gc_grads": GCGrads, "dstd_bn_grads": BNGrads,
           "dstd_block_grads": BlockGrads, "dstd_model_grads": ModelGrads, "dstd_collective_fn": COLLECTIVE_FN,
           "dstd_bn_sync": BnSyncStruct, "dstd_loss_problem": LossProblem, "dstd_seq_store": SeqStore}

# ---- entry points: header -> name -> (restype, argtypes), in header order -----
GW, GG = POINTER(GCWeights), POINTER(GCGrads)
BP, BG, BT = POINTER(BlockParams), POINTER(BlockGrads), POINTER(BlockTaps)
MP, MG = POINTER(ModelParams), POINTER(ModelGrads)
PR, SY, LP = POINTER(Profile), POINTER(BnSyncStruct), POINTER(LossProblem)

ABI = {
    "dstd_gcn.h": {
        "dstd_version": (c_char_p, []),
        "dstd_source_hash": (c_char_p, []),
        "dstd_error_string": (c_char_p, [i]),
        "dstd_dstdgc_workspace_bytes": (z, [i, i, i, i, i, i]),
        "dstd_block_workspace_bytes": (z, [i, i, i, i, i]),
        "dstd_model_workspace_bytes": (z, [i, i, i, i, i]),
        "dstd_dstdgc_fwd": (i, [i, p, i, i, i, i, i, GW, p, p, p, p, z, p]),
        "dstd_block_fwd": (i, [BP, p, i, i, i, p, p, z, p]),
        "dstd_block_fwd_ex": (i, [BP, p, i, i, i, p, p, z, p, u]),
        "dstd_model_fwd": (i, [MP, p, i, p, p, z, p]),
        "dstd_model_fwd_profiled": (i, [MP, p, i, p, p, z, p, PR]),
        "dstd_model_fwd_ex": (i, [MP, p, i, p, p, z, p, u, PR]),
        "dstd_model_fwd_schedule": (i, [i, i, i, i, i, u, i, i, i, POINTER(Launch), i]),
        "dstd_events_create": (i, [i, POINTER(p)]),
        "dstd_events_destroy": (i, [i, POINTER(p)]),
        "dstd_event_elapsed_ms": (i, [p, p, POINTER(f)]),
    },
    "dstd_gcn_train.h": {
        "dstd_dstdgc_train_saved_bytes": (z, [i, i, i, i, i, i]),
        "dstd_dstdgc_train_workspace_bytes": (z, [i, i, i, i, i, i]),
        "dstd_dstdgc_train_fwd": (i, [i, p, i, i, i, i, i, GW, p, p, p, p, z, p]),
        "dstd_dstdgc_train_bwd": (i, [i, p, i, i, i, i, i, GW, p, p, z, p, p, GG, p, p, p, z, p]),
        "dstd_dstdgc_train_saved_bytes_r": (z, [i, i, i, i, i, i, i]),
        "dstd_dstdgc_train_workspace_bytes_r": (z, [i, i, i, i, i, i, i]),
        "dstd_dstdgc_train_fwd_r": (i, [i, p, i, i, i, i, i, i, GW, p, p, p, p, z, p]),
        "dstd_dstdgc_train_bwd_r": (i, [i, p, i, i, i, i, i, i, GW, p, p, z, p, p, GG, p, p, p, z, p]),
        "dstd_block_train_saved_bytes": (z, [i, i, i, i, i]),
        "dstd_block_train_workspace_bytes": (z, [i, i, i, i, i]),
        "dstd_block_train_fwd": (i, [BP, p, i, i, i, f, p, p, z, p]),
        "dstd_block_train_bwd": (i, [BP, p, i, i, i, p, z, p, p, BG, p, z, p]),
        "dstd_block_train_fwd_ex": (i, [BP, p, i, i, i, f, p, p, z, p, u]),
        "dstd_block_train_bwd_ex": (i, [BP, p, i, i, i, p, z, p, p, BG, p, z, p, u]),
        "dstd_model_train_saved_bytes": (z, [i, i, i, i, i]),
        "dstd_model_train_workspace_bytes": (z, [i, i, i, i, i]),
        "dstd_model_train_fwd": (i, [MP, p, i, f, f, u64, p, p, z, p]),
        "dstd_model_train_bwd": (i, [MP, p, i, f, u64, p, z, p, MG, p, z, p]),
        "dstd_model_train_fwd_ex": (i, [MP, p, i, f, f, u64, p, p, z, p, u]),
        "dstd_model_train_bwd_ex": (i, [MP, p, i, f, u64, p, z, p, MG, p, p, z, p, u]),
        "dstd_bn_sync_buffer_floats": (z, [i, i, i]),
        "dstd_model_train_fwd_sync": (i, [MP, p, i, f, f, u64, p, p, z, p, u, SY]),
        "dstd_model_train_bwd_sync": (i, [MP, p, i, f, u64, p, z, p, MG, p, p, z, p, u, SY]),
        "dstd_loss_workspace_bytes": (z, []),
        "dstd_mpjpe_fwd": (i, [p, p, z, p, p, z, p]),
        "dstd_mpjpe_bwd": (i, [p, p, z, p, f, p, p]),
        "dstd_frame_mpjpe": (i, [p, p, i, i, i, i, p, i, p, p, i, p, p]),
        "dstd_debug_aggb_last": (i, []),
        "dstd_debug_bn_last": (i, []),
    },
    "dstd_gcn_aux.h": {
        "dstd_ctg_workspace_bytes": (z, [i, i, i, i]),
        "dstd_ctg_fwd": (i, [p, i, i, i, i, p, p, p, p, p, z, p]),
        "dstd_ctg_bwd": (i, [p, i, i, i, i, p, p, p, p, p, p, p, p, z, p]),
        "dstd_conv2d_workspace_bytes": (z, [i, i, i, i, i, i, i, i, i, i, i]),
        "dstd_conv2d_fwd": (i, [p, i, i, i, i, p, p, i, i, i, i, i, i, i, p, p, z, p]),
        "dstd_conv2d_bwd": (i, [p, i, i, i, i, p, i, i, i, i, i, i, i, p, p, p, p, p, z, p]),
    },
    "dstd_gcn_loss.h": {
        "dstd_losses_workspace_bytes": (z, []),
        "dstd_losses_fwd": (i, [LP, i, u, p, p, p, z, p]),
        "dstd_losses_bwd": (i, [LP, i, u, p, p, f, POINTER(p), p]),
    },
    "dstd_gcn_taps.h": {
        "dstd_block_taps_workspace_bytes": (z, [i, i, i, i, i]),
        "dstd_model_taps_workspace_bytes": (z, [i, i, i, i, i]),
        "dstd_block_fwd_taps": (i, [BP, p, i, i, i, p, BT, p, z, p, u]),
        "dstd_model_fwd_taps": (i, [MP, p, i, p, BT, p, z, p, u]),
    },
    "dstd_gcn_data.h": {
        "dstd_batch_gather": (i, [POINTER(SeqStore), p, i, p, p, p, p, p]),
    },
    "dstd_gcn_predict.h": {
        "dstd_model_predict_workspace_bytes": (z, [i, i, i, i, i]),
        "dstd_model_predict": (i, [MP, p, i, i, i, p, p, z, p, u]),
    },
}

(EXPORTS, TRAIN_EXPORTS, AUX_EXPORTS, LOSS_EXPORTS, TAPS_EXPORTS, DATA_EXPORTS,
 PREDICT_EXPORTS) = (tuple(ABI[h]) for h in ("dstd_gcn.h", "dstd_gcn_train.h", "dstd_gcn_aux.h", "dstd_gcn_loss.h",
                                             "dstd_gcn_taps.h", "dstd_gcn_data.h", "dstd_gcn_predict.h"))
del i, u, f, z, p, ll, u64, GW, GG, BP, BG, BT, MP, MG, PR, SY, LP  # shorthand of this file only


def declare(L, allow_missing=False, extra=None):
    """Give every entry point of ABI -- and of ``extra``, a table of the same
    form (dstd_native.ext.ABI) -- its restype and argtypes on the loaded
    library L.  The one rule for a symbol L does not export: it is an error,
    unless allow_missing (an earlier revision's library loaded on purpose),
    when it is skipped."""
    for header, protos in (*ABI.items(), *(extra or {}).items()):
        for name, (restype, argtypes) in protos.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                if allow_missing:
                    continue
                raise RuntimeError(f"{L._name} does not export {name} ({header}): "
                                   "rebuild with `make -C dstd-gcn_amd`") from None
            fn.restype, fn.argtypes = restype, argtypes
