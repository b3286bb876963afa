"""The ctypes binding (dstd_native.abi) against the public headers, all of it.

Every prototype of include/*.h is in the binding's table under its header with
the same arity, parameter types and return type, and the built library exports
it; every struct typedef has a Structure with the same field names, order,
types and array lengths (nested structs by class), dstd_collective_fn has
COLLECTIVE_FN; every integer DSTD_* define has its Python name with that value.

No compiler is invoked.  With equal field lists and no _pack_, ctypes lays a
Structure out by the platform's C rules, the ones the compiler of the library
follows, so equal fields settle sizes, alignments and offsets.  The reader is
tests/abi_reader.py; the cases at the end alter header text in memory and
require each alteration to be reported under the name it touches, so a reader
that matches nothing, or a comparison that accepts anything, fails here.
"""
import glob
import os

import pytest

from abi_reader import compare, int_defines, parse
from conftest import ROOT
import dstd_native as native

PROTOTYPES = {"dstd_gcn.h": 16, "dstd_gcn_train.h": 29, "dstd_gcn_aux.h": 6, "dstd_gcn_loss.h": 3,
              "dstd_gcn_taps.h": 4, "dstd_gcn_data.h": 1, "dstd_gcn_predict.h": 2}
N_STRUCTS = 14  # dstd_launch among them
# dstd_gcn.h 32 (5 codes, 2 modes, MAX_LAYERS, 8 kinds, 7 flags, 9 launches), train 6, loss 5, predict 1
N_INT_DEFINES = 44


@pytest.fixture(scope="module")
def headers():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))}


def test_reader_finds_everything_the_headers_hold(headers):
    parsed = {h: parse(t) for h, t in headers.items()}
    assert {h: len(p[3]) for h, p in parsed.items()} == PROTOTYPES
    assert sum(PROTOTYPES.values()) == 61
    assert sum(len(p[1]) for p in parsed.values()) == N_STRUCTS
    assert [k for p in parsed.values() for k in p[2]] == ["dstd_collective_fn"]
    ints = int_defines({k: v for p in parsed.values() for k, v in p[0].items()})
    assert len(ints) == N_INT_DEFINES, sorted(ints)
    assert (ints["DSTD_EINVAL"], ints["DSTD_FWD_SEPARATE_ENDS"], ints["DSTD_MAX_LAYERS"]) == (-1, 64, 16)
    # the shapes of C the reader has to get right
    s = parsed["dstd_gcn.h"][1]
    assert s["dstd_launch"] == [(n, "int", 0, None) for n in ("kind", "first_block", "num_blocks")]
    assert s["dstd_block_params"][:3] == [("cin", "int", 0, None), ("cout", "int", 0, None), ("A_s", "float", 1, None)]
    assert ("conv_s", "dstd_gc_weights", 0, "2") in s["dstd_block_params"]
    assert ("enc_prelu", "float", 1, "DSTD_MAX_LAYERS") in s["dstd_model_params"]
    assert ("events", "void", 2, None) in s["dstd_profile"]
    assert ("F", "long long", 0, None) in parsed["dstd_gcn_data.h"][1]["dstd_seq_store"]
    assert parsed["dstd_gcn_train.h"][2]["dstd_collective_fn"] == (("int", 0), [
        ("void", 1, "ctx"), ("int", 0, "op"), ("float", 1, "buf"), ("long long", 0, "count"), ("void", 1, "stream")])
    p = parsed["dstd_gcn.h"][3]
    assert p["dstd_version"] == (("char", 1), [])
    assert p["dstd_dstdgc_workspace_bytes"][0] == ("size_t", 0)
    assert p["dstd_model_fwd_ex"][1][-2:] == [("unsigned int", 0, "flags"), ("dstd_profile", 1, "prof")]
    assert ("unsigned long long", 0, "seed") in parsed["dstd_gcn_train.h"][3]["dstd_model_train_fwd"][1]
    assert ("float", 2, "dpreds") in parsed["dstd_gcn_loss.h"][3]["dstd_losses_bwd"][1]


def test_binding_agrees_with_the_headers(headers):
    assert compare(headers, native) == []
    assert len(native.KIND_NAMES) == native.KIND_COUNT
    assert (native.MAX_LAYERS, native.PREDICT_MAX_WINDOWS, native.LOSS_NTERMS) == (16, 64, 4)
    assert sum(isinstance(t, type) and issubclass(t, native.ctypes.Structure)
               for t in native.C_TYPES.values()) == N_STRUCTS


def test_library_exports_the_table_and_carries_its_signatures():
    L = native.lib()
    assert set(native.ABI) == set(PROTOTYPES)
    for h, table in native.ABI.items():
        assert len(table) == PROTOTYPES[h], h
        for name, (restype, argtypes) in table.items():
            assert hasattr(L, name), name
            fn = getattr(L, name)
            assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    for tup, h in ((native.EXPORTS, "dstd_gcn.h"), (native.TRAIN_EXPORTS, "dstd_gcn_train.h"),
                   (native.AUX_EXPORTS, "dstd_gcn_aux.h"), (native.LOSS_EXPORTS, "dstd_gcn_loss.h"),
                   (native.TAPS_EXPORTS, "dstd_gcn_taps.h"), (native.DATA_EXPORTS, "dstd_gcn_data.h"),
                   (native.PREDICT_EXPORTS, "dstd_gcn_predict.h")):
        assert tup == tuple(native.ABI[h])


def test_a_missing_symbol_is_an_error_unless_the_library_is_foreign_on_purpose():
    class Lib:  # a library that exports one symbol only
        _name = "libold.so"

        def __init__(self):
            self.dstd_version = lambda: None

    with pytest.raises(RuntimeError, match=r"libold\.so does not export dstd_source_hash \(dstd_gcn\.h\)"):
        native.declare(Lib())
    old = Lib()
    native.declare(old, allow_missing=True)
    assert old.dstd_version.restype is native.ctypes.c_char_p and old.dstd_version.argtypes == []


def _alter(text, marker, old, new):
    """text with the first `old` after `marker` replaced; both must be there."""
    at = text.index(marker)
    assert old in text[at:], (marker, old)
    return text[:at] + text[at:].replace(old, new, 1)


ALTERATIONS = {
    "two parameters swapped": ("dstd_gcn_train.h", "int dstd_model_train_bwd_ex(", "int B, float dropout_p",
                               "float dropout_p, int B", {"dstd_model_train_bwd_ex"}),
    "int turned into size_t": ("dstd_gcn.h", "int dstd_block_fwd(", "int B", "size_t B", {"dstd_block_fwd"}),
    "parameter dropped": ("dstd_gcn_data.h", "int dstd_batch_gather(", "float* all_seqs, ", "", {"dstd_batch_gather"}),
    "parameter added": ("dstd_gcn_predict.h", "int dstd_model_predict(", "unsigned flags", "unsigned flags, int k",
                        {"dstd_model_predict"}),
    "return type changed": ("dstd_gcn_train.h", "size_t dstd_loss_workspace_bytes(", "size_t", "int",
                            {"dstd_loss_workspace_bytes"}),
    "prototype added": ("dstd_gcn_aux.h", "size_t dstd_ctg_workspace_bytes(", "size_t dstd_ctg_workspace_bytes(",
                        "int dstd_ctg_new(int B);\nsize_t dstd_ctg_workspace_bytes(", {"dstd_ctg_new"}),
    "prototype removed": ("dstd_gcn_taps.h", "size_t dstd_model_taps_workspace_bytes(",
                          "size_t dstd_model_taps_workspace_bytes(int B, int T, int V, int num_feature, "
                          "int num_layers);", "", {"dstd_model_taps_workspace_bytes"}),
    "two struct fields swapped": ("dstd_gcn.h", "typedef struct dstd_block_params",
                                  "  dstd_gc_weights conv_t;\n  dstd_bn bn;",
                                  "  dstd_bn bn;\n  dstd_gc_weights conv_t;", {"dstd_block_params"}),
    "struct field added": ("dstd_gcn_data.h", "typedef struct dstd_seq_store", "int T, D, Du;", "int T, D, Du, pad;",
                           {"dstd_seq_store"}),
    "struct field type changed": ("dstd_gcn_data.h", "typedef struct dstd_seq_store", "long long F, N;", "int F, N;",
                                  {"dstd_seq_store"}),
    "array length changed": ("dstd_gcn.h", "typedef struct dstd_block_params", "conv_s[2]", "conv_s[3]",
                             {"dstd_block_params"}),
    "struct added": ("dstd_gcn_loss.h", "typedef struct dstd_loss_problem", "typedef struct dstd_loss_problem",
                     "typedef struct dstd_extra { int a; } dstd_extra;\ntypedef struct dstd_loss_problem",
                     {"dstd_extra"}),
    "callback parameter changed": ("dstd_gcn_train.h", "typedef int (*dstd_collective_fn)", "long long count",
                                   "int count", {"dstd_collective_fn"}),
    "DSTD_MAX_LAYERS changed": ("dstd_gcn.h", "#define DSTD_MAX_LAYERS", "16", "12",
                                {"DSTD_MAX_LAYERS", "dstd_model_params", "dstd_model_grads"}),
    "flag value changed": ("dstd_gcn.h", "#define DSTD_FWD_EXACT_FP32", "2u", "3u", {"DSTD_FWD_EXACT_FP32"}),
    "error code changed": ("dstd_gcn.h", "#define DSTD_ELIMIT", "-3", "-4", {"DSTD_ELIMIT"}),
    "define added": ("dstd_gcn_loss.h", "#define DSTD_LOSS_NTERMS", "#define DSTD_LOSS_NTERMS",
                     "#define DSTD_LOSS_CL3 16u\n#define DSTD_LOSS_NTERMS", {"DSTD_LOSS_CL3"}),
}


@pytest.mark.parametrize("what", sorted(ALTERATIONS))
def test_an_altered_header_is_reported_by_name(headers, what):
    h, marker, old, new, names = ALTERATIONS[what]
    altered = dict(headers, **{h: _alter(headers[h], marker, old, new)})
    reports = compare(altered, native)
    assert {r.split(":")[0] for r in reports} == names, reports
