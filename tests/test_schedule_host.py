"""The eval forward's launch schedule (csrc/dstd_plan.h) through
dstd_model_fwd_schedule with cus=256: integers in, the launch list out, no GPU.
The table is the schedule every earlier revision ran for these arguments, read
off its host code and its traced kernel sequences
(profiles/r09_schedule_trace.txt); test_gpu_enc_chain.py ties the list to what a
forward really launches."""
import ctypes
import itertools

import pytest

import dstd_native as native

PREP, ADJ_S, SPATIAL, ADJ_T, TEMPORAL, TFUSED, BLOCK, ENC_RUN, MODEL = range(9)
H36M, CMU, PW3D = (35, 22), (35, 25), (40, 23)
ADJ, FUSED, SBLOCK, ENCODERS, ENDS = (native.FWD_SEPARATE_ADJ, native.FWD_FUSED_TEMPORAL, native.FWD_SEPARATE_BLOCK,
                                      native.FWD_SEPARATE_ENCODERS, native.FWD_SEPARATE_ENDS)
EXACT, REUSE = native.FWD_EXACT_FP32, native.FWD_REUSE_CONSTANTS
CUS = 256


def plan(B, TV, L=5, flags=0, profiled=False, taps=0, C=64):
    return native.model_schedule(B, TV[0], TV[1], C, L, flags, profiled, taps, CUS)


def one(kind, b):
    return [(kind, b, 1)]


def unit(n):
    return [e for b in range(n) for k in (ADJ_S, SPATIAL, ADJ_T, TEMPORAL) for e in one(k, b)]


def blocks(bs):
    return [e for b in bs for e in one(BLOCK, b)]


PREP1 = [(PREP, -1, 0)]


def test_launch_constants_match_the_header():
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "dstd_gcn.h")).read()
    got = dict(re.findall(r"#define DSTD_LAUNCH_(\w+) (\d+)", src))
    names = ["PREP", "ADJ_S", "SPATIAL", "ADJ_T", "TEMPORAL", "TEMPORAL_FUSED", "BLOCK", "ENC_RUN", "MODEL"]
    assert got == {n: str(i) for i, n in enumerate(names)}
    assert [getattr(native, "LAUNCH_" + n) for n in names] == list(range(9))


@pytest.mark.parametrize("tv", [H36M, CMU, PW3D])
def test_default_schedules_of_the_three_configs(tv):
    """Rows 1-3 (and 19: the same at CMU and 3DPW)."""
    assert plan(256, tv) == [(MODEL, 0, 7)]
    assert plan(256, tv, flags=ENDS) == one(BLOCK, 0) + [(ENC_RUN, 1, 5)] + one(BLOCK, 6)
    assert plan(256, tv, flags=ENCODERS) == blocks(range(7))


def test_flag_rows():
    """Rows 4-11."""
    # 4: block 0's planes in a launch of their own, every later block's from the previous temporal launch
    assert plan(256, H36M, flags=SBLOCK) == one(ADJ_S, 0) + [e for b in range(7) for e in one(SPATIAL, b) + one(TFUSED, b)]
    assert len(plan(256, H36M, flags=SBLOCK)) == 15
    assert plan(256, H36M, flags=ADJ) == [e for b in range(7) for e in one(ADJ_S, b) + one(BLOCK, b)]
    assert plan(255, H36M) == unit(7)  # below one sample per CU
    assert plan(255, H36M, flags=FUSED) == [(MODEL, 0, 7)]
    assert plan(256, H36M, profiled=True) == blocks(range(7))
    assert plan(256, H36M, taps=1) == unit(7)
    assert plan(256, H36M, taps=3) == PREP1 + unit(7)
    assert plan(256, H36M, flags=EXACT) == PREP1 + unit(7)


def test_length_rows():
    """Rows 12-18: no encoder, the shortest and (row 1) longest one-launch
    forward, runs of at most 8, a left-over single encoder block."""
    assert plan(256, H36M, L=0) == blocks([0, 1])
    assert plan(256, H36M, L=1) == [(MODEL, 0, 3)]
    assert plan(256, H36M, L=1, flags=ENDS) == blocks([0, 1, 2])
    assert plan(256, H36M, L=6) == one(BLOCK, 0) + [(ENC_RUN, 1, 6)] + one(BLOCK, 7)
    assert plan(256, H36M, L=9) == one(BLOCK, 0) + [(ENC_RUN, 1, 8)] + blocks([9, 10])
    assert plan(256, H36M, L=10) == one(BLOCK, 0) + [(ENC_RUN, 1, 8), (ENC_RUN, 9, 2)] + one(BLOCK, 11)
    assert plan(256, H36M, L=16) == one(BLOCK, 0) + [(ENC_RUN, 1, 8), (ENC_RUN, 9, 8)] + one(BLOCK, 17)


def test_shapes_off_the_split_kernels():
    """Rows 20-23."""
    # 20: no split kernel off 64 channels -- but conv_st_out's temporal GC runs
    # on its 3 output channels whatever feeds it, so that one stays split and,
    # at full batch, fused
    assert plan(256, H36M, C=32) == PREP1 + unit(6) + one(ADJ_S, 6) + one(SPATIAL, 6) + one(TFUSED, 6)
    assert plan(255, H36M, C=32) == PREP1 + unit(7)
    # 21: the fused temporal kernel is not the default at T = 75
    assert plan(256, (75, 22)) == unit(7)
    # 22: and when asked for has no phase 3 (every block builds its own planes) and no whole-block launch
    assert plan(256, (75, 22), flags=FUSED) == [e for b in range(7)
                                               for e in one(ADJ_S, b) + one(SPATIAL, b) + one(TFUSED, b)]
    # 23: inside the envelope, no split kernels at all
    assert plan(256, (35, 23)) == PREP1 + unit(7)
    assert plan(256, (128, 32), flags=FUSED) == PREP1 + unit(7)


def closure(flags, profiled):
    """include/dstd_gcn.h: what each flag implies."""
    if profiled or flags & (ADJ | SBLOCK):
        flags |= ENCODERS
    if flags & ENCODERS:
        flags |= ENDS
    return flags


FLAG_SETS = [sum(c) for r in range(6) for c in itertools.combinations((ADJ, FUSED, SBLOCK, ENCODERS, ENDS), r)]


@pytest.mark.parametrize("tv", [H36M, CMU, PW3D])
def test_schedule_properties(tv):
    assert len(FLAG_SETS) == 32
    for L, flags, B, profiled in itertools.product(range(17), FLAG_SETS, (1, 255, 256), (False, True)):
        at = (tv, L, flags, B, profiled)
        p = plan(B, tv, L, flags, profiled)
        # blocks 0..L+1 in order, no gap, no overlap; a block's own launches in their order, ending in its temporal GC
        nxt, last = 0, None
        for kind, b, n in p:
            assert kind != PREP, at  # the split kernels read the model input themselves
            if n == 1 and kind not in (ENC_RUN, MODEL):
                if b == nxt - 1:
                    assert last is not None and last < kind and last not in (TEMPORAL, TFUSED, BLOCK), (at, p)
                else:
                    assert b == nxt and last in (None, TEMPORAL, TFUSED, BLOCK), (at, p)
                    nxt = b + 1
                last = kind
            else:
                assert b == nxt and last in (None, TEMPORAL, TFUSED, BLOCK), (at, p)
                nxt, last = b + n, None
        assert nxt == L + 2 and last in (None, TEMPORAL, TFUSED, BLOCK), (at, p)
        if any(k == MODEL for k, _, _ in p):
            assert p == [(MODEL, 0, L + 2)], at
            assert not flags & (ADJ | SBLOCK | ENCODERS | ENDS) and not profiled and 1 <= L <= 5, at
        for kind, b, n in p:
            if kind == ENC_RUN:
                assert 2 <= n <= 8 and b >= 1 and b + n <= L + 1, (at, p)
                assert not flags & (ADJ | SBLOCK | ENCODERS) and not profiled, at
        assert plan(B, tv, L, closure(flags, profiled), profiled) == p, at
        assert plan(B, tv, L, flags | REUSE, profiled) == p, at


def test_invalid_arguments_as_the_forward():
    """The integer checks of dstd_model_fwd_ex, with the same codes (the
    forward sees them before it touches any pointer)."""
    L = native.lib()
    out = (native.Launch * 4)()
    bad = [(0, 35, 22, 64, 5), (4, 1, 22, 64, 5), (4, 35, 0, 64, 5), (4, 35, 22, 64, -1), (4, 35, 22, 64, 17),
           (4, 129, 22, 64, 5), (4, 35, 33, 64, 5), (4, 35, 22, 65, 5), (4, 35, 22, 0, 5)]
    good = (256, 35, 22, 64, 5)
    dummy = ctypes.c_void_p(256)  # never dereferenced: the shape is refused first
    for B, T, V, C, layers in bad:
        mp = native.ModelParams()
        mp.T, mp.V, mp.num_layers, mp.num_feature, mp.in_channels = T, V, layers, C, 6
        want = L.dstd_model_fwd_ex(ctypes.byref(mp), dummy, B, dummy, dummy, 1 << 40, None, 0, None)
        assert want in (-1, -3), (B, T, V, C, layers)
        assert L.dstd_model_fwd_schedule(B, T, V, C, layers, 0, 0, 0, CUS, out, 4) == want, (B, T, V, C, layers)
    assert L.dstd_model_fwd_schedule(*good, 128, 0, 0, CUS, out, 4) == -1  # an unknown flag
    assert L.dstd_model_fwd_ex(None, None, 4, None, None, 0, None, 128, None) == -1
    assert L.dstd_model_fwd_schedule(*good, ENDS, 0, 1, CUS, out, 4) == -1  # the tap entry takes EXACT_FP32 only
    assert L.dstd_model_fwd_schedule(*good, 0, 0, 0, CUS, None, 4) == -1
    # the count does not depend on the capacity; nothing is written past it
    out[1].kind = 77
    assert L.dstd_model_fwd_schedule(*good, ENDS, 0, 0, CUS, out, 1) == 3
    assert (out[0].kind, out[0].first_block, out[0].num_blocks) == (BLOCK, 0, 1) and out[1].kind == 77
    assert L.dstd_model_fwd_schedule(*good, ENDS, 0, 0, CUS, None, 0) == 3
