"""Host-side checks of tests/guard_helper.py (the guard-band harness of
tests/test_gpu_guards.py) on CPU tensors, and of every ``*_workspace_bytes`` /
``*_saved_bytes`` export of the five headers as pure host arithmetic on the
loaded library (no GPU needed)."""
import os
import re

import pytest
import torch

import dstd_native as native
import envelope_cases as E
import guard_helper as G
from conftest import ROOT


# ---- the harness itself -----------------------------------------------------------
@pytest.mark.parametrize("nbytes", [1, 255, 256, 1000, 4096])
def test_guarded_layout(nbytes):
    g = G.Guarded(nbytes, 0x4B)
    assert g.tensor.numel() == nbytes and g.tensor.dtype == torch.uint8
    assert g.ptr % 256 == 0 and g.tensor.data_ptr() == g.ptr
    assert g.raw.numel() == 2 * G.GUARD + G.rup(nbytes, 256)
    assert bool((g.tensor == 0x4B).all())
    assert g.damage() == {}
    g.check("fresh")


def test_write_inside_is_not_flagged():
    g = G.Guarded(1000, 0x00)
    g.tensor[0] = 7
    g.tensor[999] = 7
    g.view(torch.float32, (5, 50)).fill_(3.0)
    assert g.damage() == {}
    g.check("inside")


def test_write_one_byte_before_is_caught_and_located():
    g = G.Guarded(1000, 0x00)
    g.raw[G.GUARD - 1] = 0
    assert g.damage() == {"before": (-1, -1)}
    with pytest.raises(G.GuardError, match=r"before the buffer, bytes -1\.\.-1"):
        g.check("y")


@pytest.mark.parametrize("nbytes", [1000, 1024])  # with and without a pad up to the next 256
def test_write_one_byte_after_is_caught_and_located(nbytes):
    g = G.Guarded(nbytes, 0xFF)
    g.raw[G.GUARD + nbytes] = 0
    assert g.damage() == {"after": (nbytes, nbytes)}
    with pytest.raises(G.GuardError, match=rf"after the buffer, bytes {nbytes}\.\.{nbytes}"):
        g.check("y")


def test_damage_reports_first_and_last_offset():
    g = G.Guarded(1000, 0x00)
    g.raw[G.GUARD + 1001] = 1  # in the pad up to 1024
    g.raw[G.GUARD + 1024 + 77] = 1  # in the guard proper
    g.raw[G.GUARD - 300] = 1
    g.raw[G.GUARD - 5] = 1
    assert g.damage() == {"before": (-300, -5), "after": (1001, 1024 + 77)}
    far = G.Guarded(512, 0x00)
    far.raw[-1] = 0
    far.raw[0] = 0
    assert far.damage() == {"before": (-G.GUARD, -G.GUARD), "after": (512 + G.GUARD - 1, 512 + G.GUARD - 1)}


def test_a_write_of_the_sentinels_own_byte_is_no_damage_but_any_other_is():
    """The comparison is on integers: every byte value but the one already
    there is seen, whichever byte of the word it hits."""
    want = list(G.SENTINEL.to_bytes(4, "little"))
    for k in range(4):
        g = G.Guarded(256, 0x00)
        g.raw[G.GUARD + 256 + k] = want[k]
        assert g.damage() == {}
        g.raw[G.GUARD + 256 + k] = want[k] ^ 1
        assert g.damage() == {"after": (256 + k, 256 + k)}


def test_fills_are_what_they_claim():
    assert G.FILLS == (0x00, 0xFF, 0x4B)
    z, n, f = (G.Guarded(64, fill) for fill in G.FILLS)
    assert bool((z.view(torch.float32, (16,)) == 0).all()) and bool((z.view(torch.float16, (32,)) == 0).all())
    assert bool(torch.isnan(n.view(torch.float32, (16,))).all()) and bool(torch.isnan(n.view(torch.float16, (32,))).all())
    assert bool((n.view(torch.int32, (16,)) == -1).all())
    f32, f16 = f.view(torch.float32, (16,)), f.view(torch.float16, (32,))
    assert bool(torch.isfinite(f32).all()) and abs(float(f32[0]) - 1.33e7) < 1e5  # 13323083
    assert bool(torch.isfinite(f16).all()) and abs(float(f16[0]) - 14.6) < 0.05  # 14.586
    # the sentinel: a NaN as fp32, and none of its bytes is a fill
    s = torch.tensor([G._as_int32(G.SENTINEL)], dtype=torch.int32)
    assert bool(torch.isnan(s.view(torch.float32)).all())
    assert not set(G.SENTINEL.to_bytes(4, "little")) & set(G.FILLS)
    assert G.GUARD == 1 << 20


def test_context_hands_out_exact_fresh_buffers_and_restores():
    orig = native.workspace, native.workspace_claim
    with G.guarded_workspaces(0x4B, device="cpu") as rec:
        assert native.workspace is not orig[0] and native.workspace_claim is not orig[1]
        a = native.workspace("cpu", 1000)
        b, reused = native.workspace_claim("cpu", 1000, ("tag",))
        c, reused2 = native.workspace_claim("cpu", 1000, ("tag",))
        assert a.numel() == b.numel() == c.numel() == 1000
        assert reused is False and reused2 is False
        assert len({a.data_ptr(), b.data_ptr(), c.data_ptr()}) == 3
        assert all(bool((t == 0x4B).all()) for t in (a, b, c))
        assert [g.nbytes for g in rec.handed] == [1000, 1000, 1000]
        a.fill_(1)  # the whole interior is the caller's
    assert (native.workspace, native.workspace_claim) == orig


def test_context_restores_when_the_body_raises():
    orig = native.workspace, native.workspace_claim
    with pytest.raises(KeyError):
        with G.guarded_workspaces(0x00, device="cpu"):
            native.workspace("cpu", 10)
            raise KeyError("body")
    assert (native.workspace, native.workspace_claim) == orig


def test_context_exit_catches_a_write_past_a_buffer():
    orig = native.workspace, native.workspace_claim
    with pytest.raises(G.GuardError, match=r"workspace 1 of 2 .*after the buffer, bytes 1000\.\.1000"):
        with G.guarded_workspaces(0xFF, device="cpu") as rec:
            native.workspace("cpu", 512)
            native.workspace("cpu", 1000)
            rec.handed[1].raw[G.GUARD + 1000] = 0  # one byte past the 1000 the caller asked for
    assert (native.workspace, native.workspace_claim) == orig


# ---- the size exports -----------------------------------------------------------------
def _size_exports():
    out = {}
    for h in ("dstd_gcn.h", "dstd_gcn_train.h", "dstd_gcn_loss.h", "dstd_gcn_aux.h", "dstd_gcn_taps.h"):
        src = open(os.path.join(ROOT, "include", h)).read()
        for name in re.findall(r"^size_t\s+(dstd_\w+_bytes(?:_r)?)\s*\(", src, re.M):
            out[name] = h
    return out


def _mode(c):
    return native.MODE_SPATIAL if c.mode == "spatial" else native.MODE_TEMPORAL


def _blocks():
    cases = {(c.cin, c.cout, c.T, c.V) for c in E.BLOCK_EVAL_CASES + E.BLOCK_TRAIN_CASES}
    cases |= {(ci, co, T, V) for T, V in G.SPLIT_TV for ci, co in G.SPLIT_CHANNELS}
    return sorted(cases)


def _models():
    return [(T, V, 64, L) for T, V in G.SPLIT_TV for L in G.MODEL_LAYERS] + [(5, 22, 64, 1), (128, 22, 64, 1)]


# export -> the argument tuples of the guarded GPU cases, as functions of B
ARGS = {
    "dstd_dstdgc_workspace_bytes": [lambda B, c=c: (_mode(c), B, c.cin, c.cout, c.T, c.V) for c in E.OP_CASES],
    "dstd_dstdgc_train_saved_bytes": [lambda B, c=c: (_mode(c), B, c.cin, c.cout, c.T, c.V) for c in E.OP_CASES],
    "dstd_dstdgc_train_workspace_bytes": [lambda B, c=c: (_mode(c), B, c.cin, c.cout, c.T, c.V) for c in E.OP_CASES],
    "dstd_dstdgc_train_saved_bytes_r": [lambda B, c=c, r=r: (_mode(c), B, c.cin, c.cout, c.T, c.V, r)
                                        for c in E.OP_CASES for r in sorted({1, 2, 8, c.red})],
    "dstd_dstdgc_train_workspace_bytes_r": [lambda B, c=c, r=r: (_mode(c), B, c.cin, c.cout, c.T, c.V, r)
                                            for c in E.OP_CASES for r in sorted({1, 2, 8, c.red})],
    "dstd_block_workspace_bytes": [lambda B, s=s: (B, *s) for s in _blocks()],
    "dstd_block_taps_workspace_bytes": [lambda B, s=s: (B, *s) for s in _blocks()],
    "dstd_block_train_saved_bytes": [lambda B, s=s: (B, *s) for s in _blocks()],
    "dstd_block_train_workspace_bytes": [lambda B, s=s: (B, *s) for s in _blocks()],
    "dstd_model_workspace_bytes": [lambda B, s=s: (B, *s) for s in _models()],
    "dstd_model_taps_workspace_bytes": [lambda B, s=s: (B, *s) for s in _models()],
    "dstd_model_train_saved_bytes": [lambda B, s=s: (B, *s) for s in _models()],
    "dstd_model_train_workspace_bytes": [lambda B, s=s: (B, *s) for s in _models()],
    "dstd_loss_workspace_bytes": [lambda B: ()],
    "dstd_losses_workspace_bytes": [lambda B: ()],
    "dstd_ctg_workspace_bytes": [lambda B, s=s: (B, *s[1:]) for s in G.CTG_SHAPES],
    "dstd_conv2d_workspace_bytes": [lambda B, s=s: (B, *s[1:]) for s in G.CONV_SHAPES],
}


def test_every_size_export_of_the_headers_is_covered():
    exports = _size_exports()
    assert len(exports) == 17, sorted(exports)
    assert set(exports) == set(ARGS)
    assert {n for n, _ in G.PINNED_SIZES} == set(ARGS)
    assert set(exports.values()) == {"dstd_gcn.h", "dstd_gcn_train.h", "dstd_gcn_loss.h", "dstd_gcn_aux.h",
                                     "dstd_gcn_taps.h"}


@pytest.mark.parametrize("name", sorted(ARGS))
def test_sizes_positive_and_non_decreasing_in_B(name):
    fn = getattr(native.lib(), name)
    for args in ARGS[name]:
        sizes = [int(fn(*args(B))) for B in (1, 2, 3, 4)]
        assert sizes[0] > 0, (name, args(1))
        assert sizes == sorted(sizes), (name, args(1), sizes)
        # every carved region starts on a multiple of 256 and 256 bytes of slack follow the last
        # one: nothing smaller than the slack can be a size
        assert sizes[0] >= 256, (name, args(1), sizes)


def test_taps_sizes_equal_the_plain_ones():
    L = native.lib()
    for B in (1, 2, 3):
        for s in _blocks():
            assert L.dstd_block_taps_workspace_bytes(B, *s) == L.dstd_block_workspace_bytes(B, *s), (B, s)
        for s in _models():
            assert L.dstd_model_taps_workspace_bytes(B, *s) == L.dstd_model_workspace_bytes(B, *s), (B, s)


def test_red_2_sizes_are_the_plain_ones():
    L = native.lib()
    for c in E.OP_CASES:
        a = (_mode(c), c.B, c.cin, c.cout, c.T, c.V)
        assert L.dstd_dstdgc_train_saved_bytes_r(*a, 2) == L.dstd_dstdgc_train_saved_bytes(*a)
        assert L.dstd_dstdgc_train_workspace_bytes_r(*a, 2) == L.dstd_dstdgc_train_workspace_bytes(*a)


def test_sizes_are_the_pinned_layout():
    """guard_helper.PINNED_SIZES: a size export that shrinks (a region missing
    from the measuring walk, the slack after the last region dropped) fails
    here, on the host, whether or not a kernel reaches the missing bytes."""
    G.check_pinned_sizes()
