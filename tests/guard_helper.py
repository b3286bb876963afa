"""Exact-size, guard-banded, poisoned buffers for the memory-contract tests
(tests/test_guard_host.py, tests/test_gpu_guards.py).

The C ABI promises (include/dstd_gcn.h "Conventions", dstd_gcn_train.h,
dstd_gcn_loss.h): scratch comes from a caller-owned workspace of
``*_workspace_bytes`` bytes, the library allocates nothing and keeps no state,
a train forward's ``saved`` buffer is all its backward needs, and a refused
call writes nothing.  There is no memset in the native sources, so a call that
reads a byte of its workspace before writing it reads what the caller left
there.

``Guarded`` is one allocation GUARD | inner | GUARD: the inner region has the
exact size asked for and a chosen byte fill, the guards hold a sentinel word
and are compared as integers afterwards.  ``guarded_workspaces`` puts every
``dstd_native.workspace`` / ``workspace_claim`` caller -- modules, autograd
functions, taps, the aux layers, the losses, the engine -- on such buffers.
"""
import contextlib

import torch

import dstd_native as native

# A condition, not a measurement: larger than any single carved region of the cases of
# tests/test_gpu_guards.py, so that an overrun of one region lands in memory the test owns and is
# reported instead of faulting.
GUARD = 1 << 20
ALIGN = 256
# fp32 NaN with a payload, read as int32; its bytes (EF BE C0 7F) are none of the fills
SENTINEL = 0x7FC0BEEF
# Byte patterns for scratch:
#   0x00  zeros
#   0xFF  NaN as fp32 and as f16, -1 as an integer
#   0x4B  finite and large: 0x4B4B4B4B = 1.33e7 as fp32, 0x4B4B = 14.6 as f16 -- survives max,
#         comparisons and selects where a NaN is dropped, and perturbs a max-|x| range scale
FILLS = (0x00, 0xFF, 0x4B)


def rup(n, m):
    return (n + m - 1) // m * m


class GuardError(AssertionError):
    pass


class Guarded:
    """``nbytes`` bytes filled with the byte ``fill`` between two GUARD-byte
    bands of SENTINEL words.  ``tensor``: the inner uint8 view, numel() ==
    nbytes, 256-byte aligned; ``check(what)`` raises GuardError naming the side
    and the first / last touched byte offset relative to the inner region."""

    def __init__(self, nbytes, fill=0x00, device="cpu"):
        nbytes = int(nbytes)
        assert nbytes >= 0 and 0 <= fill <= 0xFF
        self.nbytes, self.fill = nbytes, fill
        self.inner = rup(nbytes, ALIGN)
        total = GUARD + self.inner + GUARD
        raw = torch.empty(total + ALIGN, dtype=torch.uint8, device=device)
        skew = -raw.data_ptr() % ALIGN  # torch's allocators give 256+ already; make it a fact
        self.raw = raw[skew:skew + total]
        self.raw.view(torch.int32).fill_(_as_int32(SENTINEL))
        self.tensor = self.raw[GUARD:GUARD + nbytes]
        self.tensor.fill_(fill)
        assert self.tensor.numel() == nbytes and self.ptr % ALIGN == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def view(self, dtype, shape):
        """The first prod(shape) elements of the inner region as ``dtype``."""
        n = 1
        for s in shape:
            n *= int(s)
        item = torch.empty((), dtype=dtype).element_size()
        assert n * item <= self.nbytes, (n * item, self.nbytes)
        return self.tensor[:n * item].view(dtype).view(*shape)

    def _band(self, lo, hi):
        """Byte offsets (relative to the start of raw[lo:hi]) that differ from the sentinel."""
        words = self.raw[lo:hi].view(torch.int32)
        bad = (words != _as_int32(SENTINEL)).nonzero().flatten()
        if bad.numel() == 0:
            return None
        by = self.raw[lo:hi]
        want = torch.tensor(list(SENTINEL.to_bytes(4, "little")), dtype=torch.uint8, device=by.device)
        first_w, last_w = int(bad[0]), int(bad[-1])
        f = by[4 * first_w:4 * first_w + 4] != want
        l = by[4 * last_w:4 * last_w + 4] != want
        first = 4 * first_w + int(f.nonzero()[0])
        last = 4 * last_w + int(l.nonzero()[-1])
        return first, last

    def damage(self):
        """{"before": (first, last), "after": (first, last)} of touched guard
        bytes, offsets relative to the inner region's first byte (negative:
        before it; >= nbytes: past it).  Empty when both guards are intact.
        The pad from nbytes up to the next multiple of 256 counts as "after"."""
        out = {}
        b = self._band(0, GUARD)
        if b is not None:
            out["before"] = (b[0] - GUARD, b[1] - GUARD)
        a = self._band(GUARD + self.inner, GUARD + self.inner + GUARD)
        if a is not None:
            out["after"] = (self.inner + a[0], self.inner + a[1])
        if self.inner > self.nbytes:  # exact-size: bytes nbytes .. rup(nbytes, 256) are outside too
            pad = self.raw[GUARD + self.nbytes:GUARD + self.inner]
            want = torch.tensor(list(SENTINEL.to_bytes(4, "little")), dtype=torch.uint8, device=pad.device)
            idx = torch.arange(self.nbytes, self.inner, device=pad.device)
            bad = (pad != want[idx % 4]).nonzero().flatten()  # GUARD and the inner start are multiples of 4
            if bad.numel():
                first, last = self.nbytes + int(bad[0]), self.nbytes + int(bad[-1])
                if "after" in out:
                    last = out["after"][1]
                out["after"] = (first, last)
        return out

    def check(self, what="buffer"):
        d = self.damage()
        if d:
            msg = "; ".join(f"{side} the buffer, bytes {lo}..{hi} relative to its start" for side, (lo, hi) in d.items())
            raise GuardError(f"{what} ({self.nbytes} bytes): guard overwritten {msg}")


def _as_int32(word):
    return word - (1 << 32) if word >= 1 << 31 else word


class _Recorder:
    def __init__(self, fill, device_override=None):
        self.fill, self.device_override, self.handed = fill, device_override, []

    def claim(self, device, nbytes, tag):
        g = Guarded(nbytes, self.fill, self.device_override or device)
        self.handed.append(g)
        return g.tensor, False

    def workspace(self, device, nbytes):
        return self.claim(device, nbytes, None)[0]

    def check(self):
        for i, g in enumerate(self.handed):
            g.check(f"workspace {i} of {len(self.handed)}")


@contextlib.contextmanager
def guarded_workspaces(fill, device=None):
    """For the duration: ``dstd_native.workspace`` and ``workspace_claim`` hand
    out a fresh Guarded(nbytes, fill).tensor of exactly the requested size
    (``reused`` always False).  Yields the recorder (``.handed``: every
    Guarded handed out).  On a clean exit it synchronises and checks every
    guard; the originals are restored either way.  ``device`` overrides where
    the buffers live (host tests)."""
    rec = _Recorder(fill, device)
    saved = native.workspace, native.workspace_claim
    native.workspace, native.workspace_claim = rec.workspace, rec.claim
    try:
        yield rec
    finally:
        native.workspace, native.workspace_claim = saved
    if torch.cuda.is_available() and any(g.raw.is_cuda for g in rec.handed):
        torch.cuda.synchronize()
    rec.check()


# ---- shapes shared by the host and the GPU test ---------------------------------
# the layouts with split-f16 eval kernels (include/dstd_gcn.h DSTD_FWD_EXACT_FP32) and their skeletons
SPLIT_TV = ((35, 22), (35, 25), (40, 23), (75, 22))
LAYOUT_OF_V = {22: "h36m", 25: "cmu", 23: "3dpw"}
SPLIT_CHANNELS = ((64, 64), (6, 64), (64, 3))  # the model's three kinds of block
SPLIT_B = (1, 3)
MODEL_LAYERS = (2, 9)  # 9: the encoder run spans two chain launches (8 blocks, then 1)
# tests/test_gpu_train.py PLAIN / test_native_conv2d_strided_padded: (B, C, T, V) of the ConvTemporalGraphical,
# (B, cin, cout, H, W, kh, kw, sh, sw, ph, pw) of the Conv2d
CTG_SHAPES = ((2, 64, 35, 22), (2, 16, 20, 22), (2, 8, 10, 22))
CONV_SHAPES = ((2, 64, 32, 35, 22, 3, 1, 1, 1, 1, 0), (2, 16, 16, 20, 22, 3, 3, 1, 1, 1, 1),
               (2, 8, 12, 10, 22, 1, 1, 1, 1, 0, 0), (2, 5, 7, 11, 9, 3, 5, 2, 1, 1, 2))

# What the size exports return at one shape each.  Every call checks its buffer against the very
# function that sized it, so a *_workspace_bytes / *_saved_bytes that came out too small (a region
# dropped from the measuring walk, the 256-byte slack after the last region gone) would shrink the
# caller's buffer and the call's check together, and only a kernel that happens to reach the missing
# bytes would show it.  These numbers are the layout the guarded GPU runs of tests/test_gpu_guards.py
# were made on: a change of a carve changes them, and whoever changes it re-runs those tests on the
# new layout and updates the table.
PINNED_SIZES = {
    ("dstd_dstdgc_workspace_bytes", (0, 2, 24, 40, 20, 17)): 232064,
    ("dstd_dstdgc_workspace_bytes", (1, 2, 20, 24, 49, 5)): 190880,
    ("dstd_block_workspace_bytes", (3, 64, 64, 35, 22)): 2830432,
    ("dstd_block_workspace_bytes", (2, 6, 64, 17, 25)): 950048,
    ("dstd_block_taps_workspace_bytes", (3, 64, 64, 35, 22)): 2830432,
    ("dstd_model_workspace_bytes", (3, 35, 22, 64, 2)): 3261792,
    ("dstd_model_workspace_bytes", (1, 40, 23, 64, 9)): 2696832,
    ("dstd_model_taps_workspace_bytes", (3, 35, 22, 64, 2)): 3261792,
    ("dstd_dstdgc_train_saved_bytes", (0, 2, 24, 40, 20, 17)): 309920,
    ("dstd_dstdgc_train_workspace_bytes", (0, 2, 24, 40, 20, 17)): 4118016,
    ("dstd_dstdgc_train_saved_bytes_r", (1, 2, 20, 64, 35, 22, 8)): 2656304,
    ("dstd_dstdgc_train_workspace_bytes_r", (1, 2, 20, 64, 35, 22, 8)): 16658432,
    ("dstd_block_train_saved_bytes", (2, 6, 64, 17, 25)): 2833664,
    ("dstd_block_train_workspace_bytes", (2, 6, 64, 17, 25)): 15944960,
    ("dstd_model_train_saved_bytes", (2, 35, 22, 64, 2)): 20740352,
    ("dstd_model_train_workspace_bytes", (2, 35, 22, 64, 2)): 19727712,
    ("dstd_loss_workspace_bytes", ()): 768,
    ("dstd_losses_workspace_bytes", ()): 3328,
    ("dstd_ctg_workspace_bytes", (2, 16, 20, 22)): 608512,
    ("dstd_conv2d_workspace_bytes", (2, 5, 7, 11, 9, 3, 5, 2, 1, 1, 2)): 38144,
}


def check_pinned_sizes(names=None):
    """The host-side size comparison: every pinned export (or those in
    ``names``) returns its pinned size."""
    L = native.lib()
    for (name, args), want in PINNED_SIZES.items():
        if names is None or name in names:
            got = int(getattr(L, name)(*args))
            assert got == want, f"{name}{args} = {got}, pinned {want} ({got - want:+d} bytes)"
