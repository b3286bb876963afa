"""What augmenting a resident batch costs: in the gather, or in torch after it.

Two synthetic training sets with the shapes of the real ones -- H36M (T = 35,
D = 96, 66 used columns, mirrored) and 3DPW (T = 40, D = 72, 69 used columns,
mirrored), dim_used from tests/golden/dataset_batches.npz -- at batch 32 and
256, in one process.  Per batch: a rotation about axis 1 with scale and shift
(dstd_data.Augment.draw, drawn once per shape, outside the timed region) and
input noise of amplitude 2.

  plain      DeviceSequences.gather(idx): one dstd_batch_gather launch
  fused      gather(idx, transform=, noise=, noise_seed=): one
             dstd_batch_gather_aug launch
  torch      the plain gather, then include/ext/dstd_gcn_augment.h restated with
             torch ops on all four tensors (tests/augment_helper.py moved to
             torch: fp32 products and sums in the header's order, the hash in
             int64 arithmetic).  Bit-equal to `fused`, checked before timing.
  torch_bmm  the plain gather, then what a user would write without caring for
             bits: baddbmm on each of the four tensors, one torch.rand for the
             noise, indexed through the frame maps so that padded rows stay
             copies.  Equal to `fused` without noise within fp32 rounding
             (checked before timing); its noise is another stream.

Every shape is warmed, then the legs alternate over --rounds rounds; a leg's
figure is the wall time of --iters calls in a row, started after a device
synchronise and stopped after the next, per call.  That is throughput of the
enqueue-and-execute pipeline, which is what a host-bound training step sees.
The op counts are aten operators dispatched per call (views excluded), counted
by a TorchDispatchMode outside the timed region: each is at least one launch;
they are not a kernel trace.

  python scripts/augment_ab.py [--rounds 10] [--iters 300] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dstd-gcn_amd")):
    sys.path.insert(0, p)

SETS = {"h36m": dict(case="h36m_pad", T=35, input_n=10, D=96, left=[1, 2, 3, 4, 5, 17, 18, 19, 20, 21, 22, 23],
                     right=[6, 7, 8, 9, 10, 25, 26, 27, 28, 29, 30, 31]),
        "3dpw": dict(case="pw3d_pad_mirror", T=40, input_n=10, D=72, left=[1, 4, 7, 10, 13, 16, 18, 20, 22],
                     right=[2, 5, 8, 11, 14, 17, 19, 21, 23])}
WINDOWS = 2048
AMP = 2.0
_M64 = (1 << 64) - 1


def _i64(v):
    """A Python int modulo 2^64 as the int64 with the same bits."""
    v &= _M64
    return v - (1 << 64) if v >> 63 else v


def _lsr(z, k):
    """Logical right shift of an int64 tensor (torch's >> is arithmetic)."""
    return (z >> k) & ((1 << (64 - k)) - 1)


def torch_jitter(seed, index, T, frames, Du, amp):
    """amp * (2u - 1) per (batch row, source frame, used column): fp32 [B][len(frames)][Du].
    int64 multiplication and addition wrap modulo 2^64 as the header's uint64 do."""
    dev = index.device
    key = ((index[:, None] * T + frames[None, :].long())[:, :, None] * Du
           + torch.arange(Du, device=dev, dtype=torch.int64)[None, None, :])
    z = key + _i64(seed * 0x9E3779B97F4A7C15)
    z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
    z = z ^ _lsr(z, 31)
    u = _lsr(z, 40).float() * (2.0 ** -24)
    return amp * (2 * u - 1)


def torch_restatement(seqs, batch, index, xf, amp, seed):
    """include/ext/dstd_gcn_augment.h on the four tensors of a plain gather."""
    inputs, inputs_inv, targets, all_seqs = batch
    B, T, D = all_seqs.shape
    m = xf.view(B, 3, 4)[:, None, None]  # [B, 1, 1, 3, 4]
    p = all_seqs.view(B, T, D // 3, 3)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    q = torch.stack([((m[..., c, 0] * x + m[..., c, 1] * y) + m[..., c, 2] * z) + m[..., c, 3]
                     for c in range(3)], -1)
    all_seqs = q.view(B, T, D)
    targets = all_seqs[:, :, seqs._dim_used.long()]
    Du = targets.shape[2]
    inputs = targets[:, seqs._frame_in.long()] + torch_jitter(seed, index, T, seqs._frame_in, Du, amp)
    inputs_inv = targets[:, seqs._frame_inv.long()] + torch_jitter(seed, index, T, seqs._frame_inv, Du, amp)
    return inputs, inputs_inv, targets, all_seqs


def torch_bmm(seqs, batch, xf, amp, generator):
    """The idiomatic version (dim_used takes whole joints in both sets)."""
    B = xf.shape[0]
    m = xf.view(B, 3, 4)
    At, t = m[:, :, :3].transpose(1, 2), m[:, None, :, 3]
    out = [torch.baddbmm(t, x.view(B, -1, 3), At).view(x.shape) for x in batch]
    if amp:
        n = (2 * torch.rand(out[2].shape, generator=generator, device=xf.device) - 1) * amp
        out[0] = out[0] + n[:, seqs._frame_in.long()]
        out[1] = out[1] + n[:, seqs._frame_inv.long()]
    return tuple(out)


class _CountOps(torch.utils._python_dispatch.TorchDispatchMode):
    VIEWS = ("view", "select", "slice", "unsqueeze", "expand", "transpose", "alias", "detach", "_unsafe_view", "t",
             "permute", "as_strided", "squeeze", "reshape")

    def __init__(self):
        super().__init__()
        self.ops = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func.overloadpacket.__name__
        if name not in self.VIEWS:
            self.ops.append(name)
        return func(*args, **(kwargs or {}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds: at least 10")

    from dstd_data import Augment, DeviceSequences

    dev = torch.device("cuda", 0)
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "dataset_batches.npz"), allow_pickle=False)
    aug = Augment(rotate=(1, 3.14159), scale=(0.9, 1.1), shift=50.0, noise=AMP)
    rng = np.random.default_rng(0)
    shapes = {}
    for name, cfg in SETS.items():
        dim_used = fixture[cfg["case"] + "/dim_used"]
        # whole joints, which the bmm version relies on
        assert np.array_equal(dim_used.reshape(-1, 3) % 3, np.tile(np.arange(3), (len(dim_used) // 3, 1)))
        windows = np.cumsum(rng.normal(0, 10, (WINDOWS, cfg["T"], cfg["D"])), 1)
        seqs = DeviceSequences.from_windows(windows, dim_used, cfg["input_n"], cfg["T"] - cfg["input_n"], device=dev,
                                            mirror=(cfg["left"], cfg["right"]))
        for B in (32, 256):
            g = torch.Generator(device=dev)
            g.manual_seed(B)
            idx = torch.randperm(len(seqs), generator=g, device=dev)[:B].contiguous()
            shapes[f"{name} B={B}"] = (seqs, idx, aug.draw(B, g, dev), g)

    seed = 12345
    results = {}
    for what, (seqs, idx, xf, g) in shapes.items():
        legs = {
            "plain": lambda: seqs.gather(idx),
            "fused": lambda: seqs.gather(idx, transform=xf, noise=AMP, noise_seed=seed),
            "torch": lambda: torch_restatement(seqs, seqs.gather(idx), idx, xf, AMP, seed),
            "torch_bmm": lambda: torch_bmm(seqs, seqs.gather(idx), xf, AMP, g),
        }
        # outputs first
        fused, restated = legs["fused"](), legs["torch"]()
        bit_equal = all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(fused, restated))
        if not bit_equal:
            raise SystemExit(f"{what}: the torch restatement and the fused gather differ")
        clean_fused = seqs.gather(idx, transform=xf)
        clean_bmm = torch_bmm(seqs, seqs.gather(idx), xf, 0.0, g)
        bmm_diff = max(float((u - v).abs().max() / u.abs().max()) for u, v in zip(clean_fused, clean_bmm))
        if bmm_diff > 1e-5:
            raise SystemExit(f"{what}: the bmm version differs from the fused gather by {bmm_diff:.2e} of the range")
        ops = {}
        for leg, fn in legs.items():
            with _CountOps() as c:
                fn()
            ops[leg] = len(c.ops)

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / a.iters

        for fn in legs.values():  # warm this shape: code objects loaded, allocator settled
            timed(fn)
        us = {leg: [] for leg in legs}
        for r in range(a.rounds):
            for leg, fn in legs.items():
                us[leg].append(round(timed(fn), 3))
        med = {leg: statistics.median(v) for leg, v in us.items()}
        results[what] = {
            "per_round_us": us,
            "median_us": {k: round(v, 3) for k, v in med.items()},
            "range_us": {k: [min(v), max(v)] for k, v in us.items()},
            "fused_minus_plain_us": round(med["fused"] - med["plain"], 3),
            "torch_over_fused": round(med["torch"] / med["fused"], 3),
            "torch_bmm_over_fused": round(med["torch_bmm"] / med["fused"], 3),
            "ranges_overlap": {"plain_fused": max(us["plain"]) >= min(us["fused"]),
                               "fused_torch_bmm": max(us["fused"]) >= min(us["torch_bmm"]),
                               "fused_torch": max(us["fused"]) >= min(us["torch"])},
            "aten_ops_per_call": ops,
            "torch_restatement_bit_equal_to_fused": bit_equal,
            "bmm_max_difference_over_range_without_noise": bmm_diff,
        }
        print(what, json.dumps(results[what]["median_us"]), json.dumps(results[what]["range_us"]), ops, flush=True)

    result = {
        "metric": "augmented_batch_us", "unit": "us/call", "rounds": a.rounds, "iters_per_round": a.iters,
        "windows": WINDOWS, "noise_amplitude": AMP,
        "config": {"timing": "wall of iters calls in a row between two device synchronises, per call; legs alternate "
                             "within each round, one process",
                   "aten_ops_per_call": "aten operators dispatched per call, views excluded (TorchDispatchMode); "
                                        "arithmetic on the code, not a kernel trace; plain and fused count the "
                                        "allocation of the four outputs, their one native launch is not an aten op"},
        "shapes": results,
        "device_name": torch.cuda.get_device_name(0),
    }
    line = json.dumps(result)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
