"""What resampling a resident batch in time costs, inside the gather.

Two synthetic training sets with the shapes of the real ones -- H36M (T = 35,
D = 96, 66 used columns, mirrored) and 3DPW (T = 40, D = 72, 69 used columns,
mirrored), dim_used from tests/golden/dataset_batches.npz -- built by
DeviceSequences.from_sequences from whole sequences, so that windows have room
after their last frame, at batch 32 and 256, in one process.  Per batch: a
rotation about axis 1 with scale and shift, input noise of amplitude 2
(scripts/augment_ab.py's) and a playback rate uniform in [0.8, 1.25] capped by
fit_rate; all drawn once per shape, outside the timed region.

  plain    DeviceSequences.gather(idx): one dstd_batch_gather launch
  fused    gather(idx, transform=, noise=, noise_seed=): one
           dstd_batch_gather_aug launch -- the yardstick: unchanged code
  warped   gather(idx, transform=, noise=, noise_seed=, rate=): one
           dstd_batch_gather_warp launch with the same transform and noise

Before timing, `warped` at all-ones rates is checked bit-equal to `fused`.
Every shape is warmed, then the legs alternate over --rounds rounds; a leg's
figure is the wall time of --iters calls in a row, started after a device
synchronise and stopped after the next, per call.  That is throughput of the
enqueue-and-execute pipeline, which is what a host-bound training step sees;
it is not the kernels' own time.

--iters defaults to 3000, ten times scripts/augment_ab.py's: at about 18 us per
call a timed window is then some 55 ms and not 5.

  python scripts/warp_ab.py [--rounds 10] [--iters 3000] [--out FILE.json]
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
SEQUENCES, FRAMES = 8, 300  # 8 * (300 - T + 1) windows, about the 2048 of scripts/augment_ab.py
AMP = 2.0
SPEED = (0.8, 1.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds: at least 10")

    from dstd_data import Augment, DeviceSequences

    dev = torch.device("cuda", 0)
    fixture = np.load(os.path.join(ROOT, "tests", "golden", "dataset_batches.npz"), allow_pickle=False)
    aug = Augment(rotate=(1, 3.14159), scale=(0.9, 1.1), shift=50.0, noise=AMP, speed=SPEED)
    rng = np.random.default_rng(0)
    shapes = {}
    for name, cfg in SETS.items():
        dim_used = fixture[cfg["case"] + "/dim_used"]
        sequences = [np.cumsum(rng.normal(0, 10, (FRAMES, cfg["D"])), 0) for _ in range(SEQUENCES)]
        seqs = DeviceSequences.from_sequences(sequences, cfg["T"], dim_used, cfg["input_n"], cfg["T"] - cfg["input_n"],
                                              device=dev, mirror=(cfg["left"], cfg["right"]))
        for B in (32, 256):
            g = torch.Generator(device=dev)
            g.manual_seed(B)
            idx = torch.randperm(len(seqs), generator=g, device=dev)[:B].contiguous()
            xf = aug.draw(B, g, dev)
            rate = seqs.fit_rate(idx, aug.draw_speed(B, g, dev)).contiguous()
            shapes[f"{name} B={B}"] = (seqs, idx, xf, rate)

    seed = 12345
    results = {}
    for what, (seqs, idx, xf, rate) in shapes.items():
        legs = {
            "plain": lambda: seqs.gather(idx),
            "fused": lambda: seqs.gather(idx, transform=xf, noise=AMP, noise_seed=seed),
            "warped": lambda: seqs.gather(idx, transform=xf, noise=AMP, noise_seed=seed, rate=rate),
        }
        # outputs first: unit rates are the fused gather, bit for bit; the drawn rates are not
        fused = legs["fused"]()
        unit = seqs.gather(idx, transform=xf, noise=AMP, noise_seed=seed, rate=torch.ones_like(rate))
        if not all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(fused, unit)):
            raise SystemExit(f"{what}: the warped gather at unit rates and the fused gather differ")
        warped = legs["warped"]()
        if torch.equal(warped[3], fused[3]) or not bool(torch.isfinite(warped[3]).all()):
            raise SystemExit(f"{what}: the warped gather did not warp")
        blended = float((rate * (seqs.seq_len - 1) != (rate * (seqs.seq_len - 1)).floor()).float().mean())

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
            "warped_minus_fused_us": round(med["warped"] - med["fused"], 3),
            "warped_over_fused": round(med["warped"] / med["fused"], 3),
            "ranges_overlap": {"plain_fused": max(us["plain"]) >= min(us["fused"]),
                               "fused_warped": max(us["fused"]) >= min(us["warped"])},
            "rate_range": [round(float(rate.min()), 4), round(float(rate.max()), 4)],
            "share_of_rows_with_a_blended_last_frame": round(blended, 3),
            "unit_rates_bit_equal_to_fused": True,
        }
        print(what, json.dumps(results[what]["median_us"]), json.dumps(results[what]["range_us"]), flush=True)

    result = {
        "metric": "warped_batch_us", "unit": "us/call", "rounds": a.rounds, "iters_per_round": a.iters,
        "sequences": SEQUENCES, "frames_per_sequence": FRAMES, "noise_amplitude": AMP, "speed": list(SPEED),
        "config": {"timing": "wall of iters calls in a row between two device synchronises, per call; legs alternate "
                             "within each round, one process; not the kernels' own time",
                   "yardstick": "fused: dstd_batch_gather_aug, code this change does not touch"},
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
