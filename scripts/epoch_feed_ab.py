"""What feeding costs: one PredictionEngine.train epoch of 128 steps, fed three ways.

3DPW shape (T = 40, D = 72, V = 23), B = 32, 4096 synthetic windows, the shipped
5-layer model, the shipped loss (one jl2 line) with the inverse pass:

  host_w0    the reference's way: a Dataset of four float64 numpy arrays
             (dataset/pw3d.py:133-139) behind DataLoader(shuffle=True,
             pin_memory=True), num_workers=0; the engine casts and copies
             three tensors per step (engine/prediction.py _to_dev)
  host_w4    the same with num_workers=4 (spawn context, persistent workers,
             so that their start-up is paid in the warm-up round only)
  device     dstd_data.DeviceLoader(shuffle=True): the set resident on the
             GPU, one dstd_batch_gather launch per batch

Each leg has its own engine and model (same seed).  Wall time per epoch is
taken around engine.train, which synchronises once when it reports its
averages, plus one device synchronise for the last step's tail.  After one
warm-up round the legs run interleaved over --rounds rounds in this one
process; the figures are per-step medians over the rounds, and ratios of those.

  python scripts/epoch_feed_ab.py [--rounds 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dstd-gcn_amd")):
    sys.path.insert(0, p)

T, D, INPUT_N, OUTPUT_N = 40, 72, 10, 30


class HostWindows(Dataset):
    """Four float64 arrays and a 4-tuple per item, as the reference's datasets."""

    def __init__(self, all_seqs, dim_used, frame_in, frame_inv):
        used = all_seqs[:, :, dim_used]
        self.all_seqs = all_seqs
        self.input_seqs = used[:, frame_in].copy()
        self.input_seqs_inv = used[:, frame_inv].copy()
        self.output_seqs = used.copy()

    def __len__(self):
        return len(self.all_seqs)

    def __getitem__(self, item):
        return self.input_seqs[item], self.input_seqs_inv[item], self.output_seqs[item], self.all_seqs[item]


class _Log:
    def info(self, *a, **k):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    from dstd_data import DeviceLoader, DeviceSequences, frame_maps
    from engine import PredictionEngine
    from model import get_model

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    windows = np.cumsum(rng.normal(0, 10, (a.windows, T, D)), 1)
    windows[:, :, :3] = 0
    dim_used = np.arange(3, D)
    frame_in, frame_inv = frame_maps(INPUT_N, OUTPUT_N, True)
    host = HostWindows(windows, dim_used, frame_in, frame_inv)
    seqs = DeviceSequences.from_windows(windows, dim_used, INPUT_N, OUTPUT_N, padding=True, device=dev)

    loaders = {
        "host_w0": DataLoader(host, batch_size=a.batch, shuffle=True, pin_memory=True, num_workers=0),
        "host_w4": DataLoader(host, batch_size=a.batch, shuffle=True, pin_memory=True, num_workers=4,
                              multiprocessing_context="spawn", persistent_workers=True),
        "device": DeviceLoader(seqs, a.batch, shuffle=True),
    }
    opts = dict(input_channels=6, input_time_frame=INPUT_N, output_time_frame=OUTPUT_N, st_gcnn_dropout=0.0,
                joints_to_consider=23, num_feature=64, num_layers=5, layout="3dpw")
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=1000), loss=dict(joint=["jl2", 1]),
               n_out=1, transform="tsc", use_weight=False, inverse=True)
    engines = {}
    for leg in loaders:
        torch.manual_seed(0)
        engines[leg] = PredictionEngine(cfg, get_model("dstdgcn", dstdgcn=opts).to(dev).train(), _Log())
    steps = len(loaders["device"])
    assert all(len(ld) == steps for ld in loaders.values())

    def epoch(leg, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = engines[leg].train(loaders[leg], n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, loss

    for leg in loaders:  # warm-up round: kernels loaded, workers started, allocator settled
        epoch(leg, 0)
    per_step = {leg: [] for leg in loaders}
    last_loss = {}
    for r in range(a.rounds):
        for leg in loaders:
            ms, last_loss[leg] = epoch(leg, r + 1)
            per_step[leg].append(round(ms, 4))
            print(f"round {r} {leg}: {ms:.3f} ms/step", flush=True)
    med = {leg: statistics.median(v) for leg, v in per_step.items()}
    result = {
        "metric": "train_epoch_ms_per_step", "unit": "ms/step", "steps_per_epoch": steps, "batch": a.batch,
        "windows": a.windows, "rounds": a.rounds,
        "config": {"workload": "3dpw T=40 D=72 V=23, engine.train epoch, jl2 + inverse pass, Adam",
                   "timing": "wall per epoch incl. the engine's one synchronisation, legs interleaved in one process"},
        "per_round_ms_per_step": per_step,
        "median_ms_per_step": {leg: round(v, 4) for leg, v in med.items()},
        "min_ms_per_step": {leg: min(v) for leg, v in per_step.items()},
        "ratio_host_w0_over_device": round(med["host_w0"] / med["device"], 4),
        "ratio_host_w4_over_device": round(med["host_w4"] / med["device"], 4),
        "ratio_host_w4_over_host_w0": round(med["host_w4"] / med["host_w0"], 4),
        "device_set_nbytes": seqs.nbytes,
        "last_epoch_loss": {leg: round(float(v), 4) for leg, v in last_loss.items()},
        "device_name": torch.cuda.get_device_name(0),
    }
    line = json.dumps(result)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    del loaders["host_w4"]  # joins the workers


if __name__ == "__main__":
    main()
