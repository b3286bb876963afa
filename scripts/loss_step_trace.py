"""The engine's training step (PredictionEngine.train, eager) on the config-5
workload -- 3DPW, T=40, V=23, 32 sequences, inverse pass -- under one of two
loss configurations, for a kernel trace and a step time:

  --loss jl2     the shipped configuration: one unweighted jl2 line
  --loss three   joint: [jl2, 1], transition: [tl2, 1], coordinate: [cl1, 1]
                 with joint weights (use_weight: True)

  rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- \
      python scripts/loss_step_trace.py --loss three --steps 20
  python scripts/trace_summary.py OUT/*/run_kernel_trace.csv 20 --marker k_prep_nctv --last 15

Prints one JSON line: ms per step (host wall clock over one train() call of
--steps steps, which synchronises once at its end) after --warmup steps.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dstd-gcn_amd")):
    sys.path.insert(0, p)

from engine import PredictionEngine  # noqa: E402
from model import get_model  # noqa: E402

LOSSES = {"jl2": dict(joint=["jl2", 1]),
          "three": dict(joint=["jl2", 1], transition=["tl2", 1], coordinate=["cl1", 1])}


class _Log:
    def info(self, *a, **k):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", choices=list(LOSSES), default="three")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    opts = dict(input_channels=6, input_time_frame=10, output_time_frame=30, st_gcnn_dropout=0.0,
                joints_to_consider=23, num_feature=64, num_layers=5, layout="3dpw")
    m = get_model("dstdgcn", dstdgcn=opts).to(dev)
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5), loss=LOSSES[a.loss], n_out=1,
               transform="tsc", use_weight=a.loss != "jl2", inverse=True)
    eng = PredictionEngine(cfg, m, _Log())
    g = torch.Generator().manual_seed(1234)
    seq = torch.randn(a.batch, 40, 69, generator=g)
    inp = seq.clone()
    inp[:, 10:] = inp[:, 9:10]
    inv = seq.flip(1).clone()
    inv[:, 10:] = inv[:, 9:10]
    batch = tuple(t.to(dev) for t in (inp, inv, seq, seq))  # already on the device: the step is what is timed
    w = None
    if a.loss != "jl2":
        w = np.random.default_rng(7).uniform(0.0, 1.0, 23)
        w = (w - w.min()) / (w.max() - w.min())  # min-max normalised, as the reference's datasets build them
    kw = {} if w is None else {"weights": w}
    eng.train([batch] * a.warmup, 0, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = eng.train([batch] * a.steps, 1, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
    print(json.dumps({"metric": "train_step_ms", "value": round(ms, 3), "unit": "ms/step", "loss_config": a.loss,
                      "weights": w is not None, "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
                      "loss": round(float(loss), 4)}), flush=True)


if __name__ == "__main__":
    main()
