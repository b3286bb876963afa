#!/usr/bin/env python
"""A/B of the rollout: the Python window loop against DSTDGCN.predict.

  python scripts/predict_ab.py [--rounds 10 --calls 20 --config h36m --json OUT]
The loop is what a caller of ``model(x)`` writes (pad the observed frames, run
the model, slice, concatenate, re-pad: torch indexing between the forwards);
``predict`` is the same windows in one native call
(include/dstd_gcn_predict.h).  Each round times ``--calls`` calls of one, then
of the other (wall clock around work that ends in a device synchronise),
rounds interleave the two, and both are warmed at every shape first.  The
outputs are compared bit for bit before anything is timed.  Cases: B = 256 with
H = 25 and H = 100, B = 32 with H = 100.  --json writes every round.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dstd-gcn_amd"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CASES = ((256, 25), (256, 100), (32, 100))


def window_loop(model, obs, horizon):
    """The rollout contract with ``model(x)`` and torch indexing."""
    Tin, Tout = model.input_time_frame, model.output_time_frame
    T = Tin + Tout
    m = torch.tensor([min(s, Tin - 1) for s in range(T)], device=obs.device)
    x = obs[:, m]
    outs, have = [], 0
    while have < horizon:
        y = model(x)
        take = min(Tout, horizon - have)
        outs.append(y[:, Tin:Tin + take])
        have += take
        x = torch.cat([x[:, :Tin], y[:, Tin:]], 1)[:, T - Tin + m]
    return torch.cat(outs, 1)


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--config", default="h36m")
    ap.add_argument("--json", default=None, help="write every round's ms per call here")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model, opts, _ = bench.load_model(a.config, dev)
    Tin, V = opts["input_time_frame"], opts["joints_to_consider"]
    res = {}
    with torch.no_grad():
        for B, H in CASES:
            obs = torch.randn(B, Tin, V, 3, generator=torch.Generator().manual_seed(B + H)).to(dev)
            fns = {"loop": lambda: window_loop(model, obs, H), "predict": lambda: model.predict(obs, H)}
            for _ in range(3):
                outs = {k: f() for k, f in fns.items()}
            torch.cuda.synchronize()
            if not torch.equal(outs["loop"], outs["predict"]):
                raise SystemExit(f"B={B} H={H}: predict differs from the window loop")
            r = res[f"B{B}_H{H}"] = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, f in fns.items():
                    r[k].append(timed(f, a.calls))
            med = {k: float(np.median(v)) for k, v in r.items()}
            print(f"B={B} H={H}: " + ", ".join(f"{k} median {med[k]:.4f} ms (min {min(r[k]):.4f}, max {max(r[k]):.4f})"
                                               for k in fns) + f", loop / predict {med['loop'] / med['predict']:.3f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"config": a.config, "rounds": a.rounds, "calls": a.calls, "ms_per_call": res}, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
