#!/usr/bin/env python
"""A/B of training through a rollout: the hand-written window loop against
PredictionEngine.train(horizon=H).

  python scripts/rollout_train_ab.py [--rounds 10 --steps 20 --config h36m --json OUT]
Both legs are one optimizer step of the engine's configuration (inverse pass,
jl2 loss through weighted_losses, in-place gradient arena, fused Adam) on twin
models: ``loop`` rolls the windows out with ``model.forward_pair`` per window
and autograd glue between them (tests/rollout_helper.py rollout_loop_pair --
what can be written without DSTDGCN.rollout), ``chain`` is the engine's own
step over ``rollout_pair`` (include/ext/dstd_gcn_rollout.h).  Every step is
timed on its own, wall clock around one device synchronise; a round is
``--steps`` steps of one leg then of the other, both warmed first.  Before
anything is timed the two legs' gradients are compared bit for bit (dropout
off: each leg draws its own seeds); the timed steps run the shipped dropout.
Cases: B = 32 and 256, H = 25 and 100.  --json writes every step's time and the
saved bytes of each case (dstd_model_rollout_saved_bytes at the pair's 2 B).
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dstd-gcn_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import dstd_native as native  # noqa: E402
from engine import PredictionEngine  # noqa: E402
from engine.loss import weighted_losses  # noqa: E402
from rollout_helper import rollout_loop_pair  # noqa: E402

CASES = ((32, 25), (32, 100), (256, 25), (256, 100))
CFG = dict(learn=dict(opt="adam", lr=1e-4, weight_decay=0, gamma=0.9, step_size=5), loss=dict(joint=["jl2", 1]),
           n_out=1, transform="tsc", use_weight=False, inverse=True)


class _Log:
    def info(self, *a):
        pass


def loop_step(eng, inputs, inputs_inv, targets, H, step=True):
    net = eng.model.model
    n_in = net.input_time_frame
    obs = eng.transform(inputs)[:, :n_in].contiguous()
    obs_inv = eng.transform(inputs_inv)[:, :n_in].contiguous()
    preds = [eng.inverse(o) for o in rollout_loop_pair(net, obs, obs_inv, H)]
    out = weighted_losses(eng.model.loss_spec, preds, targets, [(n_in, 1), (H - 1, -1)], None)
    eng.optimizer.zero_grad()
    (out.sum() / 2).backward()
    if step:
        eng.optimizer.step()
    return out[0]


def timed_step(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--config", default="h36m")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model, opts, _ = bench.load_model(a.config, dev)
    n_in, n_out, V = opts["input_time_frame"], opts["output_time_frame"], opts["joints_to_consider"]
    L = native.lib()
    res = {}
    for B, H in CASES:
        nets = [copy.deepcopy(model).train() for _ in range(2)]
        engs = [PredictionEngine(CFG, m, _Log()) for m in nets]
        for m in nets:
            m._dstd_inplace_grads = True  # as PredictionEngine.train sets it for its steps
        seq = 0.5 * torch.randn(B, n_in + H, V * 3, generator=torch.Generator().manual_seed(B + H)).to(dev)
        inputs, inputs_inv = seq.clone(), seq.flip(1).contiguous()
        chain = lambda: engs[0]._step_rollout(inputs, inputs_inv, seq, H, None, None, False)  # noqa: E731
        loop = lambda: loop_step(engs[1], inputs, inputs_inv, seq, H)  # noqa: E731
        # gradients first, bit for bit, without dropout and without the update
        for m in nets:
            m.do_in.p = 0.0
        opt_step = engs[0].optimizer.step
        engs[0].optimizer.step = lambda: None
        la, lb = chain()[0], loop_step(engs[1], inputs, inputs_inv, seq, H, step=False)
        engs[0].optimizer.step = opt_step
        torch.cuda.synchronize()
        bad = [n for (n, p), q in zip(nets[0].named_parameters(), nets[1].parameters())
               if p.grad is not None and not torch.equal(p.grad, q.grad)]
        if bad or not torch.equal(la.reshape(-1), lb.detach().reshape(-1)):
            raise SystemExit(f"B={B} H={H}: the chain's loss or gradients differ from the loop's: {bad[:5]}")
        for m in nets:
            m.do_in.p = float(opts["st_gcnn_dropout"])
        fns = {"loop": loop, "chain": chain}
        for _ in range(3):
            for f in fns.values():
                f()
        r = {k: [] for k in fns}
        for i in range(a.rounds):
            for k, f in fns.items():
                r[k] += [timed_step(f) for _ in range(a.steps)]
            print(f"  B={B} H={H} round {i + 1}/{a.rounds}", flush=True)
        K = -(-H // n_out)
        saved = int(L.dstd_model_rollout_saved_bytes(2 * B, n_in + n_out, V, opts["num_feature"], opts["num_layers"], K))
        med = {k: float(np.median(v)) for k, v in r.items()}
        rng = {k: (float(min(v)), float(max(v))) for k, v in r.items()}
        p10_90 = {k: (float(np.percentile(v, 10)), float(np.percentile(v, 90))) for k, v in r.items()}
        res[f"B{B}_H{H}"] = dict(windows=K, saved_bytes=saved, median_ms=med, min_max_ms=rng, p10_p90_ms=p10_90,
                                 loop_over_chain=med["loop"] / med["chain"], gradients_bit_equal=True, ms_per_step=r)
        print(f"B={B} H={H} (K={K}, saved {saved / 2 ** 30:.2f} GiB): " + ", ".join(
            f"{k} median {med[k]:.3f} ms (min {rng[k][0]:.3f}, max {rng[k][1]:.3f})" for k in fns) +
            f", loop / chain {med['loop'] / med['chain']:.3f}; gradients bit-equal", flush=True)
        del nets, engs, chain, loop, fns
        native._ws_cache.clear()
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"config": a.config, "rounds": a.rounds, "steps": a.steps, "cases": res}, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
