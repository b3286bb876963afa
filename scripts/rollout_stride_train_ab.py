#!/usr/bin/env python
"""A/B of training through a strided rollout: the hand-written window loop
against PredictionEngine.train(horizon=H, stride=S).

  python scripts/rollout_stride_train_ab.py [--rounds 10 --steps 10 --config h36m --cases 32:10,32:25 --json OUT]
Both legs are one optimizer step of the engine's configuration (inverse pass,
jl2 loss through weighted_losses, in-place gradient arena, fused Adam) on twin
models: ``loop`` is tests/rollout_stride_helper.py's StridedLoop over
``model.forward_pair`` -- every window a detached leaf built with torch
indexing, the backward composed by hand with one torch.autograd.backward per
window, what can be written without ``rollout(stride=)`` -- and ``chain`` is
the engine's own step over ``rollout_pair(stride=)``
(include/ext/dstd_gcn_stride_train.h; at S = output_time_frame the unstrided
entry points).  Every step is timed on its own, wall clock around one device
synchronise; a round is ``--steps`` steps of one leg then of the other, both
warmed first.  Before anything is timed the two legs' losses and gradients are
compared bit for bit (dropout off: each leg draws its own seeds); the timed
steps run the shipped dropout.  Cases are B:S pairs at H = 100; a case whose
saved windows do not fit in free device memory is reported and skipped.
--json writes every step's time and the saved bytes of each case
(dstd_model_rollout_saved_bytes at the pair's 2 B).
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
from rollout_stride_helper import model_loop_pair  # noqa: E402

H = 100
CFG = dict(learn=dict(opt="adam", lr=1e-4, weight_decay=0, gamma=0.9, step_size=5), loss=dict(joint=["jl2", 1]),
           n_out=1, transform="tsc", use_weight=False, inverse=True)


class _Log:
    def info(self, *a):
        pass


def loop_step(eng, inputs, inputs_inv, targets, S, step=True):
    net = eng.model.model
    n_in, n = net.input_time_frame, inputs.shape[0]
    obs = eng.transform(inputs)[:, :n_in].contiguous()
    obs_inv = eng.transform(inputs_inv)[:, :n_in].contiguous()
    loop = model_loop_pair(net, obs, obs_inv, H, S)
    o = loop.out.requires_grad_()
    out = weighted_losses(eng.model.loss_spec, [eng.inverse(o[:n]), eng.inverse(o[n:])], targets,
                          [(n_in, 1), (H - 1, -1)], None)
    eng.optimizer.zero_grad()
    (out.sum() / 2).backward()
    loop.backward(o.grad, eng.model.model.parameters())
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--config", default="h36m")
    ap.add_argument("--cases", default="32:10,32:25,256:25,256:10")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    model, opts, _ = bench.load_model(a.config, dev)
    n_in, n_out, V = opts["input_time_frame"], opts["output_time_frame"], opts["joints_to_consider"]
    L = native.lib()
    res = {}
    for B, S in (tuple(int(v) for v in c.split(":")) for c in a.cases.split(",")):
        K = -(-H // S)
        saved = int(L.dstd_model_rollout_saved_bytes(2 * B, n_in + n_out, V, opts["num_feature"], opts["num_layers"], K))
        free = torch.cuda.mem_get_info(dev)[0]
        tag = f"B{B}_S{S}"
        if saved * 1.15 > free:  # (the chain's saved, plus the step's other buffers)
            print(f"B={B} S={S} (K={K}): saved {saved / 2 ** 30:.1f} GiB does not fit in {free / 2 ** 30:.1f} GiB free: "
                  "skipped", flush=True)
            res[tag] = dict(windows=K, saved_bytes=saved, skipped="saved does not fit", free_bytes=int(free))
            continue
        nets = [copy.deepcopy(model).train() for _ in range(2)]
        engs = [PredictionEngine(CFG, m, _Log()) for m in nets]
        for m in nets:
            m._dstd_inplace_grads = True  # as PredictionEngine.train sets it for its steps
        seq = 0.5 * torch.randn(B, n_in + H, V * 3, generator=torch.Generator().manual_seed(B + S)).to(dev)
        inputs, inputs_inv = seq.clone(), seq.flip(1).contiguous()
        chain = lambda: engs[0]._step_rollout(inputs, inputs_inv, seq, H, None, None, False, 0.0, S)  # noqa: E731
        loop = lambda: loop_step(engs[1], inputs, inputs_inv, seq, S)  # noqa: E731
        # losses and gradients first, bit for bit, without dropout and without the update
        for m in nets:
            m.do_in.p = 0.0
        opt_step = engs[0].optimizer.step
        engs[0].optimizer.step = lambda: None
        la, lb = chain()[0], loop_step(engs[1], inputs, inputs_inv, seq, S, step=False)
        engs[0].optimizer.step = opt_step
        torch.cuda.synchronize()
        # (a NaN equals a NaN here: with random weights the backward through ten windows can overflow at B = 256)
        same = lambda x, y: bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all())  # noqa: E731
        bad = [n for (n, p), q in zip(nets[0].named_parameters(), nets[1].parameters())
               if p.grad is not None and not same(p.grad, q.grad)]
        finite = all(bool(torch.isfinite(p.grad).all()) for p in nets[0].parameters() if p.grad is not None)
        if bad or not same(la.reshape(-1), lb.detach().reshape(-1)):
            raise SystemExit(f"B={B} S={S}: the chain's loss or gradients differ from the loop's: {bad[:5]}")
        for m in nets:
            m.do_in.p = float(opts["st_gcnn_dropout"])
        fns = {"loop": loop, "chain": chain}
        for _ in range(2):
            for f in fns.values():
                f()
        r = {k: [] for k in fns}
        for i in range(a.rounds):
            for k, f in fns.items():
                r[k] += [timed_step(f) for _ in range(a.steps)]
            print(f"  B={B} S={S} round {i + 1}/{a.rounds}", flush=True)
        med = {k: float(np.median(v)) for k, v in r.items()}
        rng = {k: (float(min(v)), float(max(v))) for k, v in r.items()}
        p10_90 = {k: (float(np.percentile(v, 10)), float(np.percentile(v, 90))) for k, v in r.items()}
        res[tag] = dict(windows=K, saved_bytes=saved, median_ms=med, min_max_ms=rng, p10_p90_ms=p10_90,
                        loop_over_chain=med["loop"] / med["chain"], gradients_bit_equal=True,
                        gradients_finite=finite, ms_per_step=r)
        print(f"B={B} S={S} (K={K}, saved {saved / 2 ** 30:.2f} GiB): " + ", ".join(
            f"{k} median {med[k]:.3f} ms (min {rng[k][0]:.3f}, max {rng[k][1]:.3f})" for k in fns) +
            f", loop / chain {med['loop'] / med['chain']:.3f}; gradients bit-equal, finite: {finite}", flush=True)
        del nets, engs, chain, loop, fns
        native._ws_cache.clear()
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"config": a.config, "horizon": H, "rounds": a.rounds, "steps": a.steps, "cases": res}, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
