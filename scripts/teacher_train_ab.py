#!/usr/bin/env python
"""A/B of scheduled sampling through a rollout: the hand-written window loop
with a torch.where per boundary against
PredictionEngine.train(horizon=H, teacher_ratio=r).

  python scripts/teacher_train_ab.py [--rounds 8 --steps 10 --ratio 0.5 --parent-lib LIB --json OUT]
Both legs are one optimizer step of the engine's configuration (inverse pass,
jl2 loss through weighted_losses, in-place gradient arena, fused Adam) on twin
models at H36M, H = 100 (four windows), B = 32 and 256: ``loop`` draws the mask
as the engine does and rolls the windows out with ``model.forward_pair`` per
window (tests/teacher_helper.py teacher_loop_pair -- what can be written
without the teacher arguments), ``chain`` is the engine's own step
(include/ext/dstd_gcn_teacher.h).  Every step is timed on its own, wall clock
around one device synchronise; a round is ``--steps`` steps of one leg then of
the other, both warmed first.  Before anything is timed the two legs' losses
and gradients are compared bit for bit under one seed (the same mask; dropout
off: each leg draws its own dropout seeds); the timed steps run the shipped
dropout and draw a mask per step.

--parent-lib: also time the free-running step (teacher_ratio = 0) of this tree's
library against a library built from the parent commit (loaded through DSTD_LIB
with DSTD_AB_FOREIGN_LIB=1), one worker process per library, rounds
interleaved.  It is the same code path, so the two ranges should overlap;
--this-first swaps the order in which the two workers start and take turns.
"""
import argparse
import copy
import json
import os
import subprocess
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
from teacher_helper import teacher_loop_pair  # noqa: E402

H = 100
BATCHES = (32, 256)
CFG = dict(learn=dict(opt="adam", lr=1e-4, weight_decay=0, gamma=0.9, step_size=5), loss=dict(joint=["jl2", 1]),
           n_out=1, transform="tsc", use_weight=False, inverse=True)


class _Log:
    def info(self, *a):
        pass


def loop_step(eng, inputs, inputs_inv, targets, ratio, step=True):
    net = eng.model.model
    n_in = net.input_time_frame
    obs = eng.transform(inputs)[:, :n_in].contiguous()
    obs_inv = eng.transform(inputs_inv)[:, :n_in].contiguous()
    K = -(-H // net.output_time_frame)
    mask = torch.rand(K, 2 * obs.shape[0], device=obs.device) < ratio
    preds = [eng.inverse(o) for o in teacher_loop_pair(net, obs, obs_inv, H, eng.transform(targets), mask)]
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


def batch(B, n_in, V, dev):
    seq = 0.5 * torch.randn(B, n_in + H, V * 3, generator=torch.Generator().manual_seed(B + H)).to(dev)
    return seq.clone(), seq.flip(1).contiguous(), seq


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)),
                p10_ms=float(np.percentile(v, 10)), p90_ms=float(np.percentile(v, 90)))


def worker(a):
    """The free-running step on the library this process loaded: a round of
    timed steps per line read, the times written back as one JSON line."""
    dev = torch.device("cuda", 0)
    model, opts, _ = bench.load_model(a.config, dev)
    eng = PredictionEngine(CFG, model.train(), _Log())
    model._dstd_inplace_grads = True
    inputs, inputs_inv, seq = batch(a.worker, opts["input_time_frame"], opts["joints_to_consider"], dev)
    fn = lambda: eng._step_rollout(inputs, inputs_inv, seq, H, None, None, False)  # noqa: E731
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "go":
            break
        print(json.dumps([timed_step(fn) for _ in range(a.steps)]), flush=True)


def free_running_ab(a, B):
    """teacher_ratio = 0 on this tree's library and on the parent's, interleaved."""
    procs = {}
    order = (("parent", os.path.abspath(a.parent_lib)), ("this", None))
    for name, lib in order[::-1] if a.this_first else order:  # the order the workers start and take their turns in
        env = dict(os.environ)
        if lib:
            env.update(DSTD_LIB=lib, DSTD_AB_FOREIGN_LIB="1")
        procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", str(B), "--steps",
                                        str(a.steps), "--config", a.config], env=env, stdin=subprocess.PIPE,
                                       stdout=subprocess.PIPE, text=True)
    r = {k: [] for k in procs}

    def answer(k, p, accept):  # the worker's next line that is an answer (its imports may print others)
        for line in p.stdout:
            if accept(line.strip()):
                return line.strip()
        raise SystemExit(f"the {k} worker ended early")

    try:
        for k, p in procs.items():
            answer(k, p, lambda s: s == "ready")
        for _ in range(a.rounds):
            for k, p in procs.items():
                p.stdin.write("go\n")
                p.stdin.flush()
                r[k] += json.loads(answer(k, p, lambda s: s.startswith("[")))
    finally:
        for p in procs.values():
            p.stdin.close()
            p.wait(timeout=60)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--ratio", type=float, default=0.5)
    ap.add_argument("--config", default="h36m")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--this-first", action="store_true", help="start and time this tree's worker before the parent's")
    ap.add_argument("--batches", type=int, nargs="+", default=list(BATCHES))
    ap.add_argument("--json", default=None)
    ap.add_argument("--worker", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker is not None:
        return worker(a)
    dev = torch.device("cuda", 0)
    model, opts, _ = bench.load_model(a.config, dev)
    n_in, V = opts["input_time_frame"], opts["joints_to_consider"]
    res = {}
    for B in a.batches:
        nets = [copy.deepcopy(model).train() for _ in range(2)]
        engs = [PredictionEngine(CFG, m, _Log()) for m in nets]
        for m in nets:
            m._dstd_inplace_grads = True  # as PredictionEngine.train sets it for its steps
        inputs, inputs_inv, seq = batch(B, n_in, V, dev)
        chain = lambda: engs[0]._step_rollout(inputs, inputs_inv, seq, H, None, None, False, a.ratio)  # noqa: E731
        loop = lambda: loop_step(engs[1], inputs, inputs_inv, seq, a.ratio)  # noqa: E731
        # gradients first, bit for bit: one seed, so one mask; no dropout, no update
        for m in nets:
            m.do_in.p = 0.0
        opt_step = engs[0].optimizer.step
        engs[0].optimizer.step = lambda: None
        torch.manual_seed(7)
        la = chain()[0]
        torch.manual_seed(7)
        lb = loop_step(engs[1], inputs, inputs_inv, seq, a.ratio, step=False)
        engs[0].optimizer.step = opt_step
        torch.cuda.synchronize()
        bad = [n for (n, p), q in zip(nets[0].named_parameters(), nets[1].parameters())
               if p.grad is not None and not torch.equal(p.grad, q.grad)]
        if bad or not torch.equal(la.reshape(-1), lb.detach().reshape(-1)):
            raise SystemExit(f"B={B}: the chain's loss or gradients differ from the loop's: {bad[:5]}")
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
            print(f"  B={B} round {i + 1}/{a.rounds}", flush=True)
        case = dict(ratio=a.ratio, gradients_bit_equal=True, ms_per_step=r, **{k: stats(v) for k, v in r.items()})
        case["loop_over_chain"] = case["loop"]["median_ms"] / case["chain"]["median_ms"]
        print(f"B={B} H={H} ratio {a.ratio}: " + ", ".join(
            f"{k} median {case[k]['median_ms']:.3f} ms (min {case[k]['min_ms']:.3f}, max {case[k]['max_ms']:.3f})"
            for k in fns) + f", loop / chain {case['loop_over_chain']:.3f}; gradients bit-equal", flush=True)
        del nets, engs, chain, loop, fns
        native._ws_cache.clear()
        torch.cuda.empty_cache()
        if a.parent_lib:
            fr = free_running_ab(a, B)
            case["free_running"] = dict(ms_per_step=fr, **{k: stats(v) for k, v in fr.items()})
            case["free_running"]["this_over_parent"] = (case["free_running"]["this"]["median_ms"] /
                                                        case["free_running"]["parent"]["median_ms"])
            print(f"B={B} H={H} ratio 0: " + ", ".join(
                f"{k} median {s['median_ms']:.3f} ms (min {s['min_ms']:.3f}, max {s['max_ms']:.3f})"
                for k, s in case["free_running"].items() if isinstance(s, dict) and "median_ms" in s) +
                f", this / parent {case['free_running']['this_over_parent']:.3f}", flush=True)
        res[f"B{B}_H{H}"] = case
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"config": a.config, "rounds": a.rounds, "steps": a.steps, "cases": res}, f, indent=1)
        print("wrote", a.json)


if __name__ == "__main__":
    main()
