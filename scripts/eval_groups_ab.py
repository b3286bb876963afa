"""What the per-action table costs: one H36M-shaped test set, evaluated two ways.

15 groups x 256 synthetic windows (T = 35, D = 96, the 22 used joints and the
ignored / copied joints of tests/golden/engine.npz), the h36m fixture model
(tests/golden/model_h36m.npz), the protocol's eight eval frames:

  per_group   the runners' way (runner/h36m.py:106-135): one PredictionEngine.test
              per group over that group's own resident set, DeviceLoader at
              batch_size = 32 -- 15 calls, 15 synchronisations, all_seqs gathered
  grouped     PredictionEngine.test_groups once over the one resident set that
              holds all groups, DeviceLoader(batch_size = 256) mixing them --
              one synchronisation, the targets read from the resident frames

Both arms run in this one process, interleaved over --rounds rounds after one
warm-up round; wall time per full table, each arm ending in its own
synchronisation(s) plus one device synchronise.  The launch counts are not
timed: per batch, the forward's launches from dstd_model_fwd_schedule for that
batch size, one gather and one metric launch (torch's element-wise kernels of
the tsc transform and its inverse, the same per batch in both arms, are not
counted).

  python scripts/eval_groups_ab.py [--rounds 10] [--out FILE.json]
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

T, D, INPUT_N, OUTPUT_N = 35, 96, 10, 25
EVAL_FRAME = [1, 3, 7, 9, 13, 17, 21, 24]


class _Log:
    def info(self, *a, **k):
        pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--groups", type=int, default=15)
    ap.add_argument("--windows", type=int, default=256, help="per group")
    ap.add_argument("--batch-per-group", type=int, default=32)
    ap.add_argument("--batch-grouped", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import dstd_native as native
    from dstd_data import DeviceLoader, DeviceSequences
    from engine import PredictionEngine
    from model import get_model

    dev = torch.device("cuda", 0)
    golden = os.path.join(ROOT, "tests", "golden")
    d = np.load(os.path.join(golden, "model_h36m.npz"), allow_pickle=False)
    e = np.load(os.path.join(golden, "engine.npz"), allow_pickle=False)
    opts = {k[4:]: d[k].item() for k in d.files if k.startswith("opt/")}
    m = get_model("dstdgcn", dstdgcn=opts)
    m.load_state_dict({k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd/")})
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5), loss=dict(joint=["jl2", 1]),
               n_out=1, transform="tsc", use_weight=False, inverse=True)
    eng = PredictionEngine(cfg, m.to(dev).eval(), _Log())
    dim_used = e["test/dim_used"]
    tables = dict(joint_to_ignore=e["test/joint_to_ignore"], joint_equal=e["test/joint_equal"])

    rng = np.random.default_rng(0)
    G, n = a.groups, a.windows
    windows = np.cumsum(rng.normal(0, 10, (G * n, T, D)), 1)
    groups = np.repeat(np.arange(G), n)
    names = [f"act{g:02d}" for g in range(G)]
    one_set = DeviceSequences.from_windows(windows, dim_used, INPUT_N, OUTPUT_N, device=dev, groups=groups,
                                           group_names=names)
    # mixed: a shuffled loader, so that every batch holds rows of many groups
    grouped_loader = DeviceLoader(one_set, a.batch_grouped, shuffle=True, seed=1)
    per_group_loaders = [DeviceLoader(DeviceSequences.from_windows(windows[groups == g], dim_used, INPUT_N, OUTPUT_N,
                                                                   device=dev), a.batch_per_group) for g in range(G)]

    def per_group():
        avg, met, table = 0.0, np.zeros(len(EVAL_FRAME)), {}
        for name, ld in zip(names, per_group_loaders):
            avg_g, met_g = eng.test(ld, INPUT_N, EVAL_FRAME, dim_used, action=name, **tables)
            table[name] = (avg_g, met_g)
            avg += avg_g
            met += met_g
        return avg / G, met / G, table

    def grouped():
        return eng.test_groups(grouped_loader, INPUT_N, EVAL_FRAME, **tables)

    arms = {"per_group": per_group, "grouped": grouped}

    def timed(arm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = arms[arm]()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    results = {arm: timed(arm)[1] for arm in arms}  # warm-up round: kernels loaded, allocator settled
    worst = max(float(np.abs(results["grouped"][2][k][1] - results["per_group"][2][k][1]).max()
                      / np.abs(results["per_group"][2][k][1]).max()) for k in names)
    ms = {arm: [] for arm in arms}
    for r in range(a.rounds):
        for arm in arms:
            t, _ = timed(arm)
            ms[arm].append(round(t, 4))
            print(f"round {r} {arm}: {t:.3f} ms/table", flush=True)
    med = {arm: statistics.median(v) for arm, v in ms.items()}

    V, feat, layers = opts["joints_to_consider"], opts["num_feature"], opts["num_layers"]

    def launches(batch, batches):
        full, last = batches
        per = {b: len(native.model_schedule(b, T, V, feat, layers)) + 2 for b in {batch, last} if b}
        return full * per[batch] + (per[last] if last else 0)

    def split(windows_n, batch):
        return windows_n // batch, windows_n % batch

    counts = {"per_group": G * launches(a.batch_per_group, split(n, a.batch_per_group)),
              "grouped": launches(a.batch_grouped, split(G * n, a.batch_grouped))}
    result = {
        "metric": "eval_table_ms", "unit": "ms/table", "groups": G, "windows_per_group": n, "rounds": a.rounds,
        "batch": {"per_group": a.batch_per_group, "grouped": a.batch_grouped},
        "config": {"workload": f"h36m T={T} D={D} V={V}, {len(EVAL_FRAME)} eval frames, fixture model",
                   "timing": "wall per full table incl. every synchronisation of the arm, arms interleaved in one process",
                   "launches": "forward launches of dstd_model_fwd_schedule + gather + metric, per batch; not timed"},
        "per_round_ms": ms,
        "median_ms": {arm: round(v, 4) for arm, v in med.items()},
        "min_ms": {arm: min(v) for arm, v in ms.items()},
        "ratio_per_group_over_grouped": round(med["per_group"] / med["grouped"], 4),
        "native_launches_per_table": counts,
        "synchronisations_per_table": {"per_group": G, "grouped": 1},
        "max_rel_difference_of_the_tables": worst,
        "avg": {arm: round(float(results[arm][0]), 6) for arm in arms},
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
