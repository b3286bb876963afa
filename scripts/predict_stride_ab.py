"""What predicting with a stride costs: one H36M-shaped batch, predicted two ways.

B = 256 observations of 10 frames (N(0,1) poses), the h36m fixture model
(tests/golden/model_h36m.npz), horizon 100, strides 5, 10 and 25 (20, 10 and 4
windows):

  native   model.predict(obs, 100, stride=S): one call of
           dstd_model_predict_strided (include/ext/dstd_gcn_stride.h); for
           S = 25 = output_time_frame that is dstd_model_predict, today's chain
  loop     tests/stride_helper.py's predict_strided_loop on the same tree: one
           model(x) per window, the windows built with torch indexing and
           torch.cat -- what a caller writes without the native call

Both arms of every stride run in this one process, interleaved over --rounds
rounds after one warm-up round.  A sample is the wall time of --calls
consecutive calls ending in one device synchronise, divided by --calls.  The
random-weight fixture model amplifies its input from window to window, so at
20 windows the values overflow; the time of these kernels does not depend on
the values, and the two arms are compared in bits (NaN included), not in value.

The native launch count is not timed: one launch for window 0, then per window
the forward's launches from dstd_model_fwd_schedule and one glue launch (the
constants are reused from the call before: no preparation launches).

  python scripts/predict_stride_ab.py [--rounds 10] [--calls 10] [--out FILE.json]
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
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "dstd-gcn_amd")):
    sys.path.insert(0, p)

HORIZON, STRIDES = 100, (5, 10, 25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed sample")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import dstd_native as native
    from model import get_model
    from stride_helper import predict_strided_loop

    dev = torch.device("cuda", 0)
    d = np.load(os.path.join(ROOT, "tests", "golden", "model_h36m.npz"), allow_pickle=False)
    opts = {k[4:]: d[k].item() for k in d.files if k.startswith("opt/")}
    m = get_model("dstdgcn", dstdgcn=opts)
    m.load_state_dict({k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd/")})
    m = m.to(dev).eval()
    Tin, Tout, V = opts["input_time_frame"], opts["output_time_frame"], opts["joints_to_consider"]
    obs = torch.randn(a.batch, Tin, V, 3, generator=torch.Generator().manual_seed(0)).to(dev)

    arms = {}
    for S in STRIDES:
        arms[f"native_s{S}"] = lambda S=S: m.predict(obs, HORIZON, stride=S)
        arms[f"loop_s{S}"] = lambda S=S: predict_strided_loop(m, obs, HORIZON, S)

    def timed(arm, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            out = arms[arm]()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls, out

    outs = {arm: timed(arm, 2)[1] for arm in arms}  # warm-up round: kernels loaded, allocator settled
    identical = {S: bool(torch.equal(outs[f"native_s{S}"].view(torch.int32), outs[f"loop_s{S}"].view(torch.int32)))
                 for S in STRIDES}
    finite = {S: bool(torch.isfinite(outs[f"loop_s{S}"]).all()) for S in STRIDES}
    del outs
    ms = {arm: [] for arm in arms}
    for r in range(a.rounds):
        for arm in arms:
            t, _ = timed(arm, a.calls)
            ms[arm].append(round(t, 4))
            print(f"round {r} {arm}: {t:.3f} ms/call", flush=True)

    fwd = len(native.model_schedule(a.batch, Tin + Tout, V, opts["num_feature"], opts["num_layers"]))
    per_stride = {}
    for S in STRIDES:
        n, l = ms[f"native_s{S}"], ms[f"loop_s{S}"]
        K = -(-HORIZON // S)
        per_stride[str(S)] = {
            "windows": K,
            "native_ms": {"min": min(n), "median": round(statistics.median(n), 4), "max": max(n)},
            "loop_ms": {"min": min(l), "median": round(statistics.median(l), 4), "max": max(l)},
            "ratio_loop_over_native_median": round(statistics.median(l) / statistics.median(n), 4),
            "ranges_overlap": not (max(n) < min(l) or max(l) < min(n)),
            "native_launches_per_call": 1 + K * (fwd + 1),
            "loop_forwards_per_call": K,
            "bit_identical": identical[S],
            "loop_output_finite": finite[S],
        }
    result = {
        "metric": "predict_stride_ms", "unit": "ms/call", "batch": a.batch, "horizon": HORIZON, "rounds": a.rounds,
        "calls_per_sample": a.calls,
        "config": {"workload": f"h36m T={Tin}+{Tout}, V={V}, B={a.batch}, fixture model, N(0,1) observations",
                   "timing": "wall of calls_per_sample consecutive calls ending in one device synchronise, per call; "
                             "arms interleaved in one process after one warm-up round",
                   "native": "model.predict(obs, horizon, stride=S); S = output_time_frame is dstd_model_predict",
                   "loop": "tests/stride_helper.py predict_strided_loop: model(x) per window, torch indexing and cat",
                   "launches": "window 0 + per window (dstd_model_fwd_schedule + 1 glue), constants reused; not timed"},
        "per_round_ms": ms,
        "strides": per_stride,
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
