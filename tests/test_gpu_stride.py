"""DSTDGCN.predict(stride=) / dstd_model_predict_strided on the MI355X: every
window contributes its first ``stride`` frames and the next one observes the
last input_n frames known by then, in one native call
(include/ext/dstd_gcn_stride.h).

The criterion has no tolerance: ``model.predict(obs, H, stride=S)`` is
``torch.equal`` to ``predict_strided_loop(model, obs, H, S)``
(tests/stride_helper.py), the window loop a caller writes with ``model(x)`` and
torch indexing -- the same forward kernels on the same windows, everything else
is copies.  The loop's bookkeeping is checked against a per-frame recursion in
tests/test_stride_host.py.

A condition on the inputs, not a measurement: the random-weight models amplify
their input about 100x per window, so every case keeps K = ceil(H / S) <= 8 and
the loop's output is finite; ``same`` asserts that of the reference side.
"""
import numpy as np
import pytest
import torch

import dstd_native as native
from conftest import group, load_npz
from dstd_data import DeviceLoader, DeviceSequences
from guard_helper import FILLS, Guarded
from model import dstdgcn_fast as F
from predict_helper import predict_loop
from stride_helper import predict_strided_loop
from test_gpu_model_chain import load_model
from test_gpu_predict import fresh_loop, observations, same, small_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, EWORKSPACE, ELIMIT = -1, -2, -3  # include/dstd_gcn.h
TAGS = ("h36m", "cmu", "3dpw", "h36m75")


def fresh_strided_loop(m, obs, H, S):
    """predict_strided_loop on a workspace no earlier call left constants in:
    the loop's first forward folds the parameters as they are now."""
    native._ws_cache.clear()
    out = predict_strided_loop(m, obs, H, S)
    torch.cuda.synchronize()
    return out


# ---- 1. the generic kernels --------------------------------------------------------
SMALL = [(4, 2, 1, 5),   # S < Tin: several windows read obs, older out and y_k together
         (2, 4, 3, 10),  # S > Tin, the last window truncated
         (3, 3, 2, 7),
         (1, 5, 2, 9),   # a single observed frame
         (5, 1, 1, 4),
         (2, 4, 4, 9),   # S = Tout
         (3, 3, 2, 1)]   # H < S


@pytest.mark.parametrize("Tin,Tout,S,H", SMALL)
def test_strided_predict_small_windows(Tin, Tout, S, H):
    """T = 6, V = 5, 8 features, one encoder block, B = 2."""
    assert -(-H // S) <= 8
    m = small_model(Tin, Tout)
    obs = observations(2, Tin, 5, 130 + 10 * Tin + S)
    got = m.predict(obs, H, stride=S)
    assert got.shape == (2, H, 5, 3) and got.is_contiguous() and not got.requires_grad
    same(got, fresh_strided_loop(m, obs, H, S), (Tin, Tout, S, H))
    if S == Tout:  # today's chain: the existing entry point, and the same frames
        same(got, m.predict(obs, H), "stride = Tout against no stride")
        same(got, fresh_loop(m, obs, H), "stride = Tout against the unstrided loop")


# ---- 2. the fixture models ---------------------------------------------------------
@pytest.mark.parametrize("arith", ["split", "fp32"])
@pytest.mark.parametrize("tag", TAGS)
def test_strided_predict_is_the_window_loop(tag, arith):
    """B = 3, S = 10, H = 53: six windows, the last truncated to three frames.
    h36m75 (Tin = 50): every window's observation mixes obs, frames of out
    written by earlier launches and frames of y_k."""
    m, opts = load_model(tag)
    m.set_gc_arithmetic(arith)
    Tin, V = opts["input_time_frame"], opts["joints_to_consider"]
    assert opts["output_time_frame"] >= 10
    obs = torch.from_numpy(load_npz(f"model_{tag}.npz")["x"][:3, :Tin].copy()).to(DEV)
    got = m.predict(obs, 53, stride=10)
    assert got.shape == (3, 53, V, 3) and got.is_contiguous() and not got.requires_grad
    same(got, fresh_strided_loop(m, obs, 53, 10), (tag, arith))


def test_strided_predict_above_one_sample_per_compute_unit():
    """B = the device's compute units + 37 (the forward is one launch per
    sample, with a ragged second round of workgroups; the glue's rows spread
    over more than one wave per workgroup and many workgroups), S = 10, H = 26."""
    m, _ = load_model("h36m")
    B = torch.cuda.get_device_properties(0).multi_processor_count + 37
    obs = observations(B, 10, 22, 220)
    same(m.predict(obs, 26, stride=10), fresh_strided_loop(m, obs, 26, 10), B)


def test_strided_predict_empty_batch_and_tracing():
    m, _ = load_model("h36m")
    obs = observations(2, 10, 22, 230)
    empty = m.predict(obs[:0], 53, stride=10)
    assert empty.shape == (0, 53, 22, 3) and empty.device == obs.device

    class Sub(torch.Tensor):
        pass

    with pytest.raises(NotImplementedError, match="stride"):  # the tracing branch: the custom op has no stride
        m.predict(obs.as_subclass(Sub), 28, stride=10)
    same(m.predict(obs, 28, stride=25), m.predict(obs, 28), "stride = Tout is the call without a stride")


# ---- 3. the memory contract --------------------------------------------------------
def _c_strided(m, obs, H, S, ws, out, flags=0):
    B, Tin = obs.shape[:2]
    return native.lib().dstd_model_predict_strided(
        native.ext_stride.model_params_ref(m._native_params()), obs.data_ptr(), B, Tin, H, S, out.ptr, ws.ptr,
        ws.nbytes, native.stream_handle(obs.device), flags)


@pytest.mark.parametrize("which", ["h36m", "T6"])
def test_strided_predict_memory_contract(which):
    """An exact-size workspace and an exact-size out between sentinel guards;
    the workspace and out filled with 0x00, 0xFF and 0x4B give bit-identical
    out (the call reads nothing it has not written -- of out, only frames that
    earlier launches of the same call wrote); obs is left alone; a refused call
    -- one byte less workspace, a stride outside 1..Tout, 65 windows -- leaves
    the workspace and out untouched."""
    if which == "h36m":
        m, _ = load_model("h36m")
        B, Tin, Tout, V, C, layers, S, H = 3, 10, 25, 22, 64, 5, 10, 53
    else:
        B, Tin, Tout, V, C, layers, S, H = 2, 4, 2, 5, 8, 1, 1, 5
        m = small_model(Tin, Tout)
    L = native.lib()
    obs = observations(B, Tin, V, 151)
    obs0 = obs.clone()
    need = L.dstd_model_predict_strided_workspace_bytes(B, Tin + Tout, V, C, layers)
    assert need <= L.dstd_model_predict_workspace_bytes(B, Tin + Tout, V, C, layers)
    out_bytes = 4 * B * H * V * 3
    outs = []
    for fill in FILLS:
        ws, out = Guarded(need, fill, DEV), Guarded(out_bytes, fill, DEV)
        assert _c_strided(m, obs, H, S, ws, out) == 0
        torch.cuda.synchronize()
        ws.check(f"workspace, fill {fill:#x}")
        out.check(f"out, fill {fill:#x}")
        outs.append(out.view(torch.float32, (B, H, V, 3)).clone())
    assert torch.equal(obs, obs0)
    for fill, o in zip(FILLS[1:], outs[1:]):
        assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32)), f"fill {fill:#x}"
    same(outs[0], fresh_strided_loop(m, obs, H, S), which)
    # refused: nothing written
    refusals = (("one byte short", need - 1, H, S, EWORKSPACE), ("stride 0", need, H, 0, EINVAL),
                ("stride Tout + 1", need, H, Tout + 1, EINVAL), ("65 windows", need, 64 * S + 1, S, ELIMIT))
    for what, nbytes, h, s, code in refusals:
        ws, out = Guarded(nbytes, 0x4B, DEV), Guarded(out_bytes, 0x4B, DEV)
        assert _c_strided(m, obs, h, s, ws, out) == code, what
        torch.cuda.synchronize()
        ws.check(f"refused workspace, {what}")
        out.check(f"refused out, {what}")
        assert bool((ws.tensor == 0x4B).all()) and bool((out.tensor == 0x4B).all()), what
        assert torch.equal(obs, obs0)


# ---- 4. constants ------------------------------------------------------------------
def test_strided_predict_shares_and_refolds_constants(monkeypatch):
    """model(x), predict(stride=10) and predict() of one batch size reuse one
    another's folded constants (same claim tag, the forward's region laid out
    alike); after an in-place update of a conv weight the next strided call
    folds again.  Each equals a loop that folds for itself."""
    m, _ = load_model("h36m")
    obs = observations(3, 10, 22, 161)
    x = obs[:, [min(s, 9) for s in range(35)]].contiguous()
    reused = []
    claim = native.workspace_claim

    def spy(device, nbytes, tag):
        buf, r = claim(device, nbytes, tag)
        reused.append(r)
        return buf, r

    native._ws_cache.clear()
    monkeypatch.setattr(native, "workspace_claim", spy)
    with torch.no_grad():
        m.predict(obs, 53)  # grows the workspace to the largest of the three sizes
        y = m(x)
        a = m.predict(obs, 53, stride=10)
        b = m.predict(obs, 53)
        y2 = m(x)
    assert reused == [False, True, True, True, True], reused
    monkeypatch.undo()
    same(a, fresh_strided_loop(m, obs, 53, 10), "strided, after a forward")
    same(b, fresh_loop(m, obs, 53), "unstrided, after a strided call")
    same(y[:, 10:20].contiguous(), a[:, :10].contiguous(), "window 0 of the strided call")
    same(y2, y, "a forward on the strided call's constants")
    w = m.encoders[2][0].stgcn[0][0].conv_t[0].conv_f.weight
    with torch.no_grad():
        m.predict(obs, 53, stride=10)
        w.mul_(1.25)
    monkeypatch.setattr(native, "workspace_claim", spy)
    del reused[:]
    c = m.predict(obs, 53, stride=10)
    assert reused == [False], reused
    monkeypatch.undo()
    same(c, fresh_strided_loop(m, obs, 53, 10), "after an in-place update")
    assert not torch.equal(a, c)


# ---- 5. graph capture --------------------------------------------------------------
def test_strided_predict_graph_capture():
    """A strided predict captured with torch.cuda.graph on one stream, replayed
    on new observations copied into the static tensor: equal to the loop."""
    m, _ = load_model("h36m")
    obs1, obs2 = observations(3, 10, 22, 171), observations(3, 10, 22, 172)
    static = obs1.clone()
    cap = torch.cuda.Stream(device=DEV)
    cap.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(cap):
        for _ in range(2):  # library load, per-kernel attributes, workspace
            m.predict(static, 28, stride=10)
    torch.cuda.current_stream(DEV).wait_stream(cap)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        out = m.predict(static, 28, stride=10)
    ws = native._ws_cache.pop((str(static.device), cap.cuda_stream), None)  # lives in the graph's pool: keep it with g
    assert ws is not None
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    static.copy_(obs2)
    g.replay()
    torch.cuda.synchronize()
    second = out.clone()
    same(first, fresh_strided_loop(m, obs1, 28, 10), "replay, the captured input")
    want = fresh_strided_loop(m, obs2, 28, 10)
    same(second, want, "replay, new observations")
    assert not torch.equal(first, second)
    del g, ws


# ---- 6. the channels-last model ----------------------------------------------------
def test_fast_model_strided_predict_is_its_window_loop():
    d = load_npz("dstdgcn_fast.npz")
    p = "model_h36m/"
    opts = {k[len(p + "opt/"):]: d[k].item() for k in d.files if k.startswith(p + "opt/")}
    m = F.DSTDGCN(**opts)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in group(d, p + "sd/").items()})
    m = m.to(DEV).eval()
    obs = torch.from_numpy(d[p + "x"][:3, :10].copy()).to(DEV)
    got = m.predict(obs, 53, stride=10)
    assert got.shape == (3, 53, 22, 3)
    same(got, fresh_strided_loop(m, obs, 53, 10), "fast")
    same(m.predict(obs, 53, stride=25), m.predict(obs, 53), "fast, stride = Tout")


# ---- 7. the engine -----------------------------------------------------------------
class _Log:
    def info(self, *a, **k):
        pass


CFG = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5), loss=dict(joint=["jl2", 1]),
           n_out=1, transform="tsc", use_weight=False, inverse=True)
GROUPS = np.array([0, 1, 0, 1, 1])


def _engine_case():
    """The h36m fixture model in a PredictionEngine and a resident set of five
    synthetic windows of 10 + 53 frames over the 32-joint skeleton, once with
    two groups (test_groups) and once without (test)."""
    from engine import PredictionEngine
    d = load_npz("engine.npz")
    m, _ = load_model("h36m")
    eng = PredictionEngine(CFG, m, _Log())
    x = 0.5 * np.random.default_rng(245).normal(size=(5, 63, 96))
    du = d["test/dim_used"]
    kw = dict(eval_frame=[0, 9, 10, 19, 20, 49, 50, 52], joint_to_ignore=d["test/joint_to_ignore"],
              joint_equal=d["test/joint_equal"])
    grouped = DeviceSequences.from_windows(x, du, 10, 53, device=DEV, groups=GROUPS)
    plain = DeviceSequences.from_windows(x, du, 10, 53, device=DEV)
    return eng, m, x.astype(np.float32), du, kw, grouped, plain


def _numpy_metric(x32, out, du, kw, rows):
    """The per-frame MPJPE of ``out`` [n, 53, 66] placed through the tables,
    over the windows ``rows``: tests/test_gpu_predict.py's restatement."""
    targ = x32.astype(np.float64)[rows]
    pred = targ.copy()
    pred[:, 10:, du] = out[rows]
    ji, je = kw["joint_to_ignore"], kw["joint_equal"]
    for c in range(3):
        pred[:, :, ji * 3 + c] = pred[:, :, je * 3 + c]
    n = len(targ)
    t3, p3 = targ.reshape(n, 63, 32, 3), pred.reshape(n, 63, 32, 3)
    return np.array([np.linalg.norm(t3[:, 10 + f] - p3[:, 10 + f], axis=-1).mean() for f in kw["eval_frame"]])


def test_engine_strided_horizon_metric():
    """test(horizon=53, stride=10) and test_groups(horizon=53, stride=10):
    the metric is the MPJPE of predict_strided_loop's output in numpy, per
    frame within the 1e-5 of the long-horizon engine tests (an fp32 sum of a
    few dozen norms against fp64)."""
    eng, m, x32, du, kw, grouped, plain = _engine_case()
    obs = torch.from_numpy(x32[:, :10][:, :, du].reshape(5, 10, 22, 3).copy()).to(DEV)
    out = fresh_strided_loop(m, obs, 53, 10)
    assert torch.isfinite(out).all()
    out = out.reshape(5, 53, 66).cpu().numpy().astype(np.float64)
    want = _numpy_metric(x32, out, du, kw, np.arange(5))
    avg, met = eng.test(DeviceLoader(plain, 2), input_n=10, dim_used=du, horizon=53, stride=10, **kw)
    print("test", met, "numpy", want)
    assert np.isfinite(want).all() and (want > 0).all()
    assert (np.abs(met - want) <= 1e-5 * np.abs(want)).all() and abs(avg - want.mean()) <= 1e-5 * want.mean()
    avg_g, met_g, table = eng.test_groups(DeviceLoader(grouped, 2), input_n=10, horizon=53, stride=10, **kw)
    assert list(table) == ["0", "1"]
    per_group = [_numpy_metric(x32, out, du, kw, np.flatnonzero(GROUPS == g)) for g in (0, 1)]
    for g in (0, 1):
        print("group", g, "test_groups", table[str(g)][1], "numpy", per_group[g])
        assert (np.abs(table[str(g)][1] - per_group[g]) <= 1e-5 * np.abs(per_group[g])).all()
        assert abs(table[str(g)][0] - per_group[g].mean()) <= 1e-5 * per_group[g].mean()
    mean = (per_group[0] + per_group[1]) / 2
    assert (np.abs(met_g - mean) <= 1e-5 * mean).all() and abs(avg_g - mean.mean()) <= 1e-5 * mean.mean()
    # the stride reaches the model: the unstrided chain gives another table
    assert not np.array_equal(met, eng.test(DeviceLoader(plain, 2), input_n=10, dim_used=du, horizon=53, **kw)[1])


def test_engine_stride_of_a_whole_window_is_the_call_without_stride():
    eng, m, x32, du, kw, grouped, plain = _engine_case()
    avg0, met0 = eng.test(DeviceLoader(plain, 2), input_n=10, dim_used=du, horizon=53, **kw)
    avg1, met1 = eng.test(DeviceLoader(plain, 2), input_n=10, dim_used=du, horizon=53, stride=25, **kw)
    assert np.isfinite(met0).all() and np.array_equal(met0, met1) and avg0 == avg1
    a0, t0, tab0 = eng.test_groups(DeviceLoader(grouped, 2), input_n=10, horizon=53, **kw)
    a1, t1, tab1 = eng.test_groups(DeviceLoader(grouped, 2), input_n=10, horizon=53, stride=25, **kw)
    assert a0 == a1 and np.array_equal(t0, t1) and list(tab0) == list(tab1)
    for name in tab0:
        assert tab0[name][0] == tab1[name][0] and np.array_equal(tab0[name][1], tab1[name][1])
    with pytest.raises(ValueError, match="stride"):
        eng.test_groups(DeviceLoader(grouped, 2), input_n=10, horizon=53, stride=26, **kw)
