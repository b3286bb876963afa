"""DSTDGCN.predict / dstd_model_predict on the MI355X: any horizon from the
observed frames in one native call (include/dstd_gcn_predict.h).

The main criterion has no tolerance: ``model.predict(obs, H)`` is
``torch.equal`` to ``predict_loop(model, obs, H)`` (tests/predict_helper.py),
the window loop a caller writes with ``model(x)`` and torch indexing -- the
same forward kernels on the same windows, everything else is copies.  The
loop's bookkeeping is checked against a closed form, and window 0 against the
reference, in tests/test_predict_host.py; window 0 is tied to the fp64 fixture
here as well.  Later windows are not compared with a free-running oracle: the
random-weight fixture models amplify their input about 100x per window and
the stack is chaotic, so bit identity with the loop plus the forward parity of
tests/test_gpu_parity.py covers them.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import dstd_native as native
from conftest import group, load_npz, model_tol, rel_err
from guard_helper import FILLS, Guarded
from model import DSTDGCB, get_model
from model import dstdgcn_fast as F
from predict_helper import predict_loop
from test_gpu_model_chain import load_model
from test_gpu_train import randomise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EWORKSPACE = -2  # include/dstd_gcn.h
TAGS = ("h36m", "cmu", "3dpw", "h36m75")


def observations(B, Tin, V, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, Tin, V, 3, generator=g).to(DEV)


def fresh_loop(m, obs, H):
    """predict_loop on a workspace no earlier call left constants in: the
    loop's first forward folds the parameters as they are now."""
    native._ws_cache.clear()
    out = predict_loop(m, obs, H)
    torch.cuda.synchronize()
    return out


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(want).all(), what
    bad = int((got != want).flatten(1).any(1).sum())
    assert torch.equal(got, want), (what, f"{bad} samples differ", float((got - want).abs().max()))


def small_model(Tin, Tout, V=5, C=8, layers=1, seed=0):
    """A freshly built model outside the split-f16 shapes (the generic
    kernels): the h36m skeleton's first V joints as the graph, every dynamic
    term alive (randomise of tests/test_gpu_train.py)."""
    torch.manual_seed(900 + 10 * Tin + Tout + seed)
    m = get_model("dstdgcn", dstdgcn=dict(input_channels=6, input_time_frame=Tin, output_time_frame=Tout,
                                          st_gcnn_dropout=0.0, joints_to_consider=V, num_feature=C,
                                          num_layers=layers, layout="h36m"))
    for blk in m.modules():
        if isinstance(blk, DSTDGCB):
            A = blk.A_s.data[:, :V, :V].clone()
            blk.A_s = nn.Parameter(A, False)
            blk.W_s = nn.Parameter(torch.zeros_like(A))
            blk.R_s = nn.Parameter(A.clone())
    randomise(m, 17 + Tin)
    return m.to(DEV).eval()


# ---- 1. the fixture models -------------------------------------------------------
@pytest.mark.parametrize("arith", ["split", "fp32"])
@pytest.mark.parametrize("tag", TAGS)
def test_predict_is_the_window_loop(tag, arith):
    """B = 3, H = 2 * Tout + 3: three windows, the last truncated (h36m75:
    Tin = 50 > Tout = 25, every later window's observed part holds frames of
    x_k and of y_k)."""
    m, opts = load_model(tag)
    m.set_gc_arithmetic(arith)
    Tin, Tout, V = opts["input_time_frame"], opts["output_time_frame"], opts["joints_to_consider"]
    obs = torch.from_numpy(load_npz(f"model_{tag}.npz")["x"][:3, :Tin].copy()).to(DEV)
    H = 2 * Tout + 3
    got = m.predict(obs, H)
    assert got.shape == (3, H, V, 3) and got.is_contiguous() and not got.requires_grad
    same(got, fresh_loop(m, obs, H), (tag, arith))


def test_predict_under_the_fused_temporal_schedule():
    m, opts = load_model("h36m")
    m._dstd_fwd_flags = native.FWD_FUSED_TEMPORAL
    assert native.model_schedule(3, 35, 22, 64, 5, native.FWD_FUSED_TEMPORAL) == [(native.LAUNCH_MODEL, 0, 7)]
    obs = observations(3, 10, 22, 11)
    same(m.predict(obs, 53), fresh_loop(m, obs, 53), "fused")


# ---- 5. window 0 against the reference -------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_first_window_matches_the_fp64_fixture(tag):
    """The fixture inputs are windows padded with their last observed frame,
    so the first Tout frames predicted from x[:, :Tin] are the fixture's
    y64[:, Tin:], under the whole-model bar with the fixture's own fp32 error."""
    m, opts = load_model(tag)
    d = load_npz(f"model_{tag}.npz")
    Tin, Tout = opts["input_time_frame"], opts["output_time_frame"]
    obs = torch.from_numpy(d["x"][:3, :Tin].copy()).to(DEV)
    got = m.predict(obs, 2 * Tout + 3)[:, :Tout].cpu().numpy()
    err, tol = rel_err(got, d["y64"][:3, Tin:]), model_tol(d["ref32_err"])
    print(f"{tag}: window 0 vs y64[:, Tin:] {err:.3e} (bar {tol:.1e})")
    assert err <= tol


# ---- 2. the one-launch schedule ---------------------------------------------------
def test_predict_at_and_above_one_sample_per_compute_unit():
    """B = the device's compute units (from there the forward is one launch
    per sample by default) with H = Tout + 1, and B = that + 37 (a ragged
    second round of workgroups)."""
    m, opts = load_model("h36m")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (cus, cus + 37):
        assert native.model_schedule(B, 35, 22, 64, 5, 0) == [(native.LAUNCH_MODEL, 0, 7)]
        obs = observations(B, 10, 22, 20 + B)
        same(m.predict(obs, 26), fresh_loop(m, obs, 26), B)


# ---- 3. the generic kernels --------------------------------------------------------
@pytest.mark.parametrize("Tin,Tout", [(2, 4), (3, 3), (4, 2), (5, 1), (1, 5)])
def test_predict_small_windows(Tin, Tout):
    """T = 6, V = 5, 8 features, one encoder block, B = 2, H = 3 * Tout + 1
    (four windows): Tin > Tout mixes observed and predicted frames in the next
    window's observed part, Tout = 1 advances one frame per window, Tin = 1
    pads a single frame."""
    m = small_model(Tin, Tout)
    obs = observations(2, Tin, 5, 30 + Tin)
    H = 3 * Tout + 1
    same(m.predict(obs, H), fresh_loop(m, obs, H), (Tin, Tout))


# ---- 4. edges ----------------------------------------------------------------------
def test_predict_edges():
    m, opts = load_model("h36m")
    obs = observations(3, 10, 22, 41)
    x = obs[:, [min(s, 9) for s in range(35)]].contiguous()
    with torch.no_grad():
        y = m(x)
    one = m.predict(obs, 1)
    same(one, y[:, 10:11].contiguous(), "H = 1")
    same(m.predict(obs, 25), y[:, 10:].contiguous(), "H = Tout")
    same(m.predict(obs), y[:, 10:].contiguous(), "the default horizon")
    full = m.predict(obs, 53)
    same(m.predict(obs[:1].contiguous(), 53), full[:1].contiguous(), "B = 1 against row 0 of B = 3")
    empty = m.predict(obs[:0], 53)
    assert empty.shape == (0, 53, 22, 3) and empty.device == obs.device
    with pytest.raises(RuntimeError, match="eval"):
        m.train().predict(obs)


# ---- 6. the memory contract --------------------------------------------------------
def _c_predict(m, obs, H, ws, out, flags=0):
    B, Tin = obs.shape[:2]
    return native.lib().dstd_model_predict(m._native_params(), obs.data_ptr(), B, Tin, H, out.ptr, ws.ptr, ws.nbytes,
                                           native.stream_handle(obs.device), flags)


@pytest.mark.parametrize("which", ["h36m", "T6"])
def test_predict_memory_contract(which):
    """An exact-size workspace and an exact-size out between sentinel guards;
    the workspace filled with 0x00, 0xFF and 0x4B gives bit-identical out (the
    call reads nothing it has not written); obs is left alone; one byte less
    workspace is refused with the workspace and out untouched."""
    if which == "h36m":
        m, _ = load_model("h36m")
        B, Tin, Tout, V, C, layers = 3, 10, 25, 22, 64, 5
    else:
        B, Tin, Tout, V, C, layers = 2, 4, 2, 5, 8, 1
        m = small_model(Tin, Tout)
    H = 2 * Tout + 1
    obs = observations(B, Tin, V, 51)
    obs0 = obs.clone()
    need = native.lib().dstd_model_predict_workspace_bytes(B, Tin + Tout, V, C, layers)
    out_bytes = 4 * B * H * V * 3
    outs = []
    for fill in FILLS:
        ws, out = Guarded(need, fill, DEV), Guarded(out_bytes, fill, DEV)
        assert _c_predict(m, obs, H, ws, out) == 0
        torch.cuda.synchronize()
        ws.check(f"workspace, fill {fill:#x}")
        out.check(f"out, fill {fill:#x}")
        outs.append(out.view(torch.float32, (B, H, V, 3)).clone())
    assert torch.equal(obs, obs0)
    for fill, o in zip(FILLS[1:], outs[1:]):
        assert torch.equal(o.view(torch.int32), outs[0].view(torch.int32)), f"fill {fill:#x}"
    same(outs[0], fresh_loop(m, obs, H), which)
    # one byte short: refused, nothing written
    ws, out = Guarded(need - 1, 0x4B, DEV), Guarded(out_bytes, 0x4B, DEV)
    assert _c_predict(m, obs, H, ws, out) == EWORKSPACE
    torch.cuda.synchronize()
    ws.check("refused workspace")
    out.check("refused out")
    assert bool((ws.tensor == 0x4B).all()) and bool((out.tensor == 0x4B).all())
    assert torch.equal(obs, obs0)


# ---- 7. constants --------------------------------------------------------------------
def test_predict_shares_and_refolds_constants(monkeypatch):
    """model(x) then predict reuses the folded constants of the forward (same
    claim tag, same workspace layout); after an in-place update of a conv
    weight the next predict folds again.  Each predict equals a loop that
    folds for itself."""
    m, _ = load_model("h36m")
    obs = observations(3, 10, 22, 61)
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
        m.predict(obs, 53)  # grows the workspace to the predict size
        m(x)
        a = m.predict(obs, 53)
        y = m(x)
    assert reused == [False, True, True, True], reused
    monkeypatch.undo()
    same(a, fresh_loop(m, obs, 53), "after a forward")
    same(y[:, 10:].contiguous(), a[:, :25].contiguous(), "a forward on predict's constants")
    w = m.encoders[2][0].stgcn[0][0].conv_t[0].conv_f.weight
    with torch.no_grad():
        m.predict(obs, 53)
        w.mul_(1.25)
    monkeypatch.setattr(native, "workspace_claim", spy)
    del reused[:]
    b = m.predict(obs, 53)
    assert reused == [False], reused
    monkeypatch.undo()
    same(b, fresh_loop(m, obs, 53), "after an in-place update")
    assert not torch.equal(a, b)


# ---- 8. graph capture ------------------------------------------------------------------
def test_predict_graph_capture():
    """predict captured with torch.cuda.graph on one stream, replayed on a
    second input copied into the static tensor: equal to eager."""
    m, _ = load_model("h36m")
    obs1, obs2 = observations(3, 10, 22, 71), observations(3, 10, 22, 72)
    static = obs1.clone()
    cap = torch.cuda.Stream(device=DEV)
    cap.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(cap):
        for _ in range(2):  # library load, per-kernel attributes, workspace
            m.predict(static, 28)
    torch.cuda.current_stream(DEV).wait_stream(cap)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        out = m.predict(static, 28)
    ws = native._ws_cache.pop((str(static.device), cap.cuda_stream), None)  # lives in the graph's pool: keep it with g
    assert ws is not None
    g.replay()
    torch.cuda.synchronize()
    same(out.clone(), m.predict(obs1, 28), "replay, the captured input")
    static.copy_(obs2)
    g.replay()
    torch.cuda.synchronize()
    want = m.predict(obs2, 28)
    same(out.clone(), want, "replay, a second input")
    assert not torch.equal(want, m.predict(obs1, 28))
    del g, ws


# ---- 9. the custom op --------------------------------------------------------------------
def test_predict_custom_op_and_compile():
    m, _ = load_model("h36m")
    obs = observations(2, 10, 22, 81)
    tensors = list(m.parameters()) + list(m.buffers())
    with torch.no_grad():
        torch.library.opcheck(torch.ops.dstd.dstdgcn_predict.default, (obs, tensors, m._dstd_uid, 28, 0),
                              test_utils=("test_schema", "test_faketensor"))
        eager = m.predict(obs, 28)
        same(torch.ops.dstd.dstdgcn_predict(obs, tensors, m._dstd_uid, 28, 0), eager, "the op")
        fn = torch.compile(lambda o: m.predict(o, 28), backend="aot_eager")
        same(fn(obs), eager, "compiled")


# ---- 10. the channels-last model ------------------------------------------------------------
def test_fast_model_predict_is_its_window_loop():
    d = load_npz("dstdgcn_fast.npz")
    p = "model_h36m/"
    opts = {k[len(p + "opt/"):]: d[k].item() for k in d.files if k.startswith(p + "opt/")}
    m = F.DSTDGCN(**opts)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in group(d, p + "sd/").items()})
    m = m.to(DEV).eval()
    obs = torch.from_numpy(d[p + "x"][:3, :10].copy()).to(DEV)
    got = m.predict(obs, 53)
    assert got.shape == (3, 53, 22, 3)
    same(got, fresh_loop(m, obs, 53), "fast")


# ---- 11. the engine ---------------------------------------------------------------------------
class _Log:
    def info(self, *a, **k):
        pass


def _engine_and_loader(frames, seed):
    """The h36m fixture model in a PredictionEngine and two batches of two
    synthetic windows of ``frames`` frames over the 32-joint skeleton; the
    inputs hold the used dims, padded with the last observed frame."""
    from engine import PredictionEngine
    d = load_npz("engine.npz")
    m, _ = load_model("h36m")
    cfg = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5),
               loss=dict(joint=["jl2", 1]), n_out=1, transform="tsc", use_weight=False, inverse=True)
    eng = PredictionEngine(cfg, m, _Log())
    g = torch.Generator().manual_seed(seed)
    all_seqs = 0.5 * torch.randn(4, frames, 96, generator=g)
    inputs = all_seqs[:, :, torch.from_numpy(d["test/dim_used"]).long()].clone()
    inputs[:, 10:] = inputs[:, 9:10]
    loader = [(inputs[:2], None, None, all_seqs[:2]), (inputs[2:], None, None, all_seqs[2:])]
    tables = dict(dim_used=d["test/dim_used"], joint_to_ignore=d["test/joint_to_ignore"],
                  joint_equal=d["test/joint_equal"])
    return eng, m, loader, inputs, all_seqs, tables


def test_engine_horizon_of_one_window_is_the_plain_test():
    """horizon = output_n: the same outputs reach the same metric kernel (one
    workgroup per eval frame, summing in an order that does not depend on where
    the outputs start), so the per-frame metric is not merely within 1e-6 of
    test() without a horizon but bit-equal to it."""
    eng, m, loader, _, _, tables = _engine_and_loader(35, 91)
    frames = [1, 3, 7, 9, 13, 24]
    avg0, met0 = eng.test(loader, input_n=10, eval_frame=frames, **tables)
    avg1, met1 = eng.test(loader, input_n=10, eval_frame=frames, horizon=25, **tables)
    print("plain", met0, "horizon 25", met1)
    assert (np.abs(met1 - met0) <= 1e-6 * np.abs(met0)).all()
    assert np.array_equal(met0, met1) and avg0 == avg1


def test_engine_long_horizon_metric():
    """horizon = 55 (three windows), eval frames up to 54: the metric is the
    MPJPE of model.predict's output placed through the same tables, in numpy."""
    eng, m, loader, inputs, all_seqs, tables = _engine_and_loader(65, 92)
    frames = [0, 1, 24, 25, 30, 49, 50, 54]
    avg, met = eng.test(loader, input_n=10, eval_frame=frames, horizon=55, **tables)
    obs = inputs[:, :10].reshape(4, 10, 22, 3).contiguous().to(DEV)
    out = m.predict(obs, 55).reshape(4, 55, 66).cpu().numpy().astype(np.float64)
    targ = all_seqs.numpy().astype(np.float64)
    pred = targ.copy()
    pred[:, 10:, tables["dim_used"]] = out
    ji, je = tables["joint_to_ignore"], tables["joint_equal"]
    for c in range(3):
        pred[:, :, ji * 3 + c] = pred[:, :, je * 3 + c]
    t3, p3 = targ.reshape(4, 65, 32, 3), pred.reshape(4, 65, 32, 3)
    want = np.array([np.linalg.norm(t3[:, 10 + f] - p3[:, 10 + f], axis=-1).mean() for f in frames])
    print("engine", met, "numpy", want)
    assert np.isfinite(want).all()
    assert (np.abs(met - want) <= 1e-5 * np.abs(want)).all()  # per frame: the windows differ in magnitude
    assert abs(avg - want.mean()) <= 1e-5 * want.mean()


def test_engine_horizon_refusals():
    eng, m, loader, inputs, all_seqs, tables = _engine_and_loader(35, 93)
    with pytest.raises(ValueError, match="frames"):  # all_seqs holds 35 frames, not 10 + 30
        eng.test(loader, input_n=10, eval_frame=[1], horizon=30, **tables)
    with pytest.raises(ValueError, match="list"):
        eng.test([([inputs[:2]], None, None, all_seqs[:2])], input_n=10, eval_frame=[1], horizon=25, **tables)

    class _Time:
        def transform(self, x):
            return x

        inverse = transform

    with pytest.raises(ValueError, match="time"):
        eng.test(loader, input_n=10, eval_frame=[1], horizon=25, time_tsfm=_Time(), **tables)
