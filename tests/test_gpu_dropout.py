"""do_in dropout of the native training path (k_dropout, csrc/dstd_train.hip;
dstd_model_train_fwd_sync / _bwd_sync, csrc/dstd_train_capi.hip) against the
fp64 oracle with the same mask.

The mask is a hash of (seed, element index, p); tests/dropout_helper.py
restates it on the host (pinned by tests/test_dropout_host.py), so the oracle
(oracle/dstdgcn_oracle.py ``drop=``) is an independent reference of a
train-mode step with dropout: y, dx, every parameter gradient and the running
statistics, through the C ABI with host and device seeds, the Python paths,
forward_pair, the channels-last model, the rollout chains and graph replays.

Criterion: the one of tests/test_gpu_train.py unchanged -- every tensor's error
over its fp32 noise floor (fp32_noise: the fp32 oracle with the same mask on
the CPU, on the GPU and over sample orders, the mask rows travelling with the
samples) under check_ratios, y and dx as two more tensors; running statistics
within 1e-5; bit identity where two native paths must agree.  One flipped mask
element moves dx by 30x .. 2000x its floor (tests/test_dropout_host.py).

Models: (A) test_gpu_predict.small_model(3, 3) -- T 6, V 5, C 8, one layer,
B 4, the generic kernels; (B) one encoder layer at the H36M shape -- T 35,
V 22, C 64, B 2.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import dropout_helper as D
import dstd_native as native
import rollout_helper as RH
import rollout_stride_helper as SH
from conftest import model_tol, rel_err
from model import get_model
from oracle import dstdgcn_oracle as O
from test_gpu_guards import NAN_OUT, Bufs, _clones, _guard_model_stats, _model_stats_of, _same
from test_gpu_predict import small_model
from test_gpu_train import N_ORDERS, check_ratios, fp32_noise, noise_ratios, rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = [0, 11, 0xFFFFFFFF12345678]
BATCH = {"A": 4, "B": 2}
GRID_ELEMENTS = 4096 * 256  # grid_for's cap times the block: k_dropout's grid stride


@functools.lru_cache(maxsize=None)
def case(name, B=None):
    """(CPU model, its state dict, x, dy) -- the inputs of tests/test_dropout_host.py."""
    m = D.model_a() if name == "A" else D.model_b()
    B = BATCH[name] if B is None else B
    x, dy = D.step_inputs(m, B, 40 + B)
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}, x, dy


def on_gpu(name, p):
    m = copy.deepcopy(case(name)[0]).to(DEV).train()
    m.do_in.p = p
    return m


def h_shape(m, B):
    return (B, m.num_feature, m.input_time_frame + m.output_time_frame, m.joints_to_consider)


def test_model_a_is_the_small_model():
    sd = case("A")[1]
    m = on_gpu("A", 0.0)
    assert [t.data_ptr() for t in model_stats(m)] == [t.data_ptr() for t in _model_stats_of(m)]
    other = small_model(3, 3).state_dict()
    assert sd.keys() == other.keys() and all(torch.equal(sd[k], other[k].cpu()) for k in sd)


# ---- the reference ---------------------------------------------------------------------
_REFS = {}


def orders_for(B):
    """Sample orders of the noise floor.  The project's 8 under-sample a batch
    of four: the two residual.0.bias gradients are analytically zero (a
    train-mode BatchNorm follows the conv), so their floor is the largest of a
    few draws of pure rounding noise over B * T * V = 120 terms, and with 8
    orders model (A) at p = 0 -- no mask at all -- put conv_st_out's at 5.94x
    once and above 3x three times in 60 input draws (p = 0.1: 4.92x once, above
    3x twice); with 24 draws of B = 4's 24 orders the largest of 60 is 2.80x at
    p = 0 and 2.75x at p = 0.1.  Every other tensor stays below 1.7x either
    way.  B = 2 has two orders, and B = 24 keeps the 8."""
    return 24 if B == 4 else N_ORDERS


def reference(key, sd, layers, xs, dys, drops, fast=False, oracle_dev="cpu"):
    """(fp64 step {y, dx, gradients}, per-tensor fp32 noise floor, per batch the
    BatchNorm records) of dropout_helper.oracle_step; cached by ``key``."""
    if key not in _REFS:
        r64 = D.oracle_step(sd, layers, xs, dys, drops, device=oracle_dev, fast=fast, record=True)
        stats = r64.pop("stats")

        def step(dev, perm):
            return D.oracle_step(sd, layers, xs, dys, drops, torch.float32, dev, fast,
                                 None if perm is None else [perm] * len(xs))

        _REFS[key] = (r64, fp32_noise(sd, (xs[0],), r64, n_orders=orders_for(xs[0].shape[0]), step=step), stats)
    return _REFS[key]


def check(got, ref, what):
    r64, noise, _ = ref
    assert set(r64) <= set(got), (what, set(r64) - set(got))
    check_ratios(noise_ratios(got, r64, noise), what)


def check_stats(new, old, recs, what):
    """(1 - m) * old + m * batch, m = 0.1, once per batch in call order,
    against the oracle's BN_RECORD (test_dstdgcb_train_forward_backward)."""
    assert len(new) == len(old) == 2 * len(recs[0]), what
    for i in range(len(recs[0])):
        for j in range(2):
            want = old[2 * i + j].double().cpu()
            for rec in recs:
                want = 0.9 * want + 0.1 * rec[i][j].double().cpu()
            assert rel(new[2 * i + j], want) < 1e-5, (what, i, j)


# ---- the native steps ------------------------------------------------------------------
def _u64(values):
    return (ctypes.c_uint64 * len(values))(*values)


def _device_seeds(values):
    return torch.from_numpy(np.array(values, dtype=np.uint64).view(np.int64)).to(DEV)


def abi_step(m, x, dy, drop, seed, flags=0, device_seed=False):
    """dstd_model_train_fwd_ex and _bwd_ex on guarded copies of the running
    statistics: {y, dx, stat<i>, parameter name: gradient}."""
    L, st = native.lib(), native.stream_handle(torch.device(DEV))
    n, t, v, _ = x.shape
    C, layers = m.num_feature, m.num_layers
    b = Bufs()
    p = native.ModelParams.from_buffer_copy(m._native_params())
    stats = _guard_model_stats(b, p, m)
    seed_t = None
    if device_seed:
        seed_t = _device_seeds([seed])
        seed, flags = seed_t.data_ptr(), flags | native.TRAIN_SEED_DEVICE
    ns = L.dstd_model_train_saved_bytes(n, t, v, C, layers)
    nw = L.dstd_model_train_workspace_bytes(n, t, v, C, layers)
    saved, ws = b.new("saved", ns, 0x4B), b.new("workspace", nw, 0x4B)
    y, dx = b.f32("y", x.shape, NAN_OUT), b.f32("dx", x.shape, NAN_OUT)
    native.check(L.dstd_model_train_fwd_ex(p, x.data_ptr(), n, 0.1, drop, seed, y.data_ptr(), saved.ptr, ns, st, flags),
                 "dstd_model_train_fwd_ex")
    params = list(m.parameters())
    arena = native.GradArena(params, torch.device(DEV), buf=b.f32("arena", (native.arena_numel(params),), 0))
    native.check(L.dstd_model_train_bwd_ex(p, x.data_ptr(), n, drop, seed, saved.ptr, ns, dy.data_ptr(),
                                           m._native_grads(arena), dx.data_ptr(), ws.ptr, nw, st, flags),
                 "dstd_model_train_bwd_ex")
    b.check()
    out = {"y": y, "dx": dx}
    out.update({f"stat{i}": s for i, s in enumerate(stats)})
    out.update({name: g for (name, _), g in zip(m.named_parameters(), arena.views()) if g is not None})
    return {k: v_.detach().clone() for k, v_ in out.items()}


def stats_of(got):
    return [got[f"stat{i}"] for i in range(sum(k.startswith("stat") for k in got))]


def model_stats(m):
    """Every BatchNorm's (running_mean, running_var) in the forward's (= the
    oracle's BN_RECORD) order, for the base and the channels-last model."""
    out = []
    blocks = [m.conv_st_in, m.bn_in] + [mod for enc in m.encoders for mod in (enc[0], enc[1])] + [m.conv_st_out]
    for mod in blocks:
        if hasattr(mod, "stgcn"):
            blk = mod.stgcn[0][0]
            if blk.in_channels != blk.out_channels:
                out += [blk.residual[1].bn.running_mean, blk.residual[1].bn.running_var]
            out += [blk.bn.bn.running_mean, blk.bn.bn.running_var]
        else:
            out += [mod.bn.running_mean, mod.bn.running_var]
    return out


def python_step(m, xs, dys, pair=False):
    """model(x) or model.forward_pair(x1, x2) and the backward of
    sum (y * dy): ({y, dx, parameter name: .grad}, statistics before, after)."""
    old = _clones(model_stats(m))
    m.zero_grad(set_to_none=True)
    xg = [x.to(DEV).requires_grad_(True) for x in xs]
    ys = m.forward_pair(*xg) if pair else (m(xg[0]),)
    sum((y * dy.to(DEV)).sum() for y, dy in zip(ys, dys)).backward()
    got = {"y": torch.cat([y.detach() for y in ys]), "dx": torch.cat([x.grad for x in xg])}
    got.update({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    return got, old, model_stats(m)


# ---- 1. the C ABI with a host seed --------------------------------------------------------
def _abi_case(name, seed, p):
    m0, sd, x, dy = case(name)
    drop = D.drop_tensor(seed, h_shape(m0, x.shape[0]), p)
    ref = reference((name, seed, float(p)), sd, m0.num_layers, [x], [dy], [drop])
    m = on_gpu(name, 0.0)  # (the C ABI takes p itself)
    got = abi_step(m, x.to(DEV), dy.to(DEV), float(p), seed)
    what = f"model {name} seed {seed:#x} p {float(p):.9g}"
    check(got, ref, what)
    check_stats(stats_of(got), _model_stats_of(m), ref[2], what)
    return got


@pytest.mark.parametrize("seed", SEEDS, ids=[hex(s) for s in SEEDS])
@pytest.mark.parametrize("name", ["A", "B"])
def test_abi_step_matches_the_masked_oracle(name, seed):
    _abi_case(name, seed, 0.1)


def test_abi_step_at_half():
    m0 = case("A")[0]
    keep = D.keep_mask(11, int(np.prod(h_shape(m0, 4))), 0.5)
    assert 0.4 < keep.mean() < 0.6 and float(D.keep_scale(0.5)) == 2.0
    _abi_case("A", 11, 0.5)


def test_abi_step_at_the_threshold():
    """u >= p at p = u[e0] (e0 kept) and at the next float32 (e0 dropped): each
    step matches its own restated mask, and the two differ."""
    m0 = case("A")[0]
    n = int(np.prod(h_shape(m0, 4)))
    u = D.uniforms(11, n)
    e0 = int(np.abs(u - np.float32(0.1)).argmin())
    p_at, p_above = u[e0], np.nextafter(u[e0], np.float32(1))
    assert D.keep_mask(11, n, p_at)[e0] and not D.keep_mask(11, n, p_above)[e0]
    at, above = _abi_case("A", 11, p_at), _abi_case("A", 11, p_above)
    assert not torch.equal(at["y"], above["y"]) and not torch.equal(at["dx"], above["dx"])


# ---- 2. the second pass of k_dropout's grid stride ----------------------------------------
def test_abi_step_past_one_grid_of_elements():
    """(B) at B 24: 1,182,720 elements of h[0], 134,144 of them in the second
    pass of the grid-stride loop.  Oracle and noise as torch ops on the GPU."""
    B, seed = 24, 11
    m0, sd, x, dy = case("B", B)
    n = int(np.prod(h_shape(m0, B)))
    assert GRID_ELEMENTS < n < 2 * GRID_ELEMENTS
    keep = D.keep_mask(seed, n, 0.1)
    assert not np.array_equal(keep[GRID_ELEMENTS:], keep[:n - GRID_ELEMENTS])  # a restarted stream is another mask
    drop = D.drop_tensor(seed, h_shape(m0, B), 0.1)
    ref = reference(("B", B, seed), sd, m0.num_layers, [x], [dy], [drop], oracle_dev=DEV)
    m = on_gpu("B", 0.0)
    got = abi_step(m, x.to(DEV), dy.to(DEV), 0.1, seed)
    check(got, ref, "model B at B 24")


# ---- 3. the seed read from the device -----------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS[1:], ids=[hex(s) for s in SEEDS[1:]])
@pytest.mark.parametrize("name", ["A", "B"])
def test_device_seed_is_the_host_seed(name, seed):
    _, _, x, dy = case(name)
    m = on_gpu(name, 0.0)
    host = abi_step(m, x.to(DEV), dy.to(DEV), 0.1, seed)
    _same(host, abi_step(m, x.to(DEV), dy.to(DEV), 0.1, seed, device_seed=True), f"model {name} seed {seed:#x}")
    other = abi_step(m, x.to(DEV), dy.to(DEV), 0.1, seed ^ 1, device_seed=True)
    assert not torch.equal(other["y"], host["y"])


# ---- 4. the Python eager path -------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["autograd", "inplace"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_python_step_matches_the_masked_oracle(name, inplace):
    m0, sd, x, dy = case(name)
    m = on_gpu(name, 0.1)
    m._dstd_inplace_grads = inplace
    (seed,) = D.drawn_seeds(5, DEV)
    drop = D.drop_tensor(seed, h_shape(m0, x.shape[0]), 0.1)
    ref = reference((name, seed, 0.1), sd, m0.num_layers, [x], [dy], [drop])
    got, old, new = python_step(m, [x], [dy])
    what = f"model {name} python inplace={inplace}"
    check(got, ref, what)
    check_stats(new, old, ref[2], what)


# ---- 5. forward_pair ------------------------------------------------------------------
def _pair_inputs(name):
    m0, sd, x, dy = case(name)
    B = x.shape[0]
    x2, dy2 = D.step_inputs(m0, B, 90 + B)
    return m0, sd, [x, x2.flip(1).contiguous()], [dy, dy2]


@pytest.mark.parametrize("name", ["A", "B"])
def test_forward_pair_masks_are_two_halves_of_one_stream(name):
    """One seed over [2n][C][T][V]: the second half's mask is the stream's
    second half, not the first half's again; BatchNorm statistics per half."""
    m0, sd, xs, dys = _pair_inputs(name)
    B = xs[0].shape[0]
    m = on_gpu(name, 0.1)
    m._dstd_inplace_grads = True  # the engine's step
    (seed,) = D.drawn_seeds(6, DEV)
    drop = D.drop_tensor(seed, h_shape(m0, 2 * B), 0.1)
    assert not torch.equal(drop[:B], drop[B:])
    ref = reference((name, "pair", seed), sd, m0.num_layers, xs, dys, [drop[:B], drop[B:]])
    got, old, new = python_step(m, xs, dys, pair=True)
    check(got, ref, f"model {name} forward_pair")
    check_stats(new, old, ref[2], f"model {name} forward_pair")


# ---- 6. the channels-last model -----------------------------------------------------------
def fast_model_a(p):
    fm, fsd = D.fast_model_a(p)
    return fm.to(DEV).train(), fsd


@pytest.mark.parametrize("pair", [False, True], ids=["forward", "forward_pair"])
def test_fast_model_masks_in_the_shadow_layout(pair):
    """The channels-last model runs the shadow's kernels: the mask is indexed
    [B][C][T][V] there, [N, T, V, C] in the channels-last oracle."""
    m0, sd, xs, dys = _pair_inputs("A")
    if not pair:
        xs, dys = xs[:1], dys[:1]
    B = xs[0].shape[0]
    fm, fsd = fast_model_a(0.1)
    (seed,) = D.drawn_seeds(7, DEV)
    drop = D.drop_tensor(seed, h_shape(m0, len(xs) * B), 0.1)
    ref = reference(("fast", pair, seed), fsd, 1, xs, dys, list(drop.chunk(len(xs))), fast=True)
    got, old, new = python_step(fm, xs, dys, pair=pair)
    check(got, ref, f"fast model A pair={pair}")
    check_stats(new, old, ref[2], f"fast model A pair={pair}")


def test_fast_model_follows_p_and_the_training_flag():
    """do_in of the outer module decides: p set after construction is the
    shadow's p, and model.eval() under autograd applies no mask."""
    m0, sd, x, dy = case("A")
    fm, fsd = fast_model_a(0.0)
    with torch.no_grad():
        fm(x.to(DEV))  # (the shadow exists now, with p = 0)
    fm.do_in.p = 0.1
    (seed,) = D.drawn_seeds(8, DEV)
    drop = D.drop_tensor(seed, h_shape(m0, x.shape[0]), 0.1)
    ref = reference(("fast", "late p", seed), fsd, 1, [x], [dy], [drop], fast=True)
    got, _, _ = python_step(fm, [x], [dy])
    check(got, ref, "fast model A, p set late")
    fm.eval()
    xg = x.to(DEV).requires_grad_(True)
    y = fm(xg)
    assert y.grad_fn is not None
    # (the train-mode step above moved the running statistics: the module's state as it is now)
    P = {k: v.detach().double().cpu() for k, v in fm.state_dict().items() if not k.endswith("num_batches_tracked")}
    y64 = O.fast_dstdgcn_fn(x.double(), P, 1).numpy()
    y32 = O.fast_dstdgcn_fn(x, {k: v.float() for k, v in P.items()}, 1).numpy()
    assert rel_err(y.detach().cpu().numpy(), y64) <= model_tol(rel_err(y32, y64))


# ---- 7. the chains ------------------------------------------------------------------------
def chain_call(m, obs, dout, H, S, drop, seeds):
    """dstd_model_rollout_fwd / _bwd (S None) or the strided pair, free running."""
    L, st = native.lib(), native.stream_handle(obs.device)
    B, Tin, V, _ = obs.shape
    T, C, layers = Tin + m.output_time_frame, m.num_feature, m.num_layers
    K = RH.windows(T, Tin, H) if S is None else SH.windows(H, S)
    assert K == len(seeds)
    b = Bufs()
    p = native.ModelParams.from_buffer_copy(m._native_params())
    _guard_model_stats(b, p, m)
    pref = native.ext.model_params_ref(p)
    ns = L.dstd_model_rollout_saved_bytes(B, T, V, C, layers, K)
    nw = (L.dstd_model_rollout_workspace_bytes(B, T, V, C, layers) if S is None else
          L.dstd_model_rollout_strided_workspace_bytes(B, T, V, C, layers, Tin, H))
    saved, ws = b.new("saved", ns, 0x4B), b.new("workspace", nw, 0x4B)
    out, dobs = b.f32("out", (B, H, V, 3), NAN_OUT), b.f32("dobs", obs.shape, NAN_OUT)
    sd = _u64(seeds)
    params = list(m.parameters())
    arena = native.GradArena(params, obs.device, buf=b.f32("arena", (native.arena_numel(params),), 0))
    gref = native.ext.model_grads_ref(m._native_grads(arena))
    free = (None, 0, None, None, None)
    if S is None:
        native.check(L.dstd_model_rollout_fwd(pref, obs.data_ptr(), B, Tin, H, 0.1, drop, sd, out.data_ptr(), saved.ptr,
                                              ns, st, 0), "dstd_model_rollout_fwd")
        native.check(L.dstd_model_rollout_bwd(pref, B, Tin, H, drop, sd, saved.ptr, ns, dout.data_ptr(), gref,
                                              dobs.data_ptr(), ws.ptr, nw, st, 0), "dstd_model_rollout_bwd")
    else:
        native.check(L.dstd_model_rollout_strided_fwd(pref, obs.data_ptr(), B, Tin, H, S, 0.1, drop, sd, out.data_ptr(),
                                                      saved.ptr, ns, *free, st, 0), "dstd_model_rollout_strided_fwd")
        native.check(L.dstd_model_rollout_strided_bwd(pref, B, Tin, H, S, drop, sd, saved.ptr, ns, dout.data_ptr(), gref,
                                                      dobs.data_ptr(), ws.ptr, nw, *free, st, 0),
                     "dstd_model_rollout_strided_bwd")
    b.check()
    res = {"out": out, "dobs": dobs}
    res.update({n: g for (n, _), g in zip(m.named_parameters(), arena.views()) if g is not None})
    return {k: v.detach().clone() for k, v in res.items()}


def chain_loop(m, obs, dout, H, S, drop, seeds):
    """The same by a window loop of dstd_model_train_fwd_ex / _bwd_ex with the
    windows' seeds, the frame shuffling in torch indexing and the backward glue
    of rollout_helper (S None) / rollout_stride_helper on float32 numpy arrays;
    gradients accumulate into one arena, window K-1 first."""
    L, st = native.lib(), native.stream_handle(obs.device)
    B, Tin, V, _ = obs.shape
    T, C, layers = Tin + m.output_time_frame, m.num_feature, m.num_layers
    Tout = T - Tin
    K = len(seeds)
    b = Bufs()
    p = native.ModelParams.from_buffer_copy(m._native_params())
    _guard_model_stats(b, p, m)
    ns = L.dstd_model_train_saved_bytes(B, T, V, C, layers)
    nw = L.dstd_model_train_workspace_bytes(B, T, V, C, layers)
    mfr = [min(s, Tin - 1) for s in range(T)]
    xs, saved, outs, h = [], [], [], obs
    x = obs[:, mfr].contiguous()
    for k in range(K):
        if S is not None:
            x = h[:, [k * S + i for i in mfr]].contiguous()
        y = torch.empty_like(x)
        saved.append(b.new(f"saved {k}", ns, 0x4B))
        native.check(L.dstd_model_train_fwd_ex(p, x.data_ptr(), B, 0.1, drop, seeds[k], y.data_ptr(), saved[k].ptr, ns, st,
                                               0), "dstd_model_train_fwd_ex")
        xs.append(x)
        if S is None:
            outs.append(y[:, Tin:Tin + min(Tout, H - k * Tout)])
            x = torch.cat([x[:, :Tin], y[:, Tin:]], 1)[:, [Tout + i for i in mfr]].contiguous()
        else:
            outs.append(y[:, Tin:Tin + min(S, H - k * S)])
            h = torch.cat([h[:, :k * S], x[:, :Tin], outs[-1]], 1)
    params = list(m.parameters())
    arena = native.GradArena(params, obs.device, buf=b.f32("arena", (native.arena_numel(params),), 0))
    grads = m._native_grads(arena)
    ws = b.new("workspace", nw, 0x4B)
    d_np = dout.cpu().numpy()
    G = None if S is None else np.zeros((B, Tin + H, V, 3), dtype=np.float32)
    for k in range(K - 1, -1, -1):
        dy = RH.glue_dy(d_np, G, T, Tin, k) if S is None else SH.glue_dy(G, d_np, T, Tin, S, k)
        dy, dx = torch.from_numpy(dy).to(DEV), torch.empty_like(xs[k])
        native.check(L.dstd_model_train_bwd_ex(p, xs[k].data_ptr(), B, drop, seeds[k], saved[k].ptr, ns, dy.data_ptr(),
                                               grads, dx.data_ptr(), ws.ptr, nw, st, 0), "dstd_model_train_bwd_ex")
        dx = dx.cpu().numpy()
        G = RH.glue_fold(dx, G, T, Tin) if S is None else SH.glue_acc(G, dx, None, T, Tin, S, k)
    b.check()
    dobs = RH.glue_obs(G, T, Tin) if S is None else G[:, :Tin]
    res = {"out": torch.cat(outs, 1), "dobs": torch.from_numpy(np.ascontiguousarray(dobs)).to(DEV)}
    res.update({n: g for (n, _), g in zip(m.named_parameters(), arena.views()) if g is not None})
    return {k: v.detach().clone() for k, v in res.items()}


@pytest.mark.parametrize("S,H", [(None, 8), (2, 5)], ids=["rollout", "stride-2"])
def test_chains_with_masks_are_the_seeded_loop(S, H):
    """Three windows with the host seeds 11, 0xFFFFFFFF12345678 and 3 at
    p = 0.1 on (A): out, dobs and every gradient of the chain equal the loop's
    bit for bit (the backward regenerates window k's mask from seed k), and
    window 0 is the masked oracle's forward."""
    m0, sd, _, _ = case("A")
    seeds, B, Tin = [11, 0xFFFFFFFF12345678, 3], 2, 3
    g = torch.Generator().manual_seed(75)
    obs, dout = torch.randn(B, Tin, 5, 3, generator=g).to(DEV), torch.randn(B, H, 5, 3, generator=g).to(DEV)
    m = on_gpu("A", 0.0)
    got, want = chain_call(m, obs, dout, H, S, 0.1, seeds), chain_loop(m, obs, dout, H, S, 0.1, seeds)
    assert got.keys() == want.keys()
    for k in got:
        assert bool(torch.isfinite(want[k]).all()) and torch.equal(got[k], want[k]), (k, rel(got[k], want[k]))
    assert float(got["dobs"].abs().max()) > 0
    unmasked = chain_call(m, obs, dout, H, S, 0.0, seeds)
    assert not torch.equal(unmasked["out"], got["out"]) and not torch.equal(unmasked["dobs"], got["dobs"])
    # window 0 against the oracle with seed 11's mask
    x0 = obs.cpu()[:, [min(s, Tin - 1) for s in range(6)]]
    P = {k: v.double() for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    drop = D.drop_tensor(11, h_shape(m0, B), 0.1)
    y64 = O.dstdgcn_fn(x0.double(), P, 1, training=True, drop=drop).numpy()
    y32 = O.dstdgcn_fn(x0, {k: v.float() for k, v in P.items()}, 1, training=True, drop=drop.float()).numpy()
    take = min(3 if S is None else S, H)
    assert rel_err(got["out"][:, :take].cpu().numpy(), y64[:, Tin:Tin + take]) <= model_tol(
        rel_err(y32[:, Tin:Tin + take], y64[:, Tin:Tin + take]))


# ---- 8. graph replays -----------------------------------------------------------------
class _Log:
    def info(self, *a, **k):
        pass


@pytest.mark.parametrize("graphed", [True, False], ids=["graph", "eager"])
def test_every_replay_draws_a_fresh_mask(graphed):
    """The engine's step with learn.graph at lr = 0 on one batch, three times:
    with p = 0.1 three different losses (a replay that reused its captured
    seed would repeat one), none of them the p = 0 loss, which repeats."""
    from engine import PredictionEngine
    opts = dict(input_channels=6, input_time_frame=3, output_time_frame=3, st_gcnn_dropout=0.1,
                joints_to_consider=22, num_feature=16, num_layers=1, layout="h36m")
    cfg = dict(learn=dict(opt="adam", lr=0.0, weight_decay=0, gamma=0.9, step_size=5, graph=True),
               loss=dict(joint=["jl2", 1]), n_out=1, transform="tsc", use_weight=False, inverse=True)
    g = torch.Generator().manual_seed(81)
    seq = 0.6 * torch.randn(4, 6, 66, generator=g)
    inp, inv = seq.clone(), seq.flip(1).clone()
    inp[:, 3:], inv[:, 3:] = inp[:, 2:3], inv[:, 2:3]
    batch = (inp, inv, seq, seq)
    losses = {}
    for p in (0.1, 0.0):
        torch.manual_seed(82)
        m = get_model("dstdgcn", dstdgcn=opts).to(DEV).train()
        m.do_in.p = p
        eng = PredictionEngine(cfg, m, _Log())
        if not graphed:
            eng._graphed = lambda: False
        losses[p] = [eng.train([batch], e) for e in range(3)]
        assert (eng._graph_step is not None) == graphed
    assert len(set(losses[0.1])) == 3, losses
    assert len(set(losses[0.0])) == 1, losses
    assert losses[0.0][0] not in losses[0.1], losses
    assert all(np.isfinite(v) for v in losses[0.1])
