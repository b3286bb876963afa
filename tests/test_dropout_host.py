"""The host restatement of the do_in dropout mask (tests/dropout_helper.py)
and the masked oracle (oracle/dstdgcn_oracle.py ``drop=``), on the CPU.

The restatement is checked against plain Python integers, the threshold's
direction at the value itself, the oracle's ``drop`` against its absence, and
-- the reason tests/test_gpu_dropout.py can see a single wrong mask element --
how far one flipped element moves y and dx against their fp32 noise floor.
"""
import functools

import numpy as np
import pytest
import torch

import dropout_helper as D
from oracle import dstdgcn_oracle as O
from test_gpu_train import MAX_RATIO

SEEDS = [0, 11, 2 ** 62 - 1, 0xFFFFFFFF12345678]  # the last is above 2^63: seed * golden wraps


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("seed", SEEDS, ids=[hex(s) for s in SEEDS])
def test_keep_mask_is_the_scalar_restatement(seed, p):
    n = 1000
    u = D.uniforms_scalar(seed, n)
    assert np.array_equal(D.uniforms(seed, n), u)
    want = np.array([bool(v >= np.float32(p)) for v in u])
    got = D.keep_mask(seed, n, p)
    assert got.dtype == np.bool_ and np.array_equal(got, want)
    assert abs(got.mean() - (1 - p)) < 4 * np.sqrt(p * (1 - p) / n)  # four sigma of n Bernoulli draws
    assert float(D.keep_scale(p)) == float(np.float32(1) / (np.float32(1) - np.float32(p)))


def test_different_seeds_and_offsets_give_different_masks():
    a = D.keep_mask(11, 4096, 0.1)
    assert not np.array_equal(a, D.keep_mask(12, 4096, 0.1))
    assert not np.array_equal(a[:2048], a[2048:])  # the two halves of a paired call


@pytest.mark.parametrize("seed", SEEDS, ids=[hex(s) for s in SEEDS])
def test_threshold_keeps_at_equality(seed):
    """u >= p: at p = u[e0] element e0 is kept, at the next float32 it is
    dropped, and only elements whose u equals u[e0] change."""
    n = 5000
    u = D.uniforms(seed, n)
    e0 = int(np.abs(u - np.float32(0.1)).argmin())
    at = D.keep_mask(seed, n, u[e0])
    above = D.keep_mask(seed, n, np.nextafter(u[e0], np.float32(1)))
    assert at[e0] and not above[e0]
    same_u = u == u[e0]
    assert np.array_equal(at[~same_u], above[~same_u])
    assert at[same_u].all() and not above[same_u].any()


def _sd(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _case(name):
    m, B = (D.model_a(), 4) if name == "A" else (D.model_b(), 2)
    x, dy = D.step_inputs(m, B, 40 + B)
    return m, _sd(m), x, dy, (B, m.num_feature, x.shape[1], x.shape[2])


@pytest.mark.parametrize("name", ["A", "B"])
def test_all_true_mask_is_no_mask(name):
    m, sd, x, dy, shape = _case(name)
    P = {k: v.double() for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    ones = torch.ones(shape, dtype=torch.float64)
    for training in (False, True):
        y0 = O.dstdgcn_fn(x.double(), P, m.num_layers, training)
        assert torch.equal(O.dstdgcn_fn(x.double(), P, m.num_layers, training, drop=ones), y0)
        assert torch.equal(O.dstdgcn_fn(x.double(), P, m.num_layers, training, drop=None), y0)
    if name == "A":
        F = {k: v.double() for k, v in D.fast_state(sd, shape[3]).items() if not k.endswith("num_batches_tracked")}
        y0 = O.fast_dstdgcn_fn(x.double(), F, m.num_layers, True)
        assert torch.equal(O.fast_dstdgcn_fn(x.double(), F, m.num_layers, True, drop=ones.permute(0, 2, 3, 1)), y0)


def test_fast_state_is_the_same_function():
    """dropout_helper.fast_state: the channels-last oracle on the converted
    state dict is the base oracle, with and without a mask (fp64; the
    conversion rounds A_s * W_s + R_s to float32 once)."""
    m, sd, x, dy, shape = _case("A")
    drop = D.drop_tensor(11, shape, 0.1)
    base = D.oracle_step(sd, m.num_layers, [x], [dy], [drop])
    fast = D.oracle_step(D.fast_state(sd, shape[3]), m.num_layers, [x], [dy], [drop], fast=True)
    for k in ("y", "dx"):
        assert np.abs(fast[k] - base[k]).max() <= 1e-5 * np.abs(base[k]).max(), k
    nomask = D.oracle_step(sd, m.num_layers, [x], [dy], [None])
    assert np.abs(nomask["y"] - base["y"]).max() > 1e-2 * np.abs(base["y"]).max()


@pytest.mark.parametrize("name", ["A", "B"])
def test_one_flipped_mask_element_is_far_above_the_noise_floor(name):
    """Detection power of tests/test_gpu_dropout.py: with one element of the
    mask flipped (a kept one dropped or a dropped one kept), y and dx of the
    fp64 oracle move by more than MAX_RATIO times their fp32 noise floor --
    max(|fp32 oracle - fp64 oracle| with the same mask, 1e-4 of the tensor's
    max), the floor of test_gpu_train.noise_ratios.

    How far depends on the element: the flip changes h[0] there by |h| / (1 - p),
    and a PReLU output can be near zero.  Over twelve elements drawn with a
    fixed generator every flip must move dx past the bar (measured over forty:
    A 15x .. 2088x, B 32x .. 378x), and the median flip must move y past it
    (measured: A 3.4x .. 1438x, median 216x; B 2.8x .. 229x, median 65x -- on B
    five of forty elements move y by less than 6x, two by less than the bar, so
    y alone does not see every element; dx does)."""
    m, sd, x, dy, shape = _case(name)
    seed, p = 11, 0.1
    n = int(np.prod(shape))
    keep = D.keep_mask(seed, n, p)
    scale = float(D.keep_scale(p))
    drop = D.drop_tensor(seed, shape, p)
    r64 = D.oracle_step(sd, m.num_layers, [x], [dy], [drop])
    r32 = D.oracle_step(sd, m.num_layers, [x], [dy], [drop], dtype=torch.float32)
    floor = {k: max(float(np.abs(r32[k] - r64[k]).max()), 1e-4 * float(np.abs(r64[k]).max())) for k in ("y", "dx")}
    elements = np.random.default_rng(0).choice(n, 12, replace=False)
    assert keep[elements].any() and not keep[elements].all()  # both directions of a flip
    moved = {"y": [], "dx": []}
    for e in elements:
        flipped = drop.clone().reshape(-1)
        flipped[e] = 0.0 if keep[e] else scale
        got = D.oracle_step(sd, m.num_layers, [x], [dy], [flipped.reshape(shape)])
        for k in moved:
            moved[k].append(float(np.abs(got[k] - r64[k]).max()) / floor[k])
    for k, v in moved.items():
        print(f"model {name}: one flipped element moves {k} by {min(v):.1f} .. {max(v):.1f} x floor, "
              f"median {np.median(v):.1f}")
    assert min(moved["dx"]) > MAX_RATIO, moved["dx"]
    assert np.median(moved["y"]) > MAX_RATIO, moved["y"]


def test_fast_model_a_derives_model_a():
    """dropout_helper.fast_model_a: the channels-last module takes the converted
    state dict, and the shadow it derives from it -- the model whose kernels
    it runs -- holds model (A)'s tensors again (the spatial adjacency as
    A_s * W_s + R_s, rounded to float32 once)."""
    sd = _case("A")[1]
    fm, fsd = D.fast_model_a(0.1)
    assert set(fm.state_dict()) == set(fsd)
    sh = fm._shadow_for(torch.device("cpu"))
    fm._sync(sh)
    got = sh.state_dict()
    assert got.keys() == sd.keys()
    for k, v in sd.items():
        pre, leaf = k.rsplit(".", 1)
        if leaf in ("A_s", "W_s", "R_s"):
            adj = got[pre + ".A_s"] * got[pre + ".W_s"] + got[pre + ".R_s"]
            assert torch.equal(adj, sd[pre + ".A_s"] * sd[pre + ".W_s"] + sd[pre + ".R_s"]), k
        else:
            assert torch.equal(got[k], v), k
    assert sh.do_in.p == 0.1
