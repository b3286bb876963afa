"""Grouped evaluation on the MI355X (include/ext/dstd_gcn_eval.h,
PredictionEngine.test_groups): dstd_store_group_mpjpe against the metric the
project already has -- dstd_frame_mpjpe on the all_seqs dstd_batch_gather
writes, bit for bit -- against an fp64 numpy restatement (tests/eval_helper.py)
where groups split the batch, and test_groups against PredictionEngine.test run
once per group.

Shapes: J = 6, T = 6, N = 7 mirrored windows and B = 5 or 6 rows are the
smallest that hold every case (plain and mirrored windows, used / unused /
copied joints, frames before and after t_out0, rows of several groups in one
batch, a window twice); B * J = 30 or 36 elements leave most of the 256 threads
of a workgroup without work.  J = 32, T = 35, B = 3 is the shape of
tests/test_gpu_guards.py::test_frame_mpjpe: 96 elements, no multiple of the
workgroup, and B = 11 there (352 elements) gives some threads two.
"""
import numpy as np
import pytest
import torch

import data_helper as H
import dstd_native as native
import eval_helper as E
from conftest import group, load_npz
from dstd_data import DeviceLoader, DeviceSequences
from model import get_model
from test_gpu_guards import Bufs, _clones, _keep, _unchanged, run_fills
from test_gpu_model_chain import load_model
from test_gpu_train import rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 1e-5  # test_frame_mpjpe's: an fp32 sum of a few dozen O(1) norms carries a few ulp


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Case:
    """A resident set, a batch index, outputs and the metric's tables."""

    def __init__(self, J, T, N, used_joints, ignore, equal, frames, t_out0, index, mirror, seed, groups=None,
                 names=None):
        rng = np.random.default_rng(seed)
        D = 3 * J
        self.dim_used = np.sort(np.concatenate([3 * np.asarray(used_joints) + c for c in range(3)]))
        self.seqs = DeviceSequences.from_windows(rng.normal(size=(N, T, D)), self.dim_used, 2, T - 2, device=DEV,
                                                 mirror=mirror, groups=groups, group_names=names)
        self.store = H.store_of(self.seqs)
        self.T, self.D, self.t_out0, self.n_used = T, D, t_out0, len(self.dim_used)
        self.used_pos, self.joint_src = E.metric_tables(D, self.dim_used, ignore, equal)
        self.frames = np.asarray(frames, dtype=np.int32)
        self.index = np.asarray(index, dtype=np.int64)
        self.outs = rng.normal(size=(len(index), T - t_out0, self.n_used)).astype(np.float32)
        self.d_index, self.d_outs = _dev(self.index), _dev(self.outs)
        self.d_up, self.d_js, self.d_fr = _dev(self.used_pos), _dev(self.joint_src), _dev(self.frames)

    def inputs(self):
        s = self.seqs
        return [self.d_index, self.d_outs, self.d_up, self.d_js, self.d_fr, s._frames, s._starts, s._mirror_src] + (
            [s.groups] if s.groups is not None else [])

    def call(self, sums, counts, group="set", n_groups=None, rows=None, tables=None):
        """One dstd_store_group_mpjpe over the batch (or its first ``rows`` rows)."""
        g = self.seqs.groups if isinstance(group, str) else group
        up, js, fr = tables if tables is not None else (self.d_up, self.d_js, self.d_fr)
        code = native.lib().dstd_store_group_mpjpe(
            native.ext_eval.seq_store_ref(self.seqs._store), self.d_index.data_ptr(),
            len(self.index) if rows is None else rows, self.d_outs.data_ptr(), self.t_out0, up.data_ptr(), self.n_used,
            js.data_ptr(), fr.data_ptr(), len(self.frames), None if g is None else g.data_ptr(),
            self.seqs.n_groups if n_groups is None else n_groups, sums.data_ptr(), counts.data_ptr(),
            native.stream_handle(torch.device(DEV)))
        native.check(code, "dstd_store_group_mpjpe")

    def frame_mpjpe(self):
        """dstd_frame_mpjpe on the all_seqs dstd_batch_gather writes for the index."""
        all_seqs = self.seqs.gather(self.d_index, outputs=("all_seqs",))[3]
        sums = torch.zeros(len(self.frames), dtype=torch.float32, device=DEV)
        code = native.lib().dstd_frame_mpjpe(all_seqs.data_ptr(), self.d_outs.data_ptr(), len(self.index), self.T, self.D,
                                             self.t_out0, self.d_up.data_ptr(), self.n_used, self.d_js.data_ptr(),
                                             self.d_fr.data_ptr(), len(self.frames), sums.data_ptr(),
                                             native.stream_handle(torch.device(DEV)))
        native.check(code, "dstd_frame_mpjpe")
        return sums

    def reference(self, group, n_groups, index=None):
        return E.group_mpjpe_reference(self.store, self.index if index is None else index, self.outs, self.t_out0,
                                       self.used_pos, self.joint_src, self.frames, group, n_groups)


def _zeros(G, K):
    return torch.zeros(G, K, dtype=torch.float32, device=DEV), torch.zeros(G, dtype=torch.int32, device=DEV)


# four of six joints predicted, joint 0 copied from joint 1, joint 3 neither: pred = targ there
SMALL = dict(J=6, T=6, N=7, used_joints=[1, 2, 4, 5], ignore=[0], equal=[1], frames=[2, 3, 5], mirror=([1], [2]))
# the shape of tests/test_gpu_guards.py::test_frame_mpjpe
WIDE = dict(J=32, T=35, N=4, used_joints=[0, 1, 2, 3, 5, 6, 7, 8, 11, 12, 13, 14, 16, 17, 18, 20, 24, 25, 26, 27, 29, 30],
            ignore=[4, 31], equal=[0, 3], frames=[10, 11, 17, 33, 34], mirror=([1, 6], [2, 7]))


# ---- bit identity with the existing metric -------------------------------------------
@pytest.mark.parametrize("what,shape,t_out0,index", [
    ("small, t_out0 = 2", SMALL, 2, [3, 10, 0, 13, 6]),
    ("small, t_out0 = 0", SMALL, 0, [3, 10, 0, 13, 6]),
    ("wide, B * J = 96", WIDE, 10, [2, 5, 0]),
    ("wide, B * J = 352", WIDE, 10, [2, 5, 0, 7, 3, 3, 1, 4, 6, 0, 2]),
])
def test_one_group_is_frame_mpjpe_bit_for_bit(what, shape, t_out0, index):
    """group = NULL, n_groups = 1, every index valid: the sums are those of
    dstd_frame_mpjpe on the gathered all_seqs, torch.equal, plain and mirrored
    windows mixed, with frames before t_out0 (t_out0 = 2: none; the frames
    start at 2) and outputs that cover the whole window (t_out0 = 0)."""
    c = Case(**shape, t_out0=t_out0, index=index, seed=41)
    want = c.frame_mpjpe()
    sums, counts = _zeros(1, len(c.frames))
    c.call(sums, counts, group=None, n_groups=1)
    torch.cuda.synchronize()
    print(what, "frame_mpjpe", want.tolist(), "store_group_mpjpe", sums[0].tolist())
    assert float(want.abs().min()) > 0
    assert torch.equal(sums[0], want), what
    assert counts.tolist() == [len(index)]
    ref, _ = c.reference(None, 1)
    assert rel(sums, torch.from_numpy(ref)) < BAR


# ---- groups ------------------------------------------------------------------------
# group 1 is empty; group 2 holds window 4 alone (and its mirrored twin 11), which the index names twice
GROUPS = [0, 0, 0, 0, 2, 0, 0]
MIXED = [0, 4, 9, 4, 3, 12]  # rows of group 0, 2, 0 (window 2 mirrored), 2, 0, 0 (window 5 mirrored)


def test_groups_accumulate_per_group():
    """Three groups in one batch, rows interleaved, against the fp64
    restatement (1e-5, test_frame_mpjpe's bar), counts exact, the empty
    group's row exactly 0, and (+=) two calls give exactly twice one call's
    sums and counts (x + x is exact).  Outputs are bit-identical whatever the
    guard-banded buffers held around them (run_fills: no workspace, so this
    pins "no dependence on stale memory" for sums that start at 0).

    A group's row against the group = NULL call on that group's rows alone:
    the implementation does not guarantee bit equality (an element's thread
    is e = b * J + j of the whole batch, so taking rows out moves the others'
    elements to other threads and the sum to another order); the 1e-5 bar
    applies."""
    c = Case(**SMALL, t_out0=2, index=MIXED, seed=42, groups=GROUPS, names=["a", "b", "c"])
    K = len(c.frames)
    assert c.seqs.groups.tolist() == GROUPS * 2
    ref, ref_counts = c.reference(GROUPS * 2, 3)
    assert ref_counts.tolist() == [4, 0, 2]
    inputs = c.inputs()
    before = _clones(inputs)

    def call(fill):
        b = Bufs()
        one, two = b.f32("sums", (3, K), 0), b.f32("sums twice", (3, K), 0)
        n1 = b.new("counts", 4 * 3, 0).view(torch.int32, (3,))
        n2 = b.new("counts twice", 4 * 3, 0).view(torch.int32, (3,))
        c.call(one, n1)
        for _ in range(2):
            c.call(two, n2)
        b.check()
        return _keep({"sums": one, "twice": two, "counts": n1, "counts twice": n2})

    got = run_fills(call, "store_group_mpjpe")
    _unchanged(inputs, before, "store_group_mpjpe")
    print("sums", got["sums"].tolist(), "fp64", ref.tolist())
    assert rel(got["sums"], torch.from_numpy(ref)) < BAR
    for g in (0, 2):
        assert rel(got["sums"][g], torch.from_numpy(ref[g])) < BAR
    assert got["counts"].tolist() == [4, 0, 2]
    assert torch.equal(got["sums"][1], torch.zeros(K, device=DEV))
    assert torch.equal(got["twice"], 2 * got["sums"]) and got["counts twice"].tolist() == [8, 0, 4]
    # each group alone, as one group
    for g in (0, 2):
        rows = [b for b, w in enumerate(MIXED) if (GROUPS * 2)[w] == g]
        alone = Case(**SMALL, t_out0=2, index=[MIXED[b] for b in rows], seed=42)
        alone.d_outs = c.d_outs[rows].contiguous()
        sums, counts = _zeros(1, K)
        alone.call(sums, counts, group=None, n_groups=1)
        torch.cuda.synchronize()
        assert counts.tolist() == [len(rows)]
        assert rel(got["sums"][g], sums[0]) < BAR, g


def test_skipped_rows_are_not_summed_counted_or_read():
    """An index of -1, an index of 2N and a window whose group id is n_groups,
    after three valid rows: the sums are bit-equal to the call on the valid
    rows alone (the skipped rows add nothing to any thread's sum), within 1e-5
    of the restatement, and the counts leave them out.  Guard bands around
    sums and counts; the inputs are compared with clones afterwards."""
    N = SMALL["N"]
    c = Case(**SMALL, t_out0=2, index=[0, 9, 5, -1, 2 * N, 6], seed=43, groups=[0, 1, 1, 0, 0, 1, 0])
    table = c.seqs.groups.clone()
    assert table.numel() == 2 * N
    table[6] = 2  # = n_groups
    inputs = c.inputs() + [table]
    before = _clones(inputs)
    K = len(c.frames)
    b = Bufs()
    sums, valid = b.f32("sums", (2, K), 0), b.f32("sums of the valid rows", (2, K), 0)
    counts = b.new("counts", 8, 0).view(torch.int32, (2,))
    counts_valid = b.new("counts of the valid rows", 8, 0).view(torch.int32, (2,))
    c.call(sums, counts, group=table, n_groups=2)
    c.call(valid, counts_valid, group=table, n_groups=2, rows=3)
    b.check()
    _unchanged(inputs, before, "skipped rows")
    ref, ref_counts = c.reference(table.cpu().numpy(), 2)
    print("sums", sums.tolist(), "valid rows alone", valid.tolist(), "fp64", ref.tolist())
    assert ref_counts.tolist() == [1, 2] and counts.tolist() == [1, 2] and counts_valid.tolist() == [1, 2]
    assert torch.equal(sums, valid)
    assert rel(sums, torch.from_numpy(ref)) < BAR and float(sums.min()) > 0
    # every row skipped: nothing is written
    c.d_index = torch.tensor([-1, 2 * N, -7, 1 << 40, 6, 6], dtype=torch.int64, device=DEV)
    b2 = Bufs()
    s2 = b2.f32("sums", (2, K), 0)
    n2 = b2.new("counts", 8, 0).view(torch.int32, (2,))
    c.call(s2, n2, group=table, n_groups=2)
    b2.check()
    assert not s2.any() and not n2.any()


def test_table_entries_out_of_range_write_nothing():
    """A frame of T or -1 leaves its column as it was (the others are those of
    the valid call, bit for bit; the counts do not depend on the frames); a
    joint_src of J or a used_pos of n_used leaves every sum as it was.  Guard
    bands around the outputs."""
    c = Case(**SMALL, t_out0=2, index=MIXED, seed=44, groups=GROUPS, names=["a", "b", "c"])
    K = len(c.frames)
    good, good_counts = _zeros(3, K)
    c.call(good, good_counts)
    b = Bufs()
    fr = _dev(np.array([c.T, 3, -1], dtype=np.int32))
    sums = b.f32("sums", (3, K), 0)
    counts = b.new("counts", 12, 0).view(torch.int32, (3,))
    c.call(sums, counts, tables=(c.d_up, c.d_js, fr))
    js = c.d_js.clone()
    js[2] = SMALL["J"]
    up = c.d_up.clone()
    up[int(c.dim_used[-1])] = c.n_used
    untouched = [b.f32(f"sums {i}", (3, K), 0) for i in range(2)]
    n = [b.new(f"counts {i}", 12, 0).view(torch.int32, (3,)) for i in range(2)]
    c.call(untouched[0], n[0], tables=(c.d_up, js, c.d_fr))
    c.call(untouched[1], n[1], tables=(up, c.d_js, c.d_fr))
    b.check()
    assert torch.equal(sums[:, 1], good[:, 1]) and not sums[:, 0].any() and not sums[:, 2].any()
    assert counts.tolist() == good_counts.tolist() == [4, 0, 2]
    for s, k in zip(untouched, n):
        assert not s.any() and k.tolist() == [4, 0, 2]
    assert H.hip_last_error() == 0


# ---- the engine ---------------------------------------------------------------------
class _Log:
    def info(self, *a, **k):
        pass


CFG = dict(learn=dict(opt="adam", lr=3e-3, weight_decay=0, gamma=0.9, step_size=5), loss=dict(joint=["jl2", 1]),
           n_out=1, transform="tsc", use_weight=False, inverse=True)
SIZES = (3, 1, 4)
_engine = {}


def engine_case():
    """The H36M model with the state dict of engine.npz (test/sd/), a resident
    set of 8 windows (the fixture's 4 and 4 copies scaled by 1.01) in groups of
    3, 1 and 4, and PredictionEngine.test per group (its own resident set,
    batch_size = 2): computed once, not to be changed."""
    if not _engine:
        from engine import PredictionEngine
        d = load_npz("engine.npz")
        opts = dict(input_channels=6, input_time_frame=10, output_time_frame=25, st_gcnn_dropout=0.1,
                    joints_to_consider=22, num_feature=64, num_layers=5, layout="h36m")
        m = get_model("dstdgcn", dstdgcn=opts)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in group(d, "test/sd/").items()})
        eng = PredictionEngine(CFG, m.to(DEV), _Log())
        x = d["test/all_seqs"].astype(np.float64)
        x = np.concatenate([x, 1.01 * x])
        groups = np.repeat(np.arange(3), SIZES)
        names = ["walking", "eating", "smoking"]
        kw = dict(eval_frame=list(d["test/eval_frame"]), joint_to_ignore=d["test/joint_to_ignore"],
                  joint_equal=d["test/joint_equal"])
        seqs = DeviceSequences.from_windows(x, d["test/dim_used"], 10, 25, device=DEV, groups=groups, group_names=names)
        per_group = {}
        for g, name in enumerate(names):
            alone = DeviceSequences.from_windows(x[groups == g], d["test/dim_used"], 10, 25, device=DEV)
            per_group[name] = eng.test(DeviceLoader(alone, 2), input_n=10, dim_used=d["test/dim_used"], **kw)
        _engine.update(eng=eng, seqs=seqs, kw=kw, per_group=per_group, names=names, d=d)
    return _engine


def _check_engine_table(got, c):
    avg, t_metric, table = got
    assert list(table) == c["names"]
    for name in c["names"]:
        avg_g, met_g = table[name]
        want_avg, want = c["per_group"][name]
        print(name, "test_groups", met_g, "test", want)
        assert met_g.shape == want.shape and (np.abs(met_g - want) <= BAR * np.abs(want)).all(), name
        assert abs(avg_g - want_avg) <= BAR * want_avg and abs(avg_g - met_g.mean()) <= 1e-12 * avg_g
    mean = np.mean([c["per_group"][n][1] for n in c["names"]], axis=0)
    assert (np.abs(t_metric - mean) <= BAR * mean).all()
    assert abs(avg - np.mean([c["per_group"][n][0] for n in c["names"]])) <= BAR * avg
    assert np.allclose(t_metric, np.mean([table[n][1] for n in c["names"]], axis=0), rtol=1e-12, atol=0)
    assert abs(avg - t_metric.mean()) <= 1e-12 * avg


def test_engine_table_is_test_per_group():
    """test_groups over DeviceLoader(batch_size=3) -- batches straddle the
    groups of 3, 1 and 4 windows and the last one is ragged -- against
    PredictionEngine.test on each group's windows alone, within 1e-5: the
    forwards are sample-independent bit for bit, only the summation order
    differs.  The first two return values are the mean over the three groups.

    The fixture's test/metric is the mean over its four windows, not a
    per-window figure, so the group of one (window 3) cannot be compared with
    it alone; groups 0 and 1 together are those four windows, and their
    count-weighted mean meets test/metric at the 2e-4 of
    tests/test_gpu_train.py::test_engine_test_metric_matches_reference."""
    c = engine_case()
    loader = DeviceLoader(c["seqs"], 3)
    assert len(loader) == 3 and len(c["seqs"]) % 3 != 0
    got = c["eng"].test_groups(loader, input_n=10, **c["kw"])
    _check_engine_table(got, c)
    table, ref = got[2], c["d"]["test/metric"]
    four = (3 * table["walking"][1] + table["eating"][1]) / 4
    assert np.abs(four - ref).max() / np.abs(ref).max() < 2e-4
    # a set without groups is one group named "all": the whole loader's metric
    plain = DeviceSequences.from_windows(c["d"]["test/all_seqs"], c["d"]["test/dim_used"], 10, 25, device=DEV)
    avg, t_metric, table = c["eng"].test_groups(DeviceLoader(plain, 3), input_n=10, **c["kw"])
    assert list(table) == ["all"] and np.array_equal(table["all"][1], t_metric) and table["all"][0] == avg
    assert np.abs(t_metric - ref).max() / np.abs(ref).max() < 2e-4


def test_engine_refusals_leave_the_valid_call_as_it_was():
    c = engine_case()
    eng, kw = c["eng"], c["kw"]
    loader = DeviceLoader(c["seqs"], 3)
    first = eng.test_groups(loader, input_n=10, **kw)

    def still_valid():
        got = eng.test_groups(loader, input_n=10, **kw)
        _check_engine_table(got, c)
        assert np.array_equal(got[1], first[1]) and got[0] == first[0]  # and bit-reproducible

    with pytest.raises(TypeError, match="DeviceLoader"):
        eng.test_groups([t for t in loader], input_n=10, **kw)
    still_valid()
    with pytest.raises(ValueError, match="frames"):  # windows of 35 frames, not 10 + 30
        eng.test_groups(loader, input_n=10, horizon=30, **kw)
    still_valid()
    for bad in ([1, 25], [-11]):
        with pytest.raises(ValueError, match="eval frame"):
            eng.test_groups(loader, input_n=10, **dict(kw, eval_frame=bad))
    still_valid()


def test_engine_channels_last_model_goes_through_the_same_call():
    """model/dstdgcn_fast.py in the engine: test_groups against test per group
    on the fixture's four windows in two interleaved groups, within 1e-5."""
    from engine import PredictionEngine
    from model import dstdgcn_fast as F
    d, e = load_npz("dstdgcn_fast.npz"), load_npz("engine.npz")
    p = "model_h36m/"
    m = F.DSTDGCN(**{k[len(p + "opt/"):]: d[k].item() for k in d.files if k.startswith(p + "opt/")})
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in group(d, p + "sd/").items()})
    eng = PredictionEngine(CFG, m.to(DEV).eval(), _Log())
    x, groups = e["test/all_seqs"].astype(np.float64), np.array([0, 1, 1, 0])
    kw = dict(eval_frame=list(e["test/eval_frame"]), joint_to_ignore=e["test/joint_to_ignore"],
              joint_equal=e["test/joint_equal"])
    seqs = DeviceSequences.from_windows(x, e["test/dim_used"], 10, 25, device=DEV, groups=groups)
    avg, t_metric, table = eng.test_groups(DeviceLoader(seqs, 3), input_n=10, **kw)
    for g in (0, 1):
        alone = DeviceSequences.from_windows(x[groups == g], e["test/dim_used"], 10, 25, device=DEV)
        want_avg, want = eng.test(DeviceLoader(alone, 2), input_n=10, dim_used=e["test/dim_used"], **kw)
        print("group", g, "test_groups", table[str(g)][1], "test", want)
        assert (want > 0).all() and (np.abs(table[str(g)][1] - want) <= BAR * want).all()
        assert abs(table[str(g)][0] - want_avg) <= BAR * want_avg
    assert np.allclose(t_metric, (table["0"][1] + table["1"][1]) / 2, rtol=1e-12, atol=0)


def test_engine_horizon_per_group():
    """Windows of 10 + 50 frames in two groups: test_groups(horizon=50) against
    test(horizon=50) on each group's windows alone, within 1e-5, eval frames in
    both windows of the rollout and at their boundary."""
    from engine import PredictionEngine
    d = load_npz("engine.npz")
    m, _ = load_model("h36m")
    eng = PredictionEngine(CFG, m, _Log())
    x = 0.5 * np.random.default_rng(45).normal(size=(5, 60, 96))
    groups = np.array([0, 1, 0, 1, 1])
    kw = dict(eval_frame=[0, 24, 25, 49], joint_to_ignore=d["test/joint_to_ignore"], joint_equal=d["test/joint_equal"])
    seqs = DeviceSequences.from_windows(x, d["test/dim_used"], 10, 50, device=DEV, groups=groups)
    avg, t_metric, table = eng.test_groups(DeviceLoader(seqs, 2), input_n=10, horizon=50, **kw)
    assert list(table) == ["0", "1"]
    for g in (0, 1):
        alone = DeviceSequences.from_windows(x[groups == g], d["test/dim_used"], 10, 50, device=DEV)
        want_avg, want = eng.test(DeviceLoader(alone, 2), input_n=10, dim_used=d["test/dim_used"], horizon=50, **kw)
        avg_g, met_g = table[str(g)]
        print("group", g, "test_groups", met_g, "test", want)
        assert np.isfinite(want).all() and (want > 0).all()
        assert (np.abs(met_g - want) <= BAR * np.abs(want)).all() and abs(avg_g - want_avg) <= BAR * want_avg
    assert np.allclose(t_metric, (table["0"][1] + table["1"][1]) / 2, rtol=1e-12, atol=0)
    assert abs(avg - t_metric.mean()) <= 1e-12 * avg
    with pytest.raises(ValueError, match="frames"):
        eng.test_groups(DeviceLoader(seqs, 2), input_n=10, horizon=25, **kw)
