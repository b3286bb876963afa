"""The envelope case table (tests/envelope_cases.py) is honest: on every case
the fp32 oracle's own error against the fp64 oracle, on every tensor the GPU
test compares and under the same normalisation, is at most half of the bar
the GPU test applies (5e-5 for ops and eval-mode blocks, 1e-4 for train-mode
blocks) -- a case whose reference arithmetic alone could not hold the bar
would test conditioning, not the kernel.  And the table's coverage claims
that are pure arithmetic hold, so that an edit cannot silently drop a branch.
"""
import pytest
import torch

import envelope_cases as E


@pytest.mark.parametrize("c", E.OP_CASES, ids=E.case_id)
def test_op_case_is_well_conditioned(c):
    built = E.build_op(c)
    errs = E.op_errors(E.op_reference(c, torch.float32, built), E.op_reference(c, torch.float64, built))
    worst = max(errs, key=errs.get)
    print(f"{E.case_id(c)}: worst fp32-oracle error {errs[worst]:.2e} ({worst})")
    assert errs[worst] <= E.OP_BAR / 2, (worst, errs[worst])


@pytest.mark.parametrize("c", E.BLOCK_EVAL_CASES, ids=E.case_id)
def test_block_eval_case_is_well_conditioned(c):
    built = E.build_block_eval(c)
    err = E.rel(E.block_eval_reference(c, torch.float32, built), E.block_eval_reference(c, torch.float64, built))
    print(f"{E.case_id(c)}: fp32-oracle error {err:.2e}")
    assert err <= E.BLOCK_EVAL_BAR / 2


@pytest.mark.parametrize("c", E.BLOCK_TRAIN_CASES + E.BN_APPLY_CASES, ids=E.case_id)
def test_block_train_case_is_well_conditioned(c):
    built = E.build_block_train(c)
    r32, r64 = E.block_train_reference(c, torch.float32, built), E.block_train_reference(c, torch.float64, built)
    errs = E.block_train_errors(r32, r64)
    worst = max(errs, key=errs.get)
    print(f"{E.case_id(c)}: worst fp32-oracle error {errs[worst]:.2e} ({worst})")
    assert errs[worst] <= E.BLOCK_TRAIN_BAR / 2, (worst, errs[worst])
    # the batch statistics the running-statistics check (bar 1e-5) is built from
    for (m32, v32), (m64, v64) in zip(r32["stats"], r64["stats"]):
        assert E.rel(m32, m64) <= 5e-6 and E.rel(v32, v64) <= 5e-6


def test_bn_apply_cases_take_their_paths():
    """The launch choice of both BatchNorms (C = 64) of each BN_APPLY_CASES
    block, by arithmetic, is the one the GPU test expects the library to
    report; no case reaches the flat path's 2^24 elements."""
    assert len(set(E.BN_APPLY_CASES)) == 5 and not set(E.BN_APPLY_CASES) & set(E.BLOCK_TRAIN_CASES)
    for c in E.BN_APPLY_CASES:
        assert c.cout == 64 and E.bn_path(c.B, c.cout, c.T, c.V) == E.BN_APPLY_EXPECT[c], c
    assert {E.BN_APPLY_EXPECT[c][:2] for c in E.BN_APPLY_CASES} == {(E.BN_MERGED_VEC, 2), (E.BN_MERGED_VEC, 4),
                                                                    (E.BN_MERGED_SCALAR, 2), (E.BN_MERGED_SCALAR, 4)}
    # the paired B=256 3DPW model step of tests/test_gpu_train.py (two groups of 256) is what runs the flat path
    assert E.bn_path(512, 64, 40, 23, groups=2) == (E.BN_FLAT, 0, 16) and E.bn_path(256, 64, 40, 23)[0] != E.BN_FLAT
    assert E.bn_path(4, 64, 35, 22) == (E.BN_MERGED_SCALAR, 1, 3) and E.bn_path(8, 64, 40, 23) == (E.BN_MERGED_VEC, 1, 5)


def test_builders_are_deterministic():
    c = E.OP_CASES[5]
    a, b = E.build_op(c), E.build_op(c)
    assert all(torch.equal(p, q) for p, q in zip(a[0].state_dict().values(), b[0].state_dict().values()))
    assert all(torch.equal(p, q) for p, q in zip(a[1:], b[1:]))
    assert len({E.case_seed(c) for c in E.OP_CASES}) == len(E.OP_CASES)


def test_cases_are_inside_the_envelope_and_tiny():
    assert len(set(E.OP_CASES)) == len(E.OP_CASES) >= 60
    for c in E.OP_CASES:
        assert c.mode in ("spatial", "temporal") and E.WHY[c]
        assert 1 <= c.B <= 3 and 2 <= c.T <= 128 and 1 <= c.V <= 32
        assert 1 <= c.cin <= 64 and 1 <= c.cout <= 64 and 1 <= c.red <= 8
    for c in E.BLOCK_EVAL_CASES + E.BLOCK_TRAIN_CASES:
        assert 1 <= c.B <= 4 and 2 <= c.T <= 128 and (c.T, c.V) not in ((35, 22), (35, 25), (40, 23), (75, 22))


S, T_ = "spatial", "temporal"
COVERAGE = {
    # aggregation slab kernels: column fragments JF = cdiv(NN, 16), pad = NN % 4
    "JF=1 spatial": lambda c: c.mode == S and E.cdiv(c.V, 16) == 1,
    "JF=1 temporal": lambda c: c.mode == T_ and E.cdiv(c.T, 16) == 1,
    "JF=4 temporal": lambda c: c.mode == T_ and E.cdiv(c.T, 16) == 4,
    "JF=4 temporal with pad": lambda c: c.mode == T_ and E.cdiv(c.T, 16) == 4 and c.T % 4,
    "no-pad NN spatial": lambda c: c.mode == S and c.V % 4 == 0,
    "no-pad NN temporal, slab": lambda c: c.mode == T_ and c.T % 4 == 0 and c.T <= 64,
    "V % 4 == 0 at odd T (vector path)": lambda c: c.V % 4 == 0 and c.T % 2 == 1,
    "NN in {16, 32, 48, 64}": lambda c: E.nn_of(c) in (16, 32, 48, 64),
    "temporal backward on the channel-chunk kernel at JF=4": lambda c: (c.mode == T_ and 49 <= c.T <= 64
                                                                        and not E.temporal_bwd_two_launch(c)),
    "two-launch temporal backward": lambda c: E.temporal_bwd_two_launch(c) and c.cout % 4 == 0,
    "two-launch temporal backward, channel tail": lambda c: E.temporal_bwd_two_launch(c) and c.cout % 4 != 0,
    "two-launch temporal backward, cout < 4": lambda c: E.temporal_bwd_two_launch(c) and c.cout < 4,
    # the agg_ok cliff
    "temporal T=64": lambda c: c.mode == T_ and c.T == 64,
    "temporal T=65": lambda c: c.mode == T_ and c.T == 65,
    # streaming conv GEMM
    "cout + 2 red > 68 (KS=20)": lambda c: 68 < c.cout + 2 * c.red <= 80,
    "cout + 2 red == 80 (kCsMax)": lambda c: c.cout + 2 * c.red == 80,
    "T*V < 16 spatial": lambda c: c.mode == S and c.T * c.V < 16,
    "T*V < 16 temporal": lambda c: c.mode == T_ and c.T * c.V < 16,
    "M=1": lambda c: c.cout == 1,
    # eval adjacency row tiles
    "k_adj RT=4 single group": lambda c: c.mode == S and 49 <= c.T <= 64,
    "k_adj T=112": lambda c: c.mode == S and c.T == 112,
    "k_adj T=113": lambda c: c.mode == S and c.T == 113,
    "k_adj RT=8 small V": lambda c: c.mode == S and c.T >= 113 and c.V <= 8,
    "k_adj T=128 V=9": lambda c: c.mode == S and c.T == 128 and c.V == 9,
    # eval GC kernels
    "ks_for(cin)=4": lambda c: 9 <= c.cin <= 16 and c.red == 2,
    "cout < 16, not 3": lambda c: c.cout < 16 and c.cout != 3 and c.red == 2,
    "V == 32 spatial": lambda c: c.mode == S and c.V == 32,
    "V == 32 temporal": lambda c: c.mode == T_ and c.V == 32,
    "V == 1 spatial": lambda c: c.mode == S and c.V == 1,
    "V == 1 temporal": lambda c: c.mode == T_ and c.V == 1,
    # k_temporal_wave: compile-time T, runtime V
    "temporal wave V=32": lambda c: c.mode == T_ and (c.cin, c.cout) == (64, 64) and c.T in (35, 40, 75) and c.V == 32,
    "temporal wave one unit": lambda c: (c.mode == T_ and (c.cin, c.cout) == (64, 64) and c.T in (35, 40, 75)
                                         and c.B * c.V == 1),
    "temporal 3->3 V=32": lambda c: c.mode == T_ and (c.cin, c.cout, c.T, c.V) == (3, 3, 35, 32),
    # transposes and small tensors
    "cin=1": lambda c: c.cin == 1,
    "T*V < 32": lambda c: c.T * c.V < 32,
    "NN=1": lambda c: E.nn_of(c) == 1,
    "NN=2": lambda c: E.nn_of(c) == 2,
    # corners
    "corner (128, 32) at 64 channels": lambda c: (c.cin, c.cout, c.T, c.V) == (64, 64, 128, 32),
    "corner (2, 1) at 1 channel": lambda c: (c.cin, c.cout, c.T, c.V) == (1, 1, 2, 1),
}


@pytest.mark.parametrize("name", list(COVERAGE))
def test_table_covers(name):
    assert any(COVERAGE[name](c) for c in E.OP_CASES), name


def test_table_holds_the_required_cases():
    have = set(E.OP_CASES)

    def has(**kw):
        return any(all(getattr(c, k) == v for k, v in kw.items()) for c in have)

    for mode in (S, T_):
        for T, V in ((2, 1), (2, 32), (128, 1), (128, 32)):
            for ch in (64, 1):
                assert has(mode=mode, cin=ch, cout=ch, T=T, V=V)
        for cin, cout in ((1, 1), (4, 5), (9, 16), (13, 17), (16, 15), (63, 1), (64, 63)):
            assert has(mode=mode, cin=cin, cout=cout)
        for red in (3, 8):
            for cin in (64, 20):
                assert has(mode=mode, cin=cin, cout=64, T=35, V=22, red=red)
        for T, V in ((3, 2), (2, 5)):
            assert has(mode=mode, T=T, V=V)
    for V in (15, 16, 17, 31, 32):
        assert has(mode=S, T=20, V=V)
    for T in (15, 16, 17, 48, 49, 63, 64, 65):
        for V in (5, 16):
            assert has(mode=T_, T=T, V=V)
    for T in (48, 64, 65, 112, 113, 127):
        assert has(mode=S, T=T, V=22)
    for T in (120, 128):
        for V in (4, 8, 9):
            assert has(mode=S, T=T, V=V)
    for T in (35, 40, 75):
        for V in (1, 32):
            for B in (1, 2):
                assert has(mode=T_, cin=64, cout=64, T=T, V=V, B=B)
    assert has(mode=T_, cin=3, cout=3, T=35, V=32)
    assert {c.T for c in E.BLOCK_EVAL_CASES} == {c.T for c in E.BLOCK_TRAIN_CASES} == {2, 16, 17, 64, 65, 113}
    assert {c.B for c in E.BLOCK_TRAIN_CASES} == {1, 4} and {c.B for c in E.BLOCK_EVAL_CASES} == {2}
    assert {(c.cin, c.cout, c.layout) for c in E.BLOCK_EVAL_CASES} == {(64, 64, "h36m"), (6, 64, "cmu"),
                                                                       (64, 3, "3dpw")}
