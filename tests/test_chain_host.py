"""The chain launches' acceptance rule (csrc/dstd_hilo.h "chain launches"), on
the host: enc_chain_append / model_chain_append take a block only if the
launch's arguments rebuild to exactly that block, so a member that no
descriptor carries cannot differ from the shared geometry unnoticed.

dstd_debug_chain_probe (csrc/dstd_capi.hip, not in the C ABI) builds the
blocks of a forward at B = 256 over made-up addresses as model_fwd does, flips
one 32-bit word of one block's BlockFusedArgs and runs the appends without a
launch: 0 accepted and the rebuild is the perturbed block, 1 refused, 2
accepted although the rebuild differs -- the silent bug, which must not exist
for any word of any block.  No GPU."""
import ctypes

import pytest

import dstd_native as native

SHAPES = [(35, 22), (35, 25), (40, 23)]  # the chain kernels' shapes (H36M, CMU, 3DPW)
LAYERS = 5
ENC_RUN, MODEL = 0, 1
ACCEPTED, REFUSED, SILENT = 0, 1, 2

# byte offsets, as csrc/dstd_hilo.h pins them (its static_asserts)
S, G, J, SN, S0 = 0, 216, 216 + 168, 216 + 392, 832  # BlockFusedArgs: s, t.g, t.j, t.sn, s0
SIZE = 1056
PQL = 80  # AdjHLArgs::pql
S_X, S_B = S + 0, S + 12
G_WIMG, G_PAD = G + 32, G + 68
J_PQL_ST, J_PQL_PAD, J_PAD = J + PQL + 12, J + PQL + 20, J + 220
SN_ALPHA, SN_OUT_SN, SN_PAD = SN + 168, SN + 200, SN + 220


def probe(tv, chain, block, offset, xor):
    f = native.lib().dstd_debug_chain_probe
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int] * 6 + [ctypes.c_uint]
    return f(tv[0], tv[1], LAYERS, chain, block, offset, xor)


def blocks(chain):
    """Model block indices of the chain: 0 conv_st_in, 1..L the encoders, L + 1 conv_st_out."""
    return range(1, LAYERS + 1) if chain == ENC_RUN else range(LAYERS + 2)


CHAINS = [pytest.param(ENC_RUN, id="enc_run"), pytest.param(MODEL, id="model")]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("tv", SHAPES)
def test_unperturbed_blocks_are_accepted(tv, chain):
    for b in blocks(chain):
        assert probe(tv, chain, b, 0, 0) == ACCEPTED


def test_probe_refuses_what_it_cannot_build():
    assert probe((35, 22), ENC_RUN, 0, 0, 0) == -1  # conv_st_in is in no run of encoder blocks
    assert probe((35, 22), MODEL, LAYERS + 2, 0, 0) == -1
    assert probe((35, 22), MODEL, 0, SIZE, 0) == -1
    assert probe((35, 22), MODEL, 0, 2, 0) == -1
    assert probe((75, 22), MODEL, 0, 0, 0) == -1  # no chain at T = 75


@pytest.mark.parametrize("xor", [1, 0x40000000])
@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("tv", SHAPES)
def test_no_word_of_any_block_is_accepted_with_a_different_rebuild(tv, chain, xor):
    seen = set()
    for b in blocks(chain):
        for off in range(0, SIZE, 4):
            r = probe(tv, chain, b, off, xor)
            assert r in (ACCEPTED, REFUSED), (b, off, r)
            seen.add(r)
    assert seen == {ACCEPTED, REFUSED}


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("tv", SHAPES)
def test_carried_words_pass_and_geometry_and_padding_words_are_refused(tv, chain):
    last = LAYERS + 1
    for b in blocks(chain):
        got = {name: probe(tv, chain, b, off, 1) for name, off in
               dict(s_x=S_X, g_wimg=G_WIMG, sn_alpha=SN_ALPHA, s_B=S_B, j_pql_st=J_PQL_ST, sn_out_sN=SN_OUT_SN,
                    g_pad=G_PAD, j_pql_pad=J_PQL_PAD, j_pad=J_PAD, sn_pad=SN_PAD).items()}
        # carried by the block's descriptor
        assert got["g_wimg"] == ACCEPTED, (b, got)
        # s.x is carried, but the kind check ties it to another member where the body
        # reads one buffer through both: an encoder block's residual (g.xres == s.x),
        # conv_st_in's model input (s0.xin == s.x); conv_st_out's is free
        assert got["s_x"] == (ACCEPTED if b == last else REFUSED), (b, got)
        # conv_st_out has no phase 3: its sn is all zero, whatever the member
        assert got["sn_alpha"] == (REFUSED if b == last else ACCEPTED), (b, got)
        # the shared geometry and the padding: in no descriptor
        for name in ("s_B", "j_pql_st", "sn_out_sN", "g_pad", "j_pql_pad", "j_pad", "sn_pad"):
            assert got[name] == REFUSED, (b, name, got)
