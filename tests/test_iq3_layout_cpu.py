"""The planar rule for all 19 weight types as the C table states it (csrc/mi355q_common.h), and the row sizes, which the planar layout must not
change (a planar row is the canonical row's bytes rearranged).

The Python side keeps no type table of its own: `ggml_mi355.is_planar` IS `mi355q_weights_are_planar`, so there is nothing to compare it with but
the rule restated here from the block layouts (`expected_planar`).  Only the IQ3_S and IQ3_XXS cases at K = 2048, 4096, 14336 tell this
layout from the one before it; the other types pin the table against a slip while it was being widened to five planes."""
import pytest

import oracle

TYPES = [oracle.Q4_0, oracle.Q4_1, oracle.Q5_0, oracle.Q5_1, oracle.Q8_0, oracle.Q2_K, oracle.Q3_K,
         oracle.Q4_K, oracle.Q5_K, oracle.Q6_K, oracle.IQ4_NL, oracle.IQ4_XS,
         oracle.IQ2_XXS, oracle.IQ2_XS, oracle.IQ2_S, oracle.IQ3_XXS, oracle.IQ3_S, oracle.IQ1_S, oracle.IQ1_M]
# (elements, bytes) per block: ggml-common.h
BLOCK = {oracle.Q4_0: (32, 18), oracle.Q4_1: (32, 20), oracle.Q5_0: (32, 22), oracle.Q5_1: (32, 24), oracle.Q8_0: (32, 34),
         oracle.Q2_K: (256, 84), oracle.Q3_K: (256, 110), oracle.Q4_K: (256, 144), oracle.Q5_K: (256, 176), oracle.Q6_K: (256, 210),
         oracle.IQ4_NL: (32, 18), oracle.IQ4_XS: (256, 136), oracle.IQ2_XXS: (256, 66), oracle.IQ2_XS: (256, 74), oracle.IQ2_S: (256, 82),
         oracle.IQ3_XXS: (256, 98), oracle.IQ3_S: (256, 110), oracle.IQ1_S: (256, 50), oracle.IQ1_M: (256, 56)}
# types with a streaming kernel, and the bytes of their planes in device order: planar iff the row and every plane start 16-byte aligned
PLANES = {oracle.Q4_0: (16, 2), oracle.Q8_0: (32, 2), oracle.Q4_K: (128, 16), oracle.Q5_K: (128, 32, 16), oracle.Q6_K: (128, 64, 16, 2),
          oracle.IQ4_NL: (16, 2), oracle.IQ4_XS: (128, 8), oracle.IQ3_XXS: (64, 32, 2), oracle.IQ3_S: (64, 32, 8, 4, 2)}
KS = (256, 2048, 4096, 14336)


@pytest.fixture(scope="module")
def G():
    import ggml_mi355 as g
    g.lib()
    return g


def expected_planar(t, k):
    if t not in PLANES:
        return False
    blck, bsize = BLOCK[t]
    nb = k // blck
    assert sum(PLANES[t]) == bsize
    off = 0
    for p in PLANES[t]:
        if off % 16:
            return False
        off += p * nb
    return (nb * bsize) % 16 == 0


@pytest.mark.parametrize("t", TYPES, ids=lambda t: oracle.TYPE_NAMES[t])
def test_planar_rule_all_types(G, t):
    for k in KS:
        assert G.is_planar(t, k) == expected_planar(t, k), (oracle.TYPE_NAMES[t], k)


def test_iq3_is_planar_at_every_llama_k(G):
    for t in (oracle.IQ3_S, oracle.IQ3_XXS):
        for k in (2048, 4096, 8192, 14336, 28672):
            assert G.is_planar(t, k)
        for k in (256, 512, 1024, 1792, 2304):
            assert not G.is_planar(t, k)


@pytest.mark.parametrize("t", TYPES, ids=lambda t: oracle.TYPE_NAMES[t])
def test_row_size_unchanged(G, t):
    blck, bsize = BLOCK[t]
    for k in KS:
        assert G.row_size(t, k) == k // blck * bsize
    assert G.row_size(t, blck + 1) == 0
