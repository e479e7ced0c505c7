"""The decode plan's row loop in both of its forms, against mi355q_mul_mat bit for bit.

A plan whose every GEMV stage has rows of whole 64-chunk steps (row_chunks % 64 == 0: every Llama K) runs the kernel without the per-lane
tail test; one stage with a partial last step puts the whole plan on the kernel with it, so the same whole-step stage is also checked there.
The loader moves from row to row of a wave by one 16-row stride of the current matrix and re-seeks only where a wave's next row lies in the
next matrix (q|k|v) -- or, in a PAIRED stage, alternates between the gate and up rows of a pair.  Covered: 1, 2, 7 and 14 steps per row,
rows with and without a chunk tail, several rows per wave, matrix boundaries inside a workgroup's range, mixed-type groups and paired stages
with odd pair counts, for every type of the {Q4_K, Q5_K, Q6_K, IQ4_XS, IQ4_NL} and {Q8_0, Q4_0} plan sets.
"""
import numpy as np
import pytest

import oracle
from qdata import quantized_weights

pytestmark = pytest.mark.gpu

# K per type: whole steps of 1, 2, 7 and 14 per row, then K with a partial last step (Q6_K rows are planar only when k % 2048 == 0: never a tail)
KS = {
    oracle.Q4_K: (2048, 4096, 14336, 28672, 2304, 768),
    oracle.Q5_K: (2048, 4096, 14336, 28672, 2304),
    oracle.Q6_K: (2048, 4096, 14336, 28672),
    oracle.IQ4_XS: (2048, 4096, 14336, 1024),
    oracle.IQ4_NL: (2048, 4096, 14336, 2304),
    oracle.Q8_0: (1024, 2048, 7168, 14336, 1280),
    oracle.Q4_0: (2048, 4096, 14336, 28672, 2304),
}
CASES = [(t, k) for t, ks in KS.items() for k in ks]


def case_id(v):
    return oracle.TYPE_NAMES[v] if isinstance(v, int) and v in (oracle.Q4_K, oracle.Q5_K, oracle.Q6_K, oracle.IQ4_XS, oracle.IQ4_NL, oracle.Q8_0, oracle.Q4_0) else str(v)


@pytest.fixture(scope="module")
def G():
    import torch
    import ggml_mi355 as g
    assert torch.cuda.is_available() and g.lib().mi355q_device_count() >= 1
    return g


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def W(G, t, m, k, rng):
    assert G.is_planar(t, k), (oracle.TYPE_NAMES[t], k)
    return G.QWeight.from_host(t, quantized_weights(t, m, k, rng, scale=0.5), m, k)


def z(torch, n):
    return torch.zeros((1, n), dtype=torch.float32, device="cuda")


def run_twice(G, torch, plan, outs, refs):
    for _ in range(2):
        for y in outs:
            y.zero_()
        plan.run(); torch.cuda.synchronize()
        assert plan.status() == 0
        for y, r in zip(outs, refs):
            assert np.array_equal(bits(y), bits(r))


@pytest.mark.parametrize("t,k", CASES, ids=case_id)
def test_one_matrix_every_step_count(G, torch, t, k):
    """4500 rows: 18 per workgroup, so waves 0 and 1 stream two rows each and the ring wraps from one row into the next at every step count."""
    rng = np.random.default_rng(7 * t + k)
    m = 4500
    w = W(G, t, m, k, rng)
    x = dev(torch, rng.standard_normal((1, k)).astype(np.float32))
    y = z(torch, m)
    plan = G.Plan([dict(ws=[w], ys=[y], x=x)])
    run_twice(G, torch, plan, [y], [G.mul_mat(w, x)])
    plan.close()


@pytest.mark.parametrize("t,k", [(oracle.Q4_K, 4096), (oracle.Q4_K, 2304), (oracle.Q6_K, 4096), (oracle.Q8_0, 2048), (oracle.Q8_0, 1280),
                                 (oracle.Q4_0, 2304), (oracle.IQ4_XS, 1024)],
                         ids=case_id)
def test_rows_cross_matrix_boundaries_inside_a_workgroup(G, torch, t, k):
    """q|k|v of one type, 2510 + 1705 + 901 rows: 20 rows per workgroup, so the boundaries fall inside workgroup ranges and waves 0-3 of those
    workgroups take their first row in one matrix and their second in the next (the loader re-seeks mid-stream)."""
    rng = np.random.default_rng(11 * t + k)
    ms = (2510, 1705, 901)
    ws = [W(G, t, m, k, rng) for m in ms]
    x = dev(torch, rng.standard_normal((1, k)).astype(np.float32))
    ys = [z(torch, m) for m in ms]
    plan = G.Plan([dict(ws=ws, ys=ys, x=x)])
    run_twice(G, torch, plan, ys, [G.mul_mat(w, x) for w in ws])
    plan.close()


@pytest.mark.parametrize("k", [4096, 2304], ids=str)
def test_mixed_type_group_with_and_without_tail(G, torch, k):
    """A group of K-quant types on one activation vector (rows crossing a matrix boundary inside workgroups of the Q4_K member)."""
    rng = np.random.default_rng(300 + k)
    types = [(oracle.Q4_K, 2510), (oracle.Q4_K, 1705), (oracle.Q5_K, 700)] + ([(oracle.Q6_K, 1031)] if k % 2048 == 0 else [])
    ws = [W(G, t, m, k, rng) for t, m in types]
    ys = [z(torch, m) for _, m in types]
    x = dev(torch, rng.standard_normal((1, k)).astype(np.float32))
    plan = G.Plan([dict(ws=ws, ys=ys, x=x)])
    run_twice(G, torch, plan, ys, [G.mul_mat(w, x) for w in ws])
    plan.close()


@pytest.mark.parametrize("t,k", [(oracle.Q4_K, 4096), (oracle.Q4_K, 2304), (oracle.Q6_K, 2048), (oracle.Q8_0, 1280), (oracle.Q4_0, 4096)],
                         ids=case_id)
@pytest.mark.parametrize("f", [1001, 4397], ids=str)
def test_paired_odd_pair_counts(G, torch, t, k, f):
    """gate|up as one PAIRED stage (SiLU(W_gate x) * (W_up x)), odd pair counts: 4 pairs per workgroup (1001) and 18 (4397: waves 0 and 1
    take two pairs -- the loader alternates gate and up rows and steps both matrices on by 16 rows), a ragged last workgroup either way."""
    rng = np.random.default_rng(500 + t + k + f)
    w_g, w_u = W(G, t, f, k, rng), W(G, t, f, k, rng)
    x = dev(torch, rng.standard_normal((1, k)).astype(np.float32))
    act, unused = z(torch, f), torch.full((1, f), 3.0, dtype=torch.float32, device="cuda")
    plan = G.Plan([dict(ws=[w_g, w_u], ys=[act, unused], x=x, y_kind=G.Y_UNARY_MUL, y_unary=G.UNARY_SILU)])
    ref = G.op_unary_mul(G.UNARY_SILU, G.mul_mat(w_g, x), G.mul_mat(w_u, x))
    run_twice(G, torch, plan, [act], [ref])
    assert bool((unused == 3.0).all())
    plan.close()


@pytest.mark.parametrize("t", [oracle.Q4_K, oracle.Q8_0], ids=lambda t: oracle.TYPE_NAMES[t])
def test_whole_step_stages_on_the_tail_kernel(G, torch, t):
    """x -> W1 (K = 4096, whole steps) -> W2 (K = 2304, a tail) -> W3 (K = 768, a tail): the tail stage puts the plan on the kernel with the
    per-lane test, which then also streams the whole-step stage; every output stays bit-identical to the node-by-node chain."""
    rng = np.random.default_rng(900 + t)
    w1, w2, w3 = W(G, t, 2304, 4096, rng), W(G, t, 768, 2304, rng), W(G, t, 4500, 768, rng)
    x = dev(torch, rng.standard_normal((1, 4096)).astype(np.float32))
    y1, y2, y3 = z(torch, 2304), z(torch, 768), z(torch, 4500)
    plan = G.Plan([dict(ws=[w1], ys=[y1], x=x), dict(ws=[w2], ys=[y2], x=y1), dict(ws=[w3], ys=[y3], x=y2)])
    r1 = G.mul_mat(w1, x); r2 = G.mul_mat(w2, r1); r3 = G.mul_mat(w3, r2)
    run_twice(G, torch, plan, [y1, y2, y3], [r1, r2, r3])
    plan.close()
