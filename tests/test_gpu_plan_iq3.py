"""IQ3_S and IQ3_XXS in the decode plan (regs engine): every output of a planned stage is bit-identical to mi355q_mul_mat on the same activation
vector -- the header's contract -- for the kernel set of the IQ3 recipes {IQ3_S, IQ3_XXS, Q4_K, Q5_K, Q6_K}.

Shapes.  A streaming step of these types is 2048 elements, so K = 2048 is one step per row and K = 6144 three: the ring of 8 slots then holds
rows of several and of one row at a time.  A plan runs one workgroup of 16 waves per CU; 96 + 32 rows are fewer than one row per workgroup (a
wave takes 0 or 1 row), 4500 rows and 6144 pairs are more than 16 per workgroup (waves take several).  The first stage of the two-stage plan
carries a third matrix of K rows beside the two small ones: its output is the only vector of a plannable length (a multiple of 2048) for the
IQ3_XXS stage behind it.  Large matrices are a few quantized rows repeated: bit-identity does not care, quantizing does (seconds per 1000 rows).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import PKG, ROOT
from qdata import quantized_weights

pytestmark = pytest.mark.gpu

IQ3 = [oracle.IQ3_S, oracle.IQ3_XXS]
ids_t = lambda t: oracle.TYPE_NAMES[t]
EPS = 1e-5


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
    assert G.is_planar(t, k), (ids_t(t), k)
    base = quantized_weights(t, min(m, 64), k, rng, scale=0.5)
    rows = np.concatenate([base] * ((m + 63) // 64))[:m] if m > 64 else base
    return G.QWeight.from_host(t, rows, m, k)


def z(torch, n):
    return torch.zeros((1, n), dtype=torch.float32, device="cuda")


def run_and_compare(torch, plan, outs, refs, times=2):
    for _ in range(times):
        for y in outs:
            y.zero_()
        plan.run(); torch.cuda.synchronize()
        assert plan.status() == 0
        for i, (y, r) in enumerate(zip(outs, refs)):
            assert np.array_equal(bits(y), bits(r)), f"output {i}"


def two_stage(G, torch, K, wrap=False):
    """X_NORM -> {IQ3_S 96, Q6_K 32, IQ3_S K} as a mixed-type group, then X_PLAIN on the K-row output -> IQ3_XXS 130."""
    rng = np.random.default_rng(3000 + K)
    w_a, w_b, w_c, w_d = W(G, oracle.IQ3_S, 96, K, rng), W(G, oracle.Q6_K, 32, K, rng), W(G, oracle.IQ3_S, K, K, rng), W(G, oracle.IQ3_XXS, 130, K, rng)
    h = dev(torch, rng.standard_normal((1, K)).astype(np.float32))
    nw = dev(torch, (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32))
    ya, yb, yc, yd = z(torch, 96), z(torch, 32), z(torch, K), z(torch, 130)
    plan = G.Plan([dict(ws=[w_a, w_b, w_c], ys=[ya, yb, yc], x=h, x_kind=G.X_NORM, norm_w=nw, eps=EPS),
                   dict(ws=[w_d], ys=[yd], x=yc)])
    try:
        x1 = G.op_add_rms_norm_mul(h, EPS, weight=nw)
        ra, rb, rc = G.mul_mat(w_a, x1), G.mul_mat(w_b, x1), G.mul_mat(w_c, x1)
        refs = [ra, rb, rc, G.mul_mat(w_d, rc)]
        assert float(refs[3].abs().max()) > 0.0
        run_and_compare(torch, plan, [ya, yb, yc, yd], refs)
        if wrap:                                                 # the run counter just below the 32-bit epoch wrap: the runs on both sides of the granule reset
            plan.debug_set_runs(0xFFFFFFFF // (plan.launch_stages + 1) - 2)
            run_and_compare(torch, plan, [ya, yb, yc, yd], refs, times=4)
    finally:
        plan.close()


@pytest.mark.parametrize("K", [2048, 6144], ids=str)
def test_two_stage_plan_is_bit_identical_to_mul_mat(G, torch, K):
    two_stage(G, torch, K, wrap=K == 2048)


@pytest.mark.parametrize("f", [2048, 6144], ids=str)
def test_paired_stage_then_down(G, torch, f):
    """gate | up of IQ3_S as one PAIRED (Y_UNARY_MUL) stage, then the IQ3_XXS down matrix on its output: 8 pairs per workgroup (f = 2048: half the
    waves take none) and 24 (f = 6144: waves 0-7 take two)."""
    rng = np.random.default_rng(4000 + f)
    K = 2048
    w_g, w_u, w_d = W(G, oracle.IQ3_S, f, K, rng), W(G, oracle.IQ3_S, f, K, rng), W(G, oracle.IQ3_XXS, 300, f, rng)
    x = dev(torch, rng.standard_normal((1, K)).astype(np.float32))
    act, unused, down = z(torch, f), torch.full((1, f), 3.0, dtype=torch.float32, device="cuda"), z(torch, 300)
    plan = G.Plan([dict(ws=[w_g, w_u], ys=[act, unused], x=x, y_kind=G.Y_UNARY_MUL, y_unary=G.UNARY_SILU),
                   dict(ws=[w_d], ys=[down], x=act)])
    try:
        r_act = G.op_unary_mul(G.UNARY_SILU, G.mul_mat(w_g, x), G.mul_mat(w_u, x))
        run_and_compare(torch, plan, [act, down], [r_act, G.mul_mat(w_d, r_act)])
        assert bool((unused == 3.0).all())
    finally:
        plan.close()


@pytest.mark.parametrize("t", IQ3, ids=ids_t)
@pytest.mark.parametrize("x_kind", ["plain", "norm_sum", "unary_mul"])
def test_several_rows_per_wave_every_x_kind(G, torch, t, x_kind):
    """4500 rows: 18 per workgroup, so waves 0 and 1 stream two rows each through one ring; the activation vector in each of its three forms."""
    rng = np.random.default_rng(5000 + 10 * t + len(x_kind))
    K, m = 2048, 4500
    w = W(G, t, m, K, rng)
    x0, x1 = (dev(torch, rng.standard_normal((1, K)).astype(np.float32)) for _ in range(2))
    nw = dev(torch, (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32))
    y, s, xo = z(torch, m), z(torch, K), z(torch, K)
    if x_kind == "plain":
        stage = dict(ws=[w], ys=[y], x=x0)
    elif x_kind == "norm_sum":
        stage = dict(ws=[w], ys=[y], x=x0, x1=x1, x_kind=G.X_NORM, norm_w=nw, eps=EPS, sum_out=s, x_out=xo)
    else:
        stage = dict(ws=[w], ys=[y], x=x0, x1=x1, x_kind=G.X_UNARY_MUL, unary=G.UNARY_SILU)
    plan = G.Plan([stage])
    try:
        if x_kind == "plain":
            outs, refs = [y], [G.mul_mat(w, x0)]
        elif x_kind == "norm_sum":
            # the sum of squares is an f64 reduction whose order is the engine's: the formed vector is taken from the plan itself (x_out), held to
            # the node op's within one ulp-scale bound, and the rows are compared with mul_mat on exactly that vector
            plan.run(); torch.cuda.synchronize()
            assert plan.status() == 0
            xr = xo.clone()
            r_x, r_sum = G.op_add_rms_norm_mul(x0, EPS, b=x1, weight=nw, want_sum=True)
            assert float((xr - r_x).abs().max()) <= 2.0 ** -22 * float(r_x.abs().max())
            outs, refs = [y, s, xo], [G.mul_mat(w, xr), r_sum, xr]
        else:
            outs, refs = [y], [G.mul_mat(w, G.op_unary_mul(G.UNARY_SILU, x0, x1))]
        run_and_compare(torch, plan, outs, refs)
    finally:
        plan.close()


def test_recipe_partners_on_a_tail_k(G, torch):
    """An IQ3 stage and a Q4_K stage whose rows end in a partial step (K = 2304) in one plan: the kernel with the per-lane tail test streams both."""
    rng = np.random.default_rng(6000)
    w1, w2 = W(G, oracle.IQ3_XXS, 2304, 2048, rng), W(G, oracle.Q4_K, 500, 2304, rng)
    x = dev(torch, rng.standard_normal((1, 2048)).astype(np.float32))
    y1, y2 = z(torch, 2304), z(torch, 500)
    plan = G.Plan([dict(ws=[w1], ys=[y1], x=x), dict(ws=[w2], ys=[y2], x=y1)])
    try:
        r1 = G.mul_mat(w1, x)
        run_and_compare(torch, plan, [y1, y2], [r1, G.mul_mat(w2, r1)])
    finally:
        plan.close()


def test_a_mix_without_a_kernel_is_refused(G, torch):
    """IQ3 types plan with the K-quants only: a plan that also holds a Q8_0 stage has no kernel instantiation and plan_create says so."""
    rng = np.random.default_rng(6100)
    w1, w2 = W(G, oracle.IQ3_S, 2048, 2048, rng), W(G, oracle.Q8_0, 64, 2048, rng)
    x = dev(torch, rng.standard_normal((1, 2048)).astype(np.float32))
    with pytest.raises(G.Mi355qError, match="no kernel instantiation"):
        G.Plan([dict(ws=[w1], ys=[z(torch, 2048)], x=x), dict(ws=[w2], ys=[z(torch, 64)], x=x)])


CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import torch
import ggml_mi355 as G
import test_gpu_plan_iq3 as T
try:
    T.two_stage(G, torch, 2048)
    print("RAN")
except G.Mi355qError as e:
    print("REFUSED", str(e).replace(chr(10), " "))
"""


def test_ring_engine_runs_the_same_checks_or_refuses():
    """The engine is chosen once per process: a fresh interpreter with MI355Q_PLAN_ENGINE=ring builds the two-stage plan.  Either it passes the
    same bit-for-bit checks, or plan_create refuses the types by name; any other end (wrong values, an abort) fails."""
    env = dict(os.environ, MI355Q_PLAN_ENGINE="ring")
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), str(PKG), str(ROOT / "tests")], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last == "RAN" or (last.startswith("REFUSED") and "plan_create" in last and "IQ3" in last), last
