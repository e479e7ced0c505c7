"""The decode plan's operand hand-off: which earlier output a stage's operand means, by VALUE ID and by ADDRESS (resolve() of plan_create,
csrc/plan.hip, and its second copy in csrc/plan_ring.hip), through the C-ABI with the ids set.

The hand-off forms and the case that pins each (names as in CASES; the ring engine runs the RING subset in one child process):
  * two outputs in ONE block of memory, ids decide ............................ shared-ids-<type> (A, B, C(id A), D(id B)), shared-ids_late-<type>
        (A stores plainly too and its consumer comes last: the plain memory holds B's values by then), shared-ids-q4_K-near_wrap (granule reset)
  * the same plan without ids: "the latest earlier output that contains" ....... shared-addr-<type> (both consumers get B)
  * a sub-vector of a labelled output (p - r.p in take()) ...................... subvec-id-<type>: offsets 0, 2048, 2560 of one 3072-row output
  * a sub-vector found by address .............................................. subvec-addr-<type>
  * several outputs of one stage, granule padding after an odd row count ....... padding-groups1 / padding-groups0: matrices of 301, 1, 2048 and 1
        rows -- one block of 2351 granules, an odd count, so the next block starts behind the round-up -- then a Q4_K + Q6_K group (its
        two members own separate granule blocks); every output that can be an operand is consumed by id (the 301-row one at offsets 0
        and 32; a 1-row output cannot be an operand -- k % 32 -- so its plain value is checked).  The verbose lines of plan_create show
        that the group ran on disjoint workgroup ranges (groups1) or one member after the other on all of them (groups0).
  * sum_out as x and, in another stage, as x1; x_out equal to the formed vector . sum_xout-<type>
  * the labelled output of a paired (Y_UNARY_MUL) stage ......................... paired-<type> (ys[1] keeps its canary)
  * operand sources: x0 plain direct / plain gathered / granules, x1 absent / plain / granules, per x_kind ... src-<x_kind>-<x0>-<x1>-<type>
        (granule operands by address for q4_K, by id for q8_0).  No weight type has a planar K that is a multiple of 32 but not of 256
        (mi355q_weights_are_planar refuses every one up to 2048: planar rows need whole 256-element spans), so the gathered form of a plain
        X_PLAIN operand is reached with MI355Q_PLAN_DIRECT=0 at K = 2048, the only way there is; the verbose line of plan_create must say
        "x0 plain direct" for the direct cases and "x0 plain" alone for the gathered one.
  * attention: q and v labelled sub-vectors of one fused projection, k's plain address range on q's, out_id consumed by the next stage
        ... attention-ids.  With 4 heads and 4 kv heads q and k have one length, and two sub-vectors of ONE output cannot share addresses,
        so k is what ggml_gallocr makes of it (include/mi355q.h: K's projection reuses the dead pre-rope Q's block): a NO_PLAIN stage with
        its own id, listed behind the fused projection, whose output lies exactly on q's memory.  By address both q and k would be that
        later vector; the ids send q to the projection and k to the later stage.  v sits at offset 512 of the projection.
  * refusals (plan_create only, nothing is launched) ............................. refuse-*: an id nobody produces, a labelled operand that
        reaches past its output, an unlabelled operand that partly overlaps an output, sum_out / x_out / y on a plain operand of the
        same stage (sum_out and y accepted with NO_PLAIN), x_out with X_PLAIN, X_PLAIN with x1, an attention q_id nobody produces, an
        operand inside an x_out vector by address and -- fixed with this file -- with the id -1 the x_out record carried internally.
        The ring engine stores an X_PLAIN stage's x_out (the vector itself) by design, so refuse-x_out_with_x_plain is not in RING; its
        check of y against a plain operand of the same stage was missing and came with this file.
  * the ring child proves its engine (tests/ring_child.py) .......................... test_ring_child_ran_the_ring_engine

What is compared with what: a stage whose operand is complete before the launch and used as it is (X_PLAIN) runs tests/qdata.py's exact data
(weights and activations whose every partial sum is an exact f32; the bound is asserted on each case's own data) and must equal the float64
product bit for bit -- where such a stage stores no plain copy, the node op on the same data is held to the exact product instead and the
consumer to the node chain.  Every other stage is compared bit for bit with the node-by-node chain (mi355q_mul_mat, mi355q_op_unary_mul,
mi355q_op_add_rms_norm_mul) on the chain's own intermediate vectors; only what lies behind an X_NORM with an addend goes through
test_gpu_plan.close_or_equal (the f64 sum of squares is added in another order there).  The attention case keeps the helper's data and
reference of tests/test_gpu_plan_attn_forms.py (exact data would make the softmax one-hot).  Every plan runs three times with its outputs
zeroed in between and status() == 0 each time; plain buffers of NO_PLAIN stages hold a canary and must keep it.  Every producer has its own
random weights and activations, so a wrong source shows in nearly every element.

Mutants of resolve(), both engines changed alike in scratch builds, this file run once against each on an MI355X; the cases that failed
(every other case passed):
  (a) the id path drops the offset (p - r.p -> 0): subvec-id-q4_K, subvec-id-q8_0 (register and ring engine), padding-groups1,
      padding-groups0 (the consumer at offset 32), attention-ids (v at offset 512).
  (b) the address path takes the EARLIEST containing output: shared-addr-q4_K, shared-addr-q8_0 (register and ring engine: both
      consumers must get B).
"""
import re

import numpy as np
import pytest

import oracle
from ring_child import run_ring_cases
from qdata import GEMV_ACT_KIND, exact_acts, exact_blocks, exact_output_bound, exact_product, gemv_amplitude, quantized_weights

import test_gpu_plan as P
import test_gpu_plan_attn_forms as A

pytestmark = pytest.mark.gpu

Q = oracle
TN = oracle.TYPE_NAMES
CANARY = 7.0
ERR_UNSUPPORTED, ERR_SHAPE, ERR_ALIGN = -1, -2, -3            # include/mi355q.h
STRADDLES = "plan_create: an activation operand straddles an earlier output"
K0 = 2048

_ORC = []


def orc():
    if not _ORC:
        _ORC.append(oracle.Oracle())
    return _ORC[0]


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


dev, bits = P.dev, P.bits


def z(torch, n):
    return torch.zeros((1, n), dtype=torch.float32, device="cuda")


def canary(torch, n):
    return torch.full((1, n), CANARY, dtype=torch.float32, device="cuda")


def same(got, ref, what):
    g, r = bits(got).reshape(-1), (bits(ref) if hasattr(ref, "detach") else np.ascontiguousarray(ref, np.float32).view(np.uint32)).reshape(-1)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert np.array_equal(g, r), f"{what}: {(g != r).sum()} of {g.size} elements differ"


class Exact:
    """A weight of qdata's exact blocks on the device, with its host rows."""

    def __init__(self, G, t, m, k, rng):
        assert G.is_planar(t, k), (TN[t], k)
        self.t, self.m, self.k = t, m, k
        self.h = exact_blocks(t, m, k, rng)
        self.w = G.QWeight.from_host(t, self.h, m, k)

    def product(self, x):
        """The float64 product as f32 [1, m], after the precondition that makes it the only possible answer."""
        assert exact_output_bound(orc(), self.t, self.h, x, self.k) < 2 ** 24, (TN[self.t], self.k)
        return exact_product(orc(), self.t, self.h, x, self.k)


def exact_x(t, k, rng):
    amp, fac = gemv_amplitude(k, True)
    return exact_acts(1, k, rng, GEMV_ACT_KIND[t], amp, fac)


def rand_w(G, t, m, k, rng):
    assert G.is_planar(t, k), (TN[t], k)
    return G.QWeight.from_host(t, quantized_weights(t, m, k, rng, scale=0.5), m, k)


def rand_x(torch, k, rng):
    return dev(torch, rng.standard_normal((1, k)).astype(np.float32))


VERBOSE_GEMV = re.compile(r"gemv stage (\d+): k (\d+), (\d+) rows, workgroups \[(\d+), (\d+)\), group (\d+), x0 (plain direct|plain|granules)")
_CAPFD = [None]                                               # test_handoff's capfd: what lets a case read plan_create's verbose lines


def run_plan(G, torch, stages, outs, check, canaries=(), reps=3, near_wrap=False, envs=None, form=None):
    """Create, then `reps` times: zero the outputs, run, status() == 0, check(), canaries untouched.
    form: called with plan_create's verbose GEMV lines [(stage, k, rows, wg0, wg1, group, x0)] -- the register engine prints them; where
    stderr is not captured (the ring child) it is skipped."""
    capfd = _CAPFD[0] if form is not None else None
    if capfd is not None:
        capfd.readouterr()
    with A.env(**dict(envs or {}, MI355Q_PLAN_VERBOSE=1 if capfd is not None else None)):
        plan = G.Plan(stages)
    if capfd is not None:
        lines = [(int(m[1]), int(m[2]), int(m[3]), int(m[4]), int(m[5]), int(m[6]), m[7]) for m in VERBOSE_GEMV.finditer(capfd.readouterr().err)]
        assert lines, "plan_create printed no gemv stage lines"
        form(lines)
    try:
        if near_wrap:                                         # the granule reset falls inside the runs below (cf. test_epoch_wrap_resets_the_granules)
            plan.debug_set_runs(0xFFFFFFFF // (plan.launch_stages + 1) - 3)
        for rep in range(reps):
            for b in outs:
                b.zero_()
            plan.run(); torch.cuda.synchronize()
            assert plan.status() == 0
            check()
            for c in canaries:
                assert bool((c == CANARY).all()), "a NO_PLAIN stage wrote its plain buffer"
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------
# two outputs in one block of memory
# ------------------------------------------------------------------------------------------------
def case_shared(G, torch, t, variant, near_wrap=False):
    rng = np.random.default_rng(A.seed_of("shared", t, variant))
    eA, eB = Exact(G, t, K0, K0, rng), Exact(G, t, K0, K0, rng)
    xa, xb = exact_x(t, K0, rng), exact_x(t, K0, rng)
    wC, wD = rand_w(G, t, 300, K0, rng), rand_w(G, t, 301, K0, rng)
    dxa, dxb = dev(torch, xa), dev(torch, xb)
    shared, yC, yD = z(torch, K0), z(torch, 300), z(torch, 301)
    nA, nB = G.mul_mat(eA.w, dxa), G.mul_mat(eB.w, dxb)
    rB = eB.product(xb)
    same(nA, eA.product(xa), "node op A against the exact product"); same(nB, rB, "node op B against the exact product")
    assert (bits(nA) != bits(nB)).mean() > 0.9                # the two values differ nearly everywhere
    ids = variant != "addr"
    sA = dict(ws=[eA.w], ys=[shared], x=dxa, no_plain=variant != "ids_late", y_ids=[1] if ids else None)
    sB = dict(ws=[eB.w], ys=[shared], x=dxb, y_ids=[2] if ids else None)
    sC = dict(ws=[wC], ys=[yC], x=shared, x_id=1 if ids else 0)
    sD = dict(ws=[wD], ys=[yD], x=shared, x_id=2 if ids else 0)
    stages = [sA, sB, sD, sC] if variant == "ids_late" else [sA, sB, sC, sD]
    rC, rD = G.mul_mat(wC, nA if ids else nB), G.mul_mat(wD, nB)

    def check():
        if variant != "ids_late":                             # (A is NO_PLAIN: the memory holds B alone)
            same(shared, rB, "B's plain copy against the exact product")
        same(yC, rC, "C: " + ("the value with A's id" if ids else "the latest output at the address, B"))
        same(yD, rD, "D: B's value")
    run_plan(G, torch, stages, [shared, yC, yD], check, reps=6 if near_wrap else 3, near_wrap=near_wrap)


# ------------------------------------------------------------------------------------------------
# sub-vectors of one fused output
# ------------------------------------------------------------------------------------------------
def case_subvec(G, torch, t, by_id):
    rng = np.random.default_rng(A.seed_of("subvec", t, by_id))
    parts = ((0, 2048, 300), (2048, 512, 301), (2560, 512, 77))          # (float offset, K, rows of the consumer)
    eF = Exact(G, t, 3072, K0, rng)
    x = exact_x(t, K0, rng)
    ws = [rand_w(G, t, m, k, rng) for _, k, m in parts]
    fused = z(torch, 3072)
    ys = [z(torch, m) for _, _, m in parts]
    rF = eF.product(x)
    nF = G.mul_mat(eF.w, dev(torch, x))
    same(nF, rF, "node op against the exact product")
    refs = [G.mul_mat(w, nF[:, o:o + k].contiguous()) for w, (o, k, _) in zip(ws, parts)]
    stages = [dict(ws=[eF.w], ys=[fused], x=dev(torch, x), y_ids=[5] if by_id else None)]
    stages += [dict(ws=[w], ys=[y], x=fused[:, o:o + k], x_id=5 if by_id else 0) for w, y, (o, k, _) in zip(ws, ys, parts)]

    def check():
        same(fused, rF, "the fused output against the exact product")
        for y, r, (o, k, _) in zip(ys, refs, parts):
            same(y, r, f"consumer of elements [{o}, {o + k})")
    run_plan(G, torch, stages, [fused] + ys, check)


# ------------------------------------------------------------------------------------------------
# several outputs of one stage, granule padding, a mixed-type group
# ------------------------------------------------------------------------------------------------
def case_padding(G, torch, groups):
    rng = np.random.default_rng(A.seed_of("padding"))
    e1 = [Exact(G, Q.Q4_K, m, K0, rng) for m in (301, 1, 2048, 1)]            # 2351 rows: the block is rounded up to an even granule count
    e2 = [Exact(G, Q.Q4_K, K0, K0, rng), Exact(G, Q.Q6_K, K0, K0, rng)]
    x1, x2 = exact_x(Q.Q4_K, K0, rng), exact_x(Q.Q4_K, K0, rng)       # (Q4_K and Q6_K pair with the same activation format)
    y1 = [z(torch, e.m) for e in e1]
    y2 = [canary(torch, K0), canary(torch, K0)]                       # the group stores no plain copies
    r1 = [e.product(x1) for e in e1]
    n2 = [G.mul_mat(e.w, dev(torch, x2)) for e in e2]
    for n, e in zip(n2, e2):
        same(n, e.product(x2), "node op against the exact product")
    n1 = [dev(torch, r) for r in r1]
    # (id, source vector, float offset, K, consumer type, rows)
    cons = [(11, 0, 0, 256, Q.Q4_K, 64), (11, 0, 32, 256, Q.Q8_0, 65), (13, 2, 0, K0, Q.Q4_K, 300), (14, 4, 0, K0, Q.Q6_K, 77), (15, 5, 0, K0, Q.Q4_K, 301)]
    srcs, nodes = y1 + y2, n1 + n2
    cw = [rand_w(G, t, m, k, rng) for _, _, _, k, t, m in cons]
    cy = [z(torch, m) for *_, m in cons]
    refs = [G.mul_mat(w, nodes[s][:, o:o + k].contiguous()) for w, (_, s, o, k, _, _) in zip(cw, cons)]
    stages = [dict(ws=[e.w for e in e1], ys=y1, x=dev(torch, x1), y_ids=[11, 12, 13, 16]),
              dict(ws=[e.w for e in e2], ys=y2, x=dev(torch, x2), y_ids=[14, 15], no_plain=True)]
    stages += [dict(ws=[w], ys=[y], x=srcs[s][:, o:o + k], x_id=i) for w, y, (i, s, o, k, _, _) in zip(cw, cy, cons)]

    def check():
        for y, r, e in zip(y1, r1, e1):
            same(y, r, f"the {e.m}-row output against the exact product")
        for y, r, c in zip(cy, refs, cons):
            same(y, r, f"consumer of id {c[0]} at offset {c[2]}")
    def form(lines):
        assert sum(e.m for e in e1) % 2 == 1 and lines[0][2] == sum(e.m for e in e1)
        (_, _, _, a0, a1, ga, _), (_, _, _, b0, b1, gb, _) = lines[1], lines[2]
        if groups == "1":
            assert ga == 2 and gb == 1 and a0 == 0 and a1 == b0 and b1 > b0, lines[1:3]      # disjoint workgroup ranges, side by side
        else:
            assert ga == 1 and gb == 1 and (a0, a1) == (b0, b1) == lines[0][3:5], lines[1:3]   # every workgroup, one after the other
    run_plan(G, torch, stages, y1 + cy, check, canaries=y2, envs=dict(MI355Q_PLAN_GROUPS=groups), form=form)


# ------------------------------------------------------------------------------------------------
# sum_out and x_out
# ------------------------------------------------------------------------------------------------
def case_sum_xout(G, torch, t):
    rng = np.random.default_rng(A.seed_of("sum_xout", t))
    eps = 1e-5
    h, o, p = rand_x(torch, K0, rng), rand_x(torch, K0, rng), rand_x(torch, K0, rng)
    nw1, nw2 = (dev(torch, (1.0 + 0.1 * rng.standard_normal(K0)).astype(np.float32)) for _ in range(2))
    w1, wT, wU, wV = rand_w(G, t, 300, K0, rng), rand_w(G, t, K0, K0, rng), rand_w(G, t, 301, K0, rng), rand_w(G, t, 77, K0, rng)
    so, xo, y1, yT, so2, yU, xo2, yV = z(torch, K0), z(torch, K0), z(torch, 300), z(torch, K0), z(torch, K0), z(torch, 301), z(torch, K0), z(torch, 77)
    stages = [
        dict(ws=[w1], ys=[y1], x=h, x1=o, x_kind=G.X_NORM, norm_w=nw1, eps=eps, sum_out=so, sum_id=21, x_out=xo),
        dict(ws=[wT], ys=[yT], x=so, x_id=21, y_ids=[22]),                                            # the sum as x
        dict(ws=[wU], ys=[yU], x=yT, x_id=22, x1=so, x1_id=21, x_kind=G.X_NORM, norm_w=nw2, eps=eps, sum_out=so2),   # ... and as x1
        dict(ws=[wV], ys=[yV], x=yT, x_id=22, x1=p, x_kind=G.X_UNARY_MUL, unary=G.UNARY_SILU, x_out=xo2),
    ]
    r_x, r_sum = G.op_add_rms_norm_mul(h, eps, b=o, weight=nw1, want_sum=True)
    r_y1, r_T = G.mul_mat(w1, r_x), G.mul_mat(wT, r_sum)
    r_xu, r_sum2 = G.op_add_rms_norm_mul(r_T, eps, b=r_sum, weight=nw2, want_sum=True)
    r_U = G.mul_mat(wU, r_xu)
    r_xv = G.op_unary_mul(G.UNARY_SILU, r_T, p)
    r_V = G.mul_mat(wV, r_xv)

    def check():
        same(so, r_sum, "sum_out"); same(yT, r_T, "the stage that reads the sum as x"); same(so2, r_sum2, "the sum of the stage that reads it as x1")
        same(xo2, r_xv, "x_out of the X_UNARY_MUL stage"); same(yV, r_V, "the X_UNARY_MUL stage")
        for got, ref, what in ((xo, r_x, "x_out of the X_NORM stage"), (y1, r_y1, "behind the norm"), (yU, r_U, "behind the second norm")):
            P.close_or_equal(got, ref, what)
    run_plan(G, torch, stages, [so, xo, y1, yT, so2, yU, xo2, yV], check)


# ------------------------------------------------------------------------------------------------
# the labelled output of a paired stage
# ------------------------------------------------------------------------------------------------
def case_paired(G, torch, t):
    rng = np.random.default_rng(A.seed_of("paired", t))
    eg, eu = Exact(G, t, K0, K0, rng), Exact(G, t, K0, K0, rng)
    x = exact_x(t, K0, rng)
    dx = dev(torch, x)
    wd = rand_w(G, t, 300, K0, rng)
    act, unused, down = z(torch, K0), canary(torch, K0), z(torch, 300)
    ng, nu = G.mul_mat(eg.w, dx), G.mul_mat(eu.w, dx)
    same(ng, eg.product(x), "gate against the exact product"); same(nu, eu.product(x), "up against the exact product")
    r_act = G.op_unary_mul(G.UNARY_SILU, ng, nu)
    r_down = G.mul_mat(wd, r_act)
    stages = [dict(ws=[eg.w, eu.w], ys=[act, unused], x=dx, y_kind=G.Y_UNARY_MUL, y_unary=G.UNARY_SILU, y_ids=[31, 0]),
              dict(ws=[wd], ys=[down], x=act, x_id=31)]

    def check():
        same(act, r_act, "the paired output"); same(down, r_down, "its consumer by id")
    run_plan(G, torch, stages, [act, down], check, canaries=[unused])


# ------------------------------------------------------------------------------------------------
# operand sources
# ------------------------------------------------------------------------------------------------
def case_sources(G, torch, t, x_kind, s0, s1):
    """x_kind "plain" / "norm" / "unary"; s0 "direct" / "gathered" (plain) / "gran"; s1 None / "plain" / "gran"."""
    rng = np.random.default_rng(A.seed_of("src", t, x_kind, s0, s1))
    eps = 1e-5
    by_id = t == Q.Q8_0
    eP = [Exact(G, t, K0, K0, rng), Exact(G, t, K0, K0, rng)]
    xp = exact_x(t, K0, rng)
    g = [z(torch, K0), z(torch, K0)]
    nG = [G.mul_mat(e.w, dev(torch, xp)) for e in eP]
    rG = [e.product(xp) for e in eP]
    y = z(torch, 300)
    stage = dict(ys=[y], x_kind={"plain": G.X_PLAIN, "norm": G.X_NORM, "unary": G.X_UNARY_MUL}[x_kind], unary=G.UNARY_SILU)
    exact_ref = None
    if s0 == "gran":
        v0 = nG[0]; stage.update(x=g[0], x_id=41 if by_id else 0)
    elif x_kind == "plain":                                   # complete before the launch and used as it is: exact data
        xe = exact_x(t, K0, rng)
        v0 = dev(torch, xe); stage.update(x=v0)
    else:
        v0 = rand_x(torch, K0, rng); stage.update(x=v0)
    v1 = None
    if s1 == "gran":
        v1 = nG[1]; stage.update(x1=g[1], x1_id=42 if by_id else 0)
    elif s1 == "plain":
        v1 = rand_x(torch, K0, rng); stage.update(x1=v1)
    if x_kind == "plain" and s0 != "gran":
        eC = Exact(G, t, 300, K0, rng)
        stage.update(ws=[eC.w]); exact_ref = eC.product(xe)
        ref = G.mul_mat(eC.w, v0)
    else:
        wc = rand_w(G, t, 300, K0, rng)
        stage.update(ws=[wc])
        if x_kind == "plain":
            xf = v0
        elif x_kind == "norm":
            nw = dev(torch, (1.0 + 0.1 * rng.standard_normal(K0)).astype(np.float32))
            stage.update(norm_w=nw, eps=eps)
            xf = G.op_add_rms_norm_mul(v0, eps, b=v1, weight=nw)
        else:
            xf = G.op_unary_mul(G.UNARY_SILU, v0, v1)
        ref = G.mul_mat(wc, xf)
    stages = [dict(ws=[e.w for e in eP], ys=g, x=dev(torch, xp), y_ids=[41, 42] if by_id else None), stage]

    def check():
        for got, r in zip(g, rG):
            same(got, r, "the producer against the exact product")
        if exact_ref is not None:
            same(y, exact_ref, "a plain X_PLAIN operand against the exact product")
        if x_kind == "norm" and s1 is not None:
            P.close_or_equal(y, ref, "behind a norm with an addend")
        else:
            same(y, ref, f"{x_kind} with x0 {s0}, x1 {s1}")
    def form(lines):
        want = {"direct": "plain direct" if x_kind == "plain" else "plain", "gathered": "plain", "gran": "granules"}[s0]
        assert lines[-1][6] == want, (lines[-1], want)
        assert lines[0][6] == ("plain" if s0 == "gathered" else "plain direct"), lines[0]
    run_plan(G, torch, stages, g + [y], check, envs=dict(MI355Q_PLAN_DIRECT=0 if s0 == "gathered" else None), form=form)


# ------------------------------------------------------------------------------------------------
# attention: q, k, v out of one fused projection, the output consumed by id
# ------------------------------------------------------------------------------------------------
def case_attention(G, torch):
    n_head, hd, n_kv, slot, E = 4, 64, 37, 20, 256
    case = A.Case(G, torch, n_head, n_head, hd, n_kv, slot, layout="rows_v", mask="f16", seed=A.seed_of("handoff-attention"), E=E)
    rng = np.random.default_rng(A.seed_of("handoff-attention", "fused"))
    n = n_head * hd
    x = case.stages[0]["x"]
    wf, wk, wo = rand_w(G, Q.Q4_K, 3 * n, E, rng), rand_w(G, Q.Q4_K, n, E, rng), rand_w(G, Q.Q4_K, 300, n, rng)
    fused, yo = z(torch, 3 * n), z(torch, 300)
    q_mem, v_mem = fused[:, 0:n], fused[:, 2 * n:3 * n]
    r_fused, r_k = G.mul_mat(wf, x), G.mul_mat(wk, x)
    assert (bits(r_k) != bits(r_fused[:, 0:n].contiguous())).mean() > 0.9 and (bits(r_k) != bits(r_fused[:, n:2 * n].contiguous())).mean() > 0.9
    # the helper's checks read q / k / v through these: q and v are the plain copies of the projection; k has none (NO_PLAIN, on q's memory),
    # so the helper gets the node op's vector, which the stored K row is then held to bit for bit
    case.q, case.k, case.v = q_mem, r_k, v_mem
    case.attn.update(q=q_mem, k=q_mem, v=v_mem, q_id=5, k_id=7, v_id=5, out_id=6)
    case.stages = [dict(ws=[wf], ys=[fused], x=x, y_ids=[5]),
                   dict(ws=[wk], ys=[q_mem], x=x, y_ids=[7], no_plain=True),           # K's projection on the memory of q: by address q AND k would be this
                   dict(attn=case.attn),
                   dict(ws=[wo], ys=[yo], x=case.out, x_id=6)]
    try:
        case.create()
        for rep in range(3):
            fused.zero_(); yo.zero_()
            A.run_and_check(case, "fa_seq", "attention-ids")                            # stores and output against the helper's reference, two runs
            same(fused, r_fused, "the fused projection (the NO_PLAIN stage on q's memory must not store)")
            same(yo, G.mul_mat(wo, case.out), "the consumer of out_id")
    finally:
        case.close()


# ------------------------------------------------------------------------------------------------
# refusals: plan_create only
# ------------------------------------------------------------------------------------------------
def refused(G, stages, code, text):
    with pytest.raises(G.Mi355qError, match=re.escape(f"plan_create failed ({code}): {text}")):
        G.Plan(stages).close()


def accepted(G, stages):
    G.Plan(stages).close()


def _refusal_parts(G, torch, t=Q.Q4_K):
    rng = np.random.default_rng(3)
    w = rand_w(G, t, K0, K0, rng)
    buf = z(torch, 2 * K0)
    return w, buf, rand_x(torch, K0, rng), rand_x(torch, K0, rng), dev(torch, np.ones(K0, np.float32))


def refuse_unknown_id(G, torch):
    w, buf, x, x1, nw = _refusal_parts(G, torch)
    y = z(torch, K0)
    refused(G, [dict(ws=[w], ys=[y], x=x, y_ids=[1]), dict(ws=[w], ys=[buf[:, :K0]], x=y, x_id=99)], ERR_SHAPE, STRADDLES)
    refused(G, [dict(ws=[w], ys=[y], x=x, x_id=1)], ERR_SHAPE, STRADDLES)             # (an id on a vector that is complete before the launch)
    refused(G, [dict(ws=[w], ys=[y], x=x, y_ids=[1]), dict(ws=[w], ys=[buf[:, :K0]], x=x, x1=y, x1_id=2, x_kind=G.X_NORM, norm_w=nw, eps=1e-5)],
            ERR_SHAPE, STRADDLES)


def refuse_past_the_output(G, torch):
    w, buf, x, x1, nw = _refusal_parts(G, torch)
    y = z(torch, K0)
    stages = lambda off: [dict(ws=[w], ys=[buf[:, :K0]], x=x, y_ids=[1]), dict(ws=[w], ys=[y], x=buf[:, off:off + K0], x_id=1)]
    accepted(G, stages(0))
    refused(G, stages(32), ERR_SHAPE, STRADDLES)


def refuse_partial_overlap(G, torch):
    w, buf, x, x1, nw = _refusal_parts(G, torch)
    y = z(torch, K0)
    stages = lambda off: [dict(ws=[w], ys=[buf[:, :K0]], x=x), dict(ws=[w], ys=[y], x=buf[:, off:off + K0])]
    accepted(G, stages(0))
    refused(G, stages(32), ERR_SHAPE, STRADDLES)
    accepted(G, stages(K0))                                   # (beside the output: a plain vector)


def refuse_sum_out_on_an_operand(G, torch):
    w, buf, x, x1, nw = _refusal_parts(G, torch)
    for so in (x, x1):
        st = dict(ws=[w], ys=[buf[:, :K0]], x=x, x1=x1, x_kind=G.X_NORM, norm_w=nw, eps=1e-5, sum_out=so)
        refused(G, [st], ERR_SHAPE, "plan_create: sum_out overlaps a plain operand of the same stage")
        accepted(G, [dict(st, no_plain=True)])


def refuse_x_out_on_an_operand(G, torch):
    w, buf, x, x1, nw = _refusal_parts(G, torch)
    for xo in (x, x1):
        for no_plain in (False, True):                        # (x_out is stored either way)
            refused(G, [dict(ws=[w], ys=[buf[:, :K0]], x=x, x1=x1, x_kind=G.X_UNARY_MUL, x_out=xo, no_plain=no_plain)], ERR_SHAPE,
                    "plan_create: x_out overlaps a plain operand of the same stage")


def refuse_y_on_an_operand(G, torch):
    w, buf, x, x1, nw = _refusal_parts(G, torch)
    for y in (x, x1):
        st = dict(ws=[w], ys=[y], x=x, x1=x1, x_kind=G.X_UNARY_MUL)
        refused(G, [st], ERR_SHAPE, "plan_create: an output overlaps a plain operand of the same stage")
        accepted(G, [dict(st, no_plain=True)])


def refuse_x_out_with_x_plain(G, torch):
    w, buf, x, x1, nw = _refusal_parts(G, torch)
    refused(G, [dict(ws=[w], ys=[buf[:, :K0]], x=x, x_out=buf[:, K0:])], ERR_ALIGN,
            "plan_create: x_out needs X_NORM / X_UNARY_MUL, 16-byte alignment and k % 4 == 0")


def refuse_x_plain_with_x1(G, torch):
    w, buf, x, x1, nw = _refusal_parts(G, torch)
    refused(G, [dict(ws=[w], ys=[buf[:, :K0]], x=x, x1=x1)], ERR_SHAPE, "plan_create: X_PLAIN takes one operand")


def refuse_attention_unknown_id(G, torch):
    case = A.Case(G, torch, 4, 4, 64, 37, 20, layout="rows_v", mask="f16", seed=1)
    case.stages[0]["y_ids"] = [1, 2, 3]
    accepted(G, [case.stages[0], dict(attn=dict(case.attn, q_id=1, k_id=2, v_id=3))])
    for name in ("q_id", "k_id", "v_id"):
        ids = dict(q_id=1, k_id=2, v_id=3); ids[name] = 9
        refused(G, [case.stages[0], dict(attn=dict(case.attn, **ids))], ERR_SHAPE, "plan_create: attn operand straddles an earlier output")


def refuse_operand_in_x_out(G, torch):
    """An x_out vector is stored plainly DURING the launch: no later stage can read it.  By address that was refused; with the id -1, which
    the x_out record carried internally, the operand resolved to a granule pointer of offset (size_t) -1 + 1 instead."""
    w, buf, x, x1, nw = _refusal_parts(G, torch)
    xo, y = z(torch, K0), z(torch, K0)
    first = dict(ws=[w], ys=[buf[:, :K0]], x=x, x1=x1, x_kind=G.X_UNARY_MUL, x_out=xo)
    refused(G, [first, dict(ws=[w], ys=[y], x=xo)], ERR_SHAPE, STRADDLES)
    refused(G, [first, dict(ws=[w], ys=[y], x=xo, x_id=-1)], ERR_SHAPE, STRADDLES)
    refused(G, [first, dict(ws=[w], ys=[y], x=x, x1=xo, x1_id=-1, x_kind=G.X_UNARY_MUL)], ERR_SHAPE, STRADDLES)
    # -1 is an id like any other: an output that carries it is found, also when an x_out record lies behind it in the list
    accepted(G, [dict(first, y_ids=[-1]), dict(ws=[w], ys=[y], x=buf[:, :K0], x_id=-1)])


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
def _cases():
    c = {}
    for t in (Q.Q4_K, Q.Q5_K, Q.Q6_K, Q.IQ3_S, Q.Q8_0, Q.Q4_0):
        c[f"shared-ids-{TN[t]}"] = lambda G, torch, t=t: case_shared(G, torch, t, "ids")
    for t in (Q.Q4_K, Q.Q8_0):
        c[f"shared-addr-{TN[t]}"] = lambda G, torch, t=t: case_shared(G, torch, t, "addr")
        c[f"shared-ids_late-{TN[t]}"] = lambda G, torch, t=t: case_shared(G, torch, t, "ids_late")
    c["shared-ids-q4_K-near_wrap"] = lambda G, torch: case_shared(G, torch, Q.Q4_K, "ids", near_wrap=True)
    for t in (Q.Q4_K, Q.Q8_0):
        c[f"subvec-id-{TN[t]}"] = lambda G, torch, t=t: case_subvec(G, torch, t, True)
        c[f"subvec-addr-{TN[t]}"] = lambda G, torch, t=t: case_subvec(G, torch, t, False)
    c["padding-groups1"] = lambda G, torch: case_padding(G, torch, "1")
    c["padding-groups0"] = lambda G, torch: case_padding(G, torch, "0")
    for t in (Q.Q4_K, Q.Q8_0):
        c[f"sum_xout-{TN[t]}"] = lambda G, torch, t=t: case_sum_xout(G, torch, t)
        c[f"paired-{TN[t]}"] = lambda G, torch, t=t: case_paired(G, torch, t)
    combos = [("plain", s0, None) for s0 in ("direct", "gathered", "gran")]
    combos += [("norm", s0, s1) for s0 in ("direct", "gran") for s1 in (None, "plain", "gran")]
    combos += [("unary", s0, s1) for s0 in ("direct", "gran") for s1 in ("plain", "gran")]
    for t in (Q.Q4_K, Q.Q8_0):
        for kind, s0, s1 in combos:
            c[f"src-{kind}-{s0}-{s1 or 'none'}-{TN[t]}"] = lambda G, torch, t=t, kind=kind, s0=s0, s1=s1: case_sources(G, torch, t, kind, s0, s1)
    c["attention-ids"] = case_attention
    for f in (refuse_unknown_id, refuse_past_the_output, refuse_partial_overlap, refuse_sum_out_on_an_operand, refuse_x_out_on_an_operand,
              refuse_y_on_an_operand, refuse_x_out_with_x_plain, refuse_x_plain_with_x1, refuse_attention_unknown_id, refuse_operand_in_x_out):
        c[f.__name__.replace("refuse_", "refuse-")] = f
    return c


CASES = _cases()
# the ring engine: the id, address, sub-vector and refusal cases, for the types it streams (no IQ3); it stores an X_PLAIN stage's x_out by design
RING = [n for n in CASES if n.startswith(("shared-", "subvec-", "refuse-")) and "iq3" not in n and n != "refuse-x_out_with_x_plain"]


@pytest.mark.parametrize("name", list(CASES))
def test_handoff(G, torch, capfd, name):
    _CAPFD[0] = capfd
    try:
        CASES[name](G, torch)
    finally:
        _CAPFD[0] = None


def run_ring_case(G, torch, name):
    """What tests/ring_child.py calls per name in the ring engine's process."""
    return CASES[name](G, torch)


@pytest.fixture(scope="module")
def ring_results():
    return run_ring_cases("test_gpu_plan_handoff", RING, timeout=600)


def test_ring_child_ran_the_ring_engine(ring_results):
    assert ring_results[3] == "ring", ring_results


@pytest.mark.parametrize("name", RING)
def test_ring_engine(ring_results, name):
    rc, lines, err, _ = ring_results
    assert name in lines, (rc, err)
    assert lines[name].startswith("PASS"), lines[name]
