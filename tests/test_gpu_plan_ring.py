"""The ring engine of the decode plan (csrc/plan_ring.hip, MI355Q_PLAN_ENGINE=ring), run on the cases of the register engine's tests.

The engine is chosen once per process, so every case runs in ONE fresh interpreter started with MI355Q_PLAN_ENGINE=ring (tests/ring_child.py);
it prints a PASS / FAIL line per case and each test here asserts its own line.  What the child runs:
  * the GEMV prologues and output forms of tests/test_gpu_plan.py (X_PLAIN, X_NORM with x1 / sum_out / x_out, X_UNARY_MUL, Y_UNARY_MUL, NO_PLAIN,
    a mixed-type group, epoch wrap): bit-identical to mul_mat on the node ops' activation vector, as there;
  * the f16 attention cases of tests/test_gpu_plan_attn_forms.py, short last splits and empty ones included.  The ring engine has one attention
    form, the global one (plan_attn, f32 accumulation; the CPU's f16-rounded probabilities at one split with a transposed V), so every case is
    held to the float64 bound -- the flash-layout single-split cases too, where the register engine follows the CPU's F16 accumulator -- with the
    stored rows bit-exact and the two garbage fillings giving the same bits.
"""
import numpy as np
import pytest

import oracle
from ring_child import run_ring_cases

pytestmark = pytest.mark.gpu

GEMV_CASES = [
    "prologues-q4_K", "prologues-q6_K", "prologues-q8_0",
    "y_unary_mul-q4_K-4096", "y_unary_mul-q6_K-14336", "y_unary_mul-q8_0-10007",
    "no_plain", "mixed_type_group-concurrent", "mixed_type_group-one_after_the_other", "x_out", "epoch_wrap",
    "attention_stage_against_the_node_ops", "stage_behind_attention-one_split", "stage_behind_attention-three_splits",
]
ATTN_CASES = [
    "fa_seq-8.8.32-kv128", "fa_seq-8.2.64-kv256-neox", "fa_seq-4.4.96-kv96", "fa_seq-32.8.128-kv256", "fa_seq-4.1.192-kv160-mqa", "fa_seq-4.4.256-kv64",
    "p_f16-8.8.32-kv128", "p_f16-32.8.128-kv256", "p_f16-4.4.256-kv64",
    "lds-combine-16.4.64-kv600", "lds-combine-short_last-32.8.128-kv1001", "lds-combine-32.8.128-kv1024-T", "global-32.8.128-kv4096", "global-32.8.128-kv4096-T",
    "global-64.8.128-kv2048", "global-unaligned-cache-32.8.128-kv256", "fallback-p_f16-32.8.128-kv100-T", "fallback-combine-8.8.32-kv300-per150-T",
]
ROPE_CASES = [f"{name}+{opt}" for name in ("fa_seq-32.8.128-kv256", "lds-combine-32.8.128-kv1024-T")
              for opt in ("freq_factors", "yarn", "ndims_half_mode0", "ndims_quarter_mode2", "pos100000")]
MASK_CASES = [f"{name}+{pattern}" for name in ("lds-combine-32.8.128-kv1024", "fallback-p_f16-32.8.128-kv100-T")
              for pattern in ("leading_run", "middle_run", "whole_split", "one_live_pos0")]
NKV_CASES = ["nkv-pos255-win256", "nkv-pos700-win704", "nkv-pos0-win1", "nkv-pos4-win5", "nkv-pos1000-win5000", "nkv_fa-win100",
             "nkv_rows-win5", "nkv_rows-win301"]
ALL = GEMV_CASES + ATTN_CASES + ROPE_CASES + MASK_CASES + NKV_CASES

GEMV_KINDS = ("prologues", "y_unary_mul", "no_plain", "mixed_type_group", "x_out", "epoch_wrap", "attention_stage_against_the_node_ops",
              "stage_behind_attention")


def gemv(G, torch, name):
    import test_gpu_plan as P
    t = {"q4_K": oracle.Q4_K, "q6_K": oracle.Q6_K, "q8_0": oracle.Q8_0}
    kind, _, rest = name.partition("-")
    if kind == "prologues": return P.test_norm_and_unary_prologues_match_the_node_ops(G, torch, t[rest])
    if kind == "y_unary_mul":
        ty, F = rest.split("-"); return P.test_paired_output_unary_mul(G, torch, t[ty], int(F))
    if kind == "no_plain": return P.test_no_plain_outputs_are_not_written(G, torch)
    if kind == "mixed_type_group": return P.test_mixed_type_stage_runs_as_a_group(G, torch, "1" if rest == "concurrent" else "0")
    if kind == "x_out": return P.test_x_out_stores_the_formed_vector(G, torch)
    if kind == "epoch_wrap": return P.test_epoch_wrap_resets_the_granules(G, torch)
    if kind == "attention_stage_against_the_node_ops": return P.test_attention_stage_against_the_node_ops(G, torch)
    if kind == "stage_behind_attention": return P.test_stage_behind_attention_skips_the_attention_workgroups(G, torch, 96 if rest == "one_split" else 600)
    raise KeyError(name)


def attn(G, torch, name):
    import test_gpu_plan_attn_forms as A
    if name.startswith("nkv_rows-win"):
        w = int(name[len("nkv_rows-win"):])
        case = A.Case(G, torch, 32, 8, 128, 1024, w - 1, "rows_v", mask="f32", n_kv_dev=w, seed=A.seed_of("rows_dev", w))
    elif name.startswith("nkv_fa-win"):
        w = int(name[len("nkv_fa-win"):])
        case = A.Case(G, torch, 32, 8, 128, 256, w - 1, "rows_v", mask="f16", n_kv_dev=w, seed=A.seed_of("fa_dev", w))
    elif name.startswith("nkv-"):
        pos, w = name[len("nkv-pos"):].split("-win")
        case = A.n_kv_dev_bench_case(G, torch, int(pos), int(w))
    else:
        base, _, opt = name.partition("+")
        over = {}
        if opt in A.ROPE_OPTS:
            rope, ff, pos = A.rope_option(opt, A.FORM_CASES[base][2], np.random.default_rng(A.seed_of(base, opt)))
            over = dict(rope=rope, ff=ff, pos=pos)
        elif opt:
            n_head, _, _, n_kv, slot = A.FORM_CASES[base][:5]
            live, slot = A.mask_pattern(opt, n_kv, slot, A.expected_splits(torch, n_head, n_kv))
            over = dict(live=live, slot=slot)
        case, form, envs = A.make_case(G, torch, base, **over)
        try:
            case.create(**envs)
            return A.run_and_check(case, form, name)
        finally:
            case.close()
    try:
        case.create()
        return A.run_and_check(case, "lds", name)
    finally:
        case.close()


def run_ring_case(G, torch, name):
    """What tests/ring_child.py calls per name in the ring engine's process."""
    return gemv(G, torch, name) if name.split("-")[0] in GEMV_KINDS else attn(G, torch, name)


@pytest.fixture(scope="module")
def ring_results():
    return run_ring_cases("test_gpu_plan_ring", ALL)[:3]


@pytest.mark.parametrize("name", ALL)
def test_ring_engine(ring_results, name):
    rc, lines, err = ring_results
    assert name in lines, (rc, err)
    assert lines[name].startswith("PASS"), lines[name]
