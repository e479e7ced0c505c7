"""The exact inputs of tests/qdata.py (exact_blocks / exact_acts), checked on the CPU for all 19 weight types: they are what lets
tests/test_gpu_mmq_forms.py hold the matrix-core tiers, and tests/test_gpu_gemv_forms.py the per-column tiers, to bit equality, so their
properties are proven here, without a GPU."""
import numpy as np
import pytest

import oracle
from qdata import (EXACT_CANONICAL_K, EXACT_FORM_KS, EXACT_UNIT, GEMV_ACT_KIND, GEMV_FORM_DATA, GEMV_PLANAR_TYPES, exact_acts, exact_blocks,
                   exact_output_bound, exact_product, exact_sum_bound, exact_x_unit, gemv_amplitude)

TYPES = [oracle.Q4_0, oracle.Q4_1, oracle.Q5_0, oracle.Q5_1, oracle.Q8_0, oracle.Q2_K, oracle.Q3_K,
         oracle.Q4_K, oracle.Q5_K, oracle.Q6_K, oracle.IQ4_NL, oracle.IQ4_XS,
         oracle.IQ2_XXS, oracle.IQ2_XS, oracle.IQ2_S, oracle.IQ3_XXS, oracle.IQ3_S, oracle.IQ1_S, oracle.IQ1_M]
ids_t = lambda t: oracle.TYPE_NAMES[t]

# Distinct magnitudes asked of every type: 16, except where the format under the |integer| < 256 limit has fewer levels.  Those maxima are
# counted from the format, not from the generator: the 2-bit code books hold the magnitudes {8, 25, 43} and the limit leaves the scale
# factors 1 + 2s = {1, 3, 5}: 9 distinct products; IQ3_XXS has {4, 12, 20, 28, 36, 44, 52, 62} x {1, 3}: 16 products, 14 of them distinct
# (12 = 3 x 4 and 36 = 3 x 12 occur twice).
_IQ2_LEVELS = len({g * s for g in (8, 25, 43) for s in (1, 3, 5)})
_IQ3_XXS_LEVELS = len({g * s for g in (4, 12, 20, 28, 36, 44, 52, 62) for s in (1, 3)})
MIN_LEVELS = {t: 16 for t in TYPES}
MIN_LEVELS.update({oracle.IQ2_XXS: _IQ2_LEVELS, oracle.IQ2_XS: _IQ2_LEVELS, oracle.IQ2_S: _IQ2_LEVELS, oracle.IQ3_XXS: _IQ3_XXS_LEVELS})


def bf16_round_trip(a: np.ndarray) -> np.ndarray:
    """f32 -> bf16 (round to nearest even) -> f32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def test_level_maxima_are_what_the_formats_allow():
    assert _IQ2_LEVELS == 9 and _IQ3_XXS_LEVELS == 14


@pytest.mark.parametrize("t", TYPES, ids=ids_t)
def test_exact_blocks_are_bf16_integers(orc, t):
    rng = np.random.default_rng(900 + t)
    K = 2048
    w = exact_blocks(t, 96, K, rng)
    assert w.dtype == np.uint8 and w.shape == (96, orc.row_size(t, K))
    dq = orc.dequantize(t, w, K)
    assert np.array_equal(bf16_round_trip(dq).view(np.uint32), dq.view(np.uint32)), "a weight is not a bf16 number"
    ints = dq.astype(np.float64) / EXACT_UNIT[t]
    assert np.array_equal(ints, np.round(ints)) and np.abs(ints).max() < 256
    mags = np.unique(np.abs(ints))
    assert len(mags) >= MIN_LEVELS[t], (ids_t(t), len(mags))
    assert (ints > 0).any() and (ints < 0).any()
    # the payload is still random: every byte of a block takes many values (the constraint touches scale fields only)
    blocks = w.reshape(-1, orc.type_size(t))
    assert (np.array([len(np.unique(blocks[:, i])) for i in range(blocks.shape[1])]) >= 2).sum() >= blocks.shape[1] - 8


@pytest.mark.parametrize("kind", ["bf16", "q8_0", "q8_k"])
def test_exact_acts(orc, kind):
    rng = np.random.default_rng(5)
    x = exact_acts(7, 1024, rng, kind)
    assert np.array_equal(x, np.round(x)) and np.array_equal(bf16_round_trip(x), x)
    body = np.abs(x) <= 16
    if kind == "bf16":
        assert body.all() and len(np.unique(x)) == 33
        return
    blk = 32 if kind == "q8_0" else 256
    assert (~body).reshape(7, -1, blk).sum(axis=2).min() == 1 and np.abs(x).max() == 127
    # the CPU's activation quantizer is the identity on them: d = +-1 and the quants are the values
    act = oracle.Q8_0 if kind == "q8_0" else oracle.Q8_K
    for mode in (oracle.ROUND_AWAY, oracle.ROUND_EVEN):
        q = orc.quantize_act(act, x, mode)
        if kind == "q8_0":
            b = q.reshape(7, -1, 34)
            assert (np.ascontiguousarray(b[:, :, :2]).view(np.float16) == 1.0).all()
            assert np.array_equal(b[:, :, 2:].view(np.int8).reshape(7, -1).astype(np.float32), x)
        else:
            b = q.reshape(7, -1, 292)
            d = np.ascontiguousarray(b[:, :, :4]).view(np.float32)
            assert (np.abs(d) == 1.0).all()
            assert np.array_equal((b[:, :, 4:260].view(np.int8).astype(np.float32) * d).reshape(7, -1), x)


@pytest.mark.parametrize("t", TYPES, ids=ids_t)
def test_sums_stay_below_2_24(orc, t):
    """The precondition of the GPU tests at every K they use (the bound does not depend on the row or token count beyond the maximum it
    takes; the GPU tests assert it again on their own data)."""
    rng = np.random.default_rng(700 + t)
    kinds = {oracle.Q4_K: ("bf16", "q8_k"), oracle.Q8_0: ("bf16", "q8_0")}.get(t, ("bf16",))
    for K in EXACT_FORM_KS.get(t, ()) + (EXACT_CANONICAL_K[t], 2048):
        w = exact_blocks(t, 256, K, rng)
        for kind in kinds:
            x = exact_acts(64, K, rng, kind)
            b = exact_sum_bound(orc, t, w, x, K)
            assert b < 2 ** 24, (ids_t(t), K, kind, b)
            true = (np.abs(x).astype(np.float64) @ (np.abs(orc.dequantize(t, w, K)).astype(np.float64) / EXACT_UNIT[t]).T).max()
            assert true <= b


@pytest.mark.parametrize("t,kind", [(oracle.Q4_K, "q8_k"), (oracle.Q8_0, "q8_0")], ids=["q4_K", "q8_0"])
def test_cpu_arithmetic_is_exact_on_them(orc, t, kind):
    """The CPU's own mul_mat (quantized activations, integer block sums, f32 block order) gives the float64 integer product bit for bit."""
    rng = np.random.default_rng(40 + t)
    for M, N, K in ((70, 9, 256), (33, 5, 4352)):
        w = exact_blocks(t, M, K, rng); x = exact_acts(N, K, rng, kind)
        assert exact_sum_bound(orc, t, w, x, K) < 2 ** 24
        exact = exact_product(orc, t, w, x, K)
        for mode in (oracle.ROUND_AWAY, oracle.ROUND_EVEN):
            got = orc.mul_mat(t, w, x, M, N, K, round_mode=mode)
            assert np.array_equal(got.view(np.uint32), exact.view(np.uint32))
        assert np.array_equal(exact.astype(np.float64), x.astype(np.float64) @ orc.dequantize(t, w, K).astype(np.float64).T)


# ------------------------------------------------------------------------------------------------
# the data of tests/test_gpu_gemv_forms.py
# ------------------------------------------------------------------------------------------------
def test_exact_acts_defaults_are_unchanged():
    """amp = 16 and no factors draw what exact_acts drew before it had those arguments."""
    a = exact_acts(3, 512, np.random.default_rng(8), "q8_k")
    rng = np.random.default_rng(8)
    b = rng.integers(-16, 17, (3, 512)).astype(np.float32)
    b.reshape(3, 2, 256)[:, :, 3] = -127.0
    assert np.array_equal(a, b)
    assert np.abs(exact_acts(4, 256, np.random.default_rng(9), "bf16", amp=2)).max() == 2


@pytest.mark.parametrize("kind", ["q8_0", "q8_1", "q8_k"])
def test_scaled_acts_quantize_to_their_factor(orc, kind):
    """With a factor 2^e per activation block the CPU's quantizer gives d = 2^e exactly and the integer quants of the unscaled block; an
    identity-quantized Q8_1 block has an exact f16 s = d * sum(q)."""
    rng = np.random.default_rng(77)
    n, k, es = 5, 1024, (-2, -1, 0, 1, 2)
    x = exact_acts(n, k, rng, "q8_k" if kind == "q8_k" else "q8_0", amp=16, factors=es)
    assert exact_x_unit(x) == 0.25 and exact_x_unit(exact_acts(n, k, rng, "q8_0")) == 1.0
    act = {"q8_0": oracle.Q8_0, "q8_1": oracle.Q8_1, "q8_k": oracle.Q8_K}[kind]
    for mode in (oracle.ROUND_AWAY, oracle.ROUND_EVEN):
        q = orc.quantize_act(act, x, mode)
        if kind == "q8_k":
            b = q.reshape(n, -1, 292)
            d = np.abs(np.ascontiguousarray(b[:, :, :4]).view(np.float32).reshape(n, -1))
            qs = b[:, :, 4:260].view(np.int8).astype(np.float32) * np.sign(np.ascontiguousarray(b[:, :, :4]).view(np.float32))
            blk = 256
        else:
            hdr = 2 if kind == "q8_0" else 4
            b = q.reshape(n, -1, 32 + hdr)
            d = np.ascontiguousarray(b[:, :, :2]).view(np.float16).astype(np.float32).reshape(n, -1)
            qs = b[:, :, hdr:].view(np.int8).astype(np.float32)
            blk = 32
            if kind == "q8_1":
                s = np.ascontiguousarray(b[:, :, 2:4]).view(np.float16).astype(np.float64).reshape(n, -1)
                assert np.array_equal(s, d.astype(np.float64) * qs.sum(axis=2)), "the f16 s field of a Q8_1 block is not exact"
        assert set(np.unique(np.log2(d))) == set(float(e) for e in es)
        assert np.array_equal((qs * d[:, :, None]).reshape(n, k), x)
        assert np.abs(qs).max() == 127 and (np.abs(qs).reshape(n, -1, blk).max(axis=2) == 127).all()


def test_gemv_form_data_table():
    """The table names every planar type at its single-step K and at ring K of 2 and 3 steps, and its amplitudes are gemv_amplitude's."""
    have = {(t, k) for t, k, _, _ in GEMV_FORM_DATA}
    for t in GEMV_PLANAR_TYPES:
        assert sum(1 for tt, _ in have if tt == t) >= 4
    for t, k, amp, fac in GEMV_FORM_DATA:
        assert (amp, fac) == gemv_amplitude(k, fac is not None) and k % (32 if GEMV_ACT_KIND[t] == "q8_0" else 256) == 0
    assert {t for t, _ in have} == set(TYPES)


@pytest.mark.parametrize("entry", GEMV_FORM_DATA, ids=lambda e: f"{ids_t(e[0])}-{e[1]}-{'scaled' if e[3] else 'identity'}")
def test_gemv_form_data_is_exact_on_the_cpu(orc, entry):
    """Per table entry: every output's sum (|w| + 2 mins) |x| is below 2^24 smallest units, and the CPU arithmetic the per-column tiers
    restate (quantized activations, integer block sums, one f32 product per block) returns the float64 product bit for bit."""
    t, K, amp, fac = entry
    rng = np.random.default_rng(300 + 1000 * t + K)
    M, N = 20, 3
    w = exact_blocks(t, M, K, rng)
    x = exact_acts(N, K, rng, GEMV_ACT_KIND[t], amp, fac)
    dq = orc.dequantize(t, w, K)
    b = exact_output_bound(orc, t, w, x, K, dq)
    assert b < 2 ** 24, (ids_t(t), K, amp, fac, b)
    true = (np.abs(x).astype(np.float64) @ np.abs(dq).astype(np.float64).T).max() / (EXACT_UNIT[t] * exact_x_unit(x))
    assert true <= b
    exact = exact_product(orc, t, w, x, K, dq)
    for mode in (oracle.ROUND_AWAY, oracle.ROUND_EVEN):
        got = orc.mul_mat(t, w, x, M, N, K, round_mode=mode)
        assert np.array_equal(got.view(np.uint32), exact.view(np.uint32)), (ids_t(t), K, amp, fac, mode)


@pytest.mark.parametrize("t", [oracle.Q4_0, oracle.Q5_1, oracle.Q6_K], ids=ids_t)         # Q8_0, Q8_1 and Q8_K activations
def test_gemv_form_data_mul_mat_id_is_exact_on_the_cpu(orc, t):
    K = 2304 if t == oracle.Q6_K else 3104
    amp, fac = gemv_amplitude(K, True)
    assert (t, K, amp, fac) in GEMV_FORM_DATA
    rng = np.random.default_rng(600 + t)
    M, n_expert, n_tok, n_used = 12, 4, 3, 2
    as_ = exact_blocks(t, n_expert * M, K, rng)
    ids = np.array([[0, 3], [2, 2], [1, 0]], np.int32)        # (one token picks the same expert twice)
    for x_ne1 in (1, n_used):
        x = exact_acts(n_tok * x_ne1, K, rng, GEMV_ACT_KIND[t], amp, fac)
        assert exact_output_bound(orc, t, as_, x, K) < 2 ** 24
        got = orc.mul_mat_id(t, as_, x.reshape(n_tok, x_ne1, K), ids, M, K, n_expert)
        rows = as_.reshape(n_expert, M, -1)
        for tk in range(n_tok):
            for u in range(n_used):
                exact = exact_product(orc, t, rows[ids[tk, u]], x.reshape(n_tok, x_ne1, K)[tk, u % x_ne1][None], K)[0]
                assert np.array_equal(got[tk, u].view(np.uint32), exact.view(np.uint32)), (ids_t(t), x_ne1, tk, u)


def test_q8_0_sentinels_are_the_identity_under_q8_k_too(orc):
    """A call that mixes Q8_0- and Q8_K-paired weights shares its activations: a sentinel per 32-block (no factors) is identity-quantized by
    both quantizers, so both CPU products are exact on it."""
    rng = np.random.default_rng(91)
    K, M, N = 2048, 20, 4
    amp, _ = gemv_amplitude(K, False)
    x = exact_acts(N, K, rng, "q8_0", amp)
    for t in (oracle.Q4_K, oracle.Q8_0):
        w = exact_blocks(t, M, K, rng)
        assert exact_output_bound(orc, t, w, x, K) < 2 ** 24
        assert np.array_equal(orc.mul_mat(t, w, x, M, N, K).view(np.uint32), exact_product(orc, t, w, x, K).view(np.uint32))
