"""The references of the float-weight GEMV tests (tests/fw_ref.py) against the recorded outputs of the reference CPU backend: f32_to_bf16 against
tests/golden/bf16_kv_convert.npz, vec_dot_bf16_avx2 against the K = 128 entries of tests/golden/bf16_kv_mul_mat.npz, bit for bit.  (The f16 side,
oracle.glue.vec_dot_f16_simd, is held to the reference by tests/test_oracle_glue.py.)  Validates the yardstick: no device, passes without the kernel."""
from pathlib import Path

import numpy as np

from fw_ref import f32_to_bf16, mul_mat_bf16, vec_dot_bf16_avx2, same_bits      # noqa: F401  (vec_dot_bf16_avx2: the restatement under test)

GOLDEN = Path(__file__).resolve().parent / "golden"


def test_f32_to_bf16_reproduces_the_cpu_bits():
    g = np.load(GOLDEN / "bf16_kv_convert.npz", allow_pickle=False)
    assert np.array_equal(f32_to_bf16(g["x"]), g["bits"])
    assert np.isnan(g["x"]).any() and np.isinf(g["x"]).any()                 # (the fixture covers the NaN rule and the infinities)


def test_vec_dot_bf16_avx2_reproduces_the_cpu_bits():
    g = np.load(GOLDEN / "bf16_kv_mul_mat.npz", allow_pickle=False)
    w, x = g["w_k128"], g["x_k128"]
    for n in range(1, 9):
        want = g[f"y_k128_n{n}"]
        got = mul_mat_bf16(w, x[:n])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), n


def test_vec_dot_bf16_avx2_tail_in_double():
    g = np.load(GOLDEN / "bf16_kv_mul_mat.npz", allow_pickle=False)           # (K = 100 and K = 8: the tail the kernel leaves to op_mul_mat_f)
    for K in (100, 8):
        got = mul_mat_bf16(g[f"w_k{K}"], g[f"x_k{K}"][:3])
        assert np.array_equal(got.view(np.uint32), g[f"y_k{K}_n3"].view(np.uint32)), K


def test_same_bits_tells_signed_zeros_and_nans():
    a = np.array([0.0, 1.0, np.nan], np.float32)
    assert same_bits(a, a.copy())
    assert not same_bits(np.array([-0.0, 1.0, np.nan], np.float32), a)
    assert not same_bits(np.array([0.0, 1.0, 2.0], np.float32), a) and not same_bits(a, np.array([0.0, 1.0, 2.0], np.float32))
