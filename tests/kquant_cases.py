"""Seeded cases of the K-quant scale-record tests (tests/test_gpu_kquant_records.py) and of the script that recorded their outputs
(tests/golden/make_kquant_records_golden.py): the weights, the activations and the batch sizes, one definition for both."""
from __future__ import annotations

import numpy as np

import oracle
from qdata import random_blocks

M = 64
# K = 256 (one block), the Llama-3-8B K's of the attention / FFN-up (4096) and FFN-down (14336) products
KS = (256, 4096, 14336)
# GEMV tier (N <= 8) and both prefill tiers (Q4_K: integer matrix cores, Q5_K: bf16 matrix cores; N > 8)
NS = (1, 2, 8, 16, 64)
TYPES = (oracle.Q4_K, oracle.Q5_K)


def case_inputs(t: int, k: int, n: int):
    rng = np.random.default_rng(1000 * t + 7 * (k // 256) + n)
    w = random_blocks(t, M, k, rng, scale=0.5)
    x = rng.standard_normal((n, k)).astype(np.float32)
    return w, x


def golden_key(t: int, k: int, n: int) -> str:
    return f"{oracle.TYPE_NAMES[t]}_k{k}_n{n}"
