#!/usr/bin/env python3
"""Generate tests/golden/fa_fused_prefill_gqa_d128_kv256.npz from the REAL reference: GGML_OP_FLASH_ATTN_EXT for a prompt-sized batch on an
F16 K / V cache, computed by the reference CPU backend through oracle/_ref (refshim ref_flash_attn_ext).  It is the yardstick of
tests/test_gpu_fa_fused.py: the fused matrix-core kernel must be as close to the CPU as the three-step matrix-core path is.
Run where the reference build exists:  python tests/golden/make_fa_fused_golden.py
Seeded gaussians; q is stored as the f16 values the CPU rounds it to anyway (half the bytes); arrays only (loadable with allow_pickle=False)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import oracle  # noqa: E402

OUT = Path(__file__).resolve().parent
TAG = "prefill_gqa_d128_kv256"
H, HK, N, D, N_KV = 4, 2, 48, 128, 256


def main() -> None:
    ref = oracle.Reference("avx2")                                    # (the reference CPU backend itself, as make_flash_attn_golden.py)
    rng = np.random.default_rng(sum(map(ord, TAG)))
    q = rng.standard_normal((1, H, N, D)).astype(np.float16)
    k = rng.standard_normal((1, HK, N_KV, D)).astype(np.float16)
    v = rng.standard_normal((1, HK, N_KV, D)).astype(np.float16)
    mask = np.zeros((64, N_KV), np.float16)                           # rows padded to GGML_KQ_MASK_PAD
    for t in range(N):
        mask[t, N_KV - N + t + 1:] = -np.inf                          # causal: the batch is the last N positions of the window
    scale = np.float32(1.0 / np.sqrt(D))
    y = ref.flash_attn_ext(q.astype(np.float32), k, v, mask, float(scale))
    assert np.isfinite(y).all()
    np.savez_compressed(OUT / f"fa_fused_{TAG}.npz", q=q, k=k, v=v, mask=mask, scale=scale, max_bias=np.float32(0), softcap=np.float32(0), y=y)
    print("wrote", OUT / f"fa_fused_{TAG}.npz")


if __name__ == "__main__":
    main()
