#!/usr/bin/env python3
"""Generate tests/golden/bf16_kv_*.npz from the REAL reference (oracle/_ref/avx2, the x86-64-v3 build): a bf16 KV cache (-ctk bf16 -ctv bf16).
  * bf16_kv_convert.npz   f32 values with NaNs, infinities, subnormals and exact ties -> the reference's bf16 bits (from_float of GGML_TYPE_BF16)
  * bf16_kv_mul_mat.npz   MUL_MAT with a bf16 src0 (ggml_vec_dot_bf16 after rounding src1 to bf16): decode widths N = 1..8, K = 128 / 100 / 8
                          (the tail past the last 32-chunk), a GQA broadcast, the transposed V view of the -fa 0 graph, and one N = 32 batch
  * bf16_kv_fa_*.npz      FLASH_ATTN_EXT on a bf16 cache (ggml-cpu/ops.cpp:6686-6905) with the cache bytes the reference stores
  * bf16_kv_loop.npz      a 24-step decode: the output of every step over the growing window and the cache bytes
Run where the reference sources exist:  python tests/golden/make_bf16_kv_golden.py   (arrays only: loadable with allow_pickle=False)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import oracle  # noqa: E402

OUT = Path(__file__).resolve().parent
BF16 = 30


def special_values() -> np.ndarray:
    u = [0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFF800001, 0x7F8000FF, 0xFFFFFFFF,          # NaNs: quiet, signalling, payload in the low half only
         0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,                                    # infinities, the largest finite (rounds to inf), a tie there
         0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x00007FFF, 0x007FFFFF, 0x00400000, 0x80400001, # subnormals, their ties
         0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000,                          # ties to even (down, up), just above / below a tie
         0x00000000, 0x80000000, 0x3F800000, 0x3F7FFFFF, 0x33800000]
    rng = np.random.default_rng(5)
    r = rng.integers(0, 2**32, 4096 - len(u), dtype=np.uint64).astype(np.uint32)
    r[::3] = (r[::3] & 0xFFFF0000) | 0x8000                                                               # many exact ties
    return np.concatenate([np.asarray(u, np.uint32), r]).view(np.float32)


def to_bf16(ref, x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty(x.size, np.uint16)
    ref.lib.ref_from_float_ref(BF16, oracle._ptr(x.reshape(-1)), oracle._ptr(out), x.size)
    return out.reshape(x.shape)


def mul_mat(ref, w_bits: np.ndarray, x: np.ndarray) -> np.ndarray:
    """w_bits uint16 [M, K] (bf16), x f32 [N, K] -> [N, M] on the reference CPU backend."""
    M, K = w_bits.shape
    return ref.mul_mat(BF16, np.ascontiguousarray(w_bits), np.ascontiguousarray(x, np.float32), M, x.shape[0], K)


def fa(ref, q, kf, vf, mask, scale, max_bias=0.0, softcap=0.0):
    """FLASH_ATTN_EXT with a bf16 K / V cache made from f32 kf / vf by the reference: (out [B, N, H, DV], k bits, v bits)."""
    q = np.ascontiguousarray(q, np.float32); kf = np.ascontiguousarray(kf, np.float32); vf = np.ascontiguousarray(vf, np.float32)
    ne = lambda a: np.asarray(list(a.shape)[::-1], np.int64)
    m = np.ascontiguousarray(mask, np.float32) if mask is not None else None
    out = np.empty((q.shape[0], q.shape[2], q.shape[1], vf.shape[3]), np.float32)
    kb = np.empty(kf.shape, np.uint16); vb = np.empty(vf.shape, np.uint16)                             # 2 bytes per element
    rc = ref.lib.ref_flash_attn_ext_t(oracle._ptr(q), oracle._ptr(ne(q)), oracle._ptr(kf), oracle._ptr(ne(kf)), oracle._ptr(vf), oracle._ptr(ne(vf)),
                                      oracle._ptr(m) if m is not None else None, m.shape[0] if m is not None else 0, scale, max_bias, softcap, BF16,
                                      oracle._ptr(out), oracle._ptr(kb), oracle._ptr(vb), 1)
    assert rc == 0, rc
    return out, kb, vb


def causal_mask(N: int, n_kv: int, first_masked: int, rng=None, alibi: bool = False) -> np.ndarray:
    mask = np.zeros((64 if N <= 64 else N, n_kv), np.float32)                                           # rows padded to GGML_KQ_MASK_PAD
    for t in range(N):
        mask[t, first_masked + t:] = -np.inf
    if alibi:
        mask[:N] += (rng.standard_normal((N, n_kv)) * 0.1).astype(np.float16).astype(np.float32)
    return mask.astype(np.float16)


# tag: (n_head, n_head_kv, n_queries, head_dim, n_kv, first masked position of query 0 (None: no mask), max_bias, logit_softcap)
FA_CASES = {
    "decode_gqa_d128_kv256": (8, 2, 1, 128, 256, 201, 0.0, 0.0),
    "decode_nomask_d64_kv1": (4, 4, 1, 64, 1, None, 0.0, 0.0),
    "batch3_d80_kv40": (4, 2, 3, 80, 40, 35, 0.0, 0.0),                 # head size 80: a tail of 16 past the last 32-chunk
    "alibi_d128_kv64": (8, 8, 2, 128, 64, 60, 8.0, 0.0),
    "softcap_d96_kv64": (4, 1, 1, 96, 64, 64, 0.0, 10.0),
    "prefill_gqa_d128_kv256": (4, 2, 48, 128, 256, 200, 0.0, 0.0),      # >= 16 queries: the matrix-core path when the workspace is given
}


def main() -> None:
    ref = oracle.Reference("avx2")
    # ---- conversion
    x = special_values()
    np.savez_compressed(OUT / "bf16_kv_convert.npz", x=x, bits=to_bf16(ref, x))
    # ---- MUL_MAT
    rng = np.random.default_rng(11)
    mm = {}
    for K in (128, 100, 8):
        w = to_bf16(ref, rng.standard_normal((40, K)).astype(np.float32))
        xs = rng.standard_normal((8, K)).astype(np.float32)
        mm[f"w_k{K}"] = w; mm[f"x_k{K}"] = xs
        for N in range(1, 9):
            mm[f"y_k{K}_n{N}"] = mul_mat(ref, w, xs[:N])
    # GQA: src0 [2 kv heads, 24, 64] broadcast over 4 heads of src1 [4, 3, 64]
    w = to_bf16(ref, rng.standard_normal((2, 24, 64)).astype(np.float32)); xs = rng.standard_normal((4, 3, 64)).astype(np.float32)
    mm["w_gqa"] = w; mm["x_gqa"] = xs; mm["y_gqa"] = np.stack([mul_mat(ref, w[h // 2], xs[h]) for h in range(4)])
    # transposed V: a cache [2 kv heads, DV = 32, n_ctx = 96] (each row one output dim over the positions), the product over the first n_kv = 70 positions
    cache = to_bf16(ref, rng.standard_normal((2, 32, 96)).astype(np.float32)); kq = rng.standard_normal((4, 2, 70)).astype(np.float32)
    mm["cache_vt"] = cache; mm["x_vt"] = kq; mm["y_vt"] = np.stack([mul_mat(ref, cache[h // 2, :, :70], kq[h]) for h in range(4)])
    # a batch: the matrix-core path
    w = to_bf16(ref, rng.standard_normal((64, 256)).astype(np.float32)); xs = rng.standard_normal((32, 256)).astype(np.float32)
    mm["w_batch"] = w; mm["x_batch"] = xs; mm["y_batch"] = mul_mat(ref, w, xs)
    np.savez_compressed(OUT / "bf16_kv_mul_mat.npz", **mm)
    # ---- FLASH_ATTN_EXT
    for tag, (H, Hk, N, DK, n_kv, first_masked, max_bias, softcap) in FA_CASES.items():
        rng = np.random.default_rng(sum(map(ord, tag)))
        q = rng.standard_normal((1, H, N, DK)).astype(np.float32)
        kf = rng.standard_normal((1, Hk, n_kv, DK)).astype(np.float32); vf = rng.standard_normal((1, Hk, n_kv, DK)).astype(np.float32)
        mask = causal_mask(N, n_kv, first_masked, rng, max_bias > 0) if first_masked is not None else None
        scale = np.float32(1.0 / np.sqrt(DK))
        y, kb, vb = fa(ref, q, kf, vf, mask, float(scale), max_bias, softcap)
        assert np.isfinite(y).all()
        extra = {"mask": mask} if mask is not None else {}
        np.savez_compressed(OUT / f"bf16_kv_fa_{tag}.npz", q=q, k=kb, v=vb, scale=scale, max_bias=np.float32(max_bias), softcap=np.float32(softcap), y=y, **extra)
    # the longest window accepted (8192 positions): inputs from a seed (a 2 MB cache is not stored), the output and a digest of the cache bytes
    rng = np.random.default_rng(8192)
    q = rng.standard_normal((1, 2, 1, 64)).astype(np.float32)
    kf = rng.standard_normal((1, 1, 8192, 64)).astype(np.float32); vf = rng.standard_normal((1, 1, 8192, 64)).astype(np.float32)
    mask = causal_mask(1, 8192, 8000)
    y, kb, vb = fa(ref, q, kf, vf, mask, 0.125)
    np.savez_compressed(OUT / "bf16_kv_long_kv8192.npz", seed=np.int64(8192), y=y, k_sum=np.uint64(kb.astype(np.uint64).sum()), v_sum=np.uint64(vb.astype(np.uint64).sum()))
    # ---- a 24-step decode: token t stores its K / V row at position t of a 32-position cache and attends to positions 0 .. t
    rng = np.random.default_rng(24)
    H, Hk, D, n_ctx, steps = 4, 2, 64, 32, 24
    qs = rng.standard_normal((steps, 1, H, 1, D)).astype(np.float32)
    kf = rng.standard_normal((1, Hk, steps, D)).astype(np.float32); vf = rng.standard_normal((1, Hk, steps, D)).astype(np.float32)
    ys = []
    for t in range(steps):
        mask = causal_mask(1, t + 1, t + 1)
        y, kb, vb = fa(ref, qs[t], kf[:, :, :t + 1], vf[:, :, :t + 1], mask, 0.125)
        ys.append(y)
    np.savez_compressed(OUT / "bf16_kv_loop.npz", q=qs, kf=kf, vf=vf, y=np.stack(ys), k=kb, v=vb, n_ctx=np.int64(n_ctx))
    print("wrote bf16_kv fixtures to", OUT)


if __name__ == "__main__":
    main()
