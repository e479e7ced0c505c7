#!/usr/bin/env python3
"""Generate tests/golden/kvq_*.npz from the REAL reference (oracle/_ref/avx2, the x86-64-v3 build): a Q4_1 / Q5_0 / Q5_1 / IQ4_NL KV cache
(-ctk T -ctv T).  Per type T:
  * kvq_T_store.npz   f32 rows -> the blocks CPY f32 -> T stores (the type's from_float = its `_ref` row quantizer; for IQ4_NL this is NOT what
                      ggml_quantize_chunk writes): an all-zero block, an all-tiny one (IQ4_NL's GROUP_MAX_EPS branch, first and later in a row),
                      magnitude ties of both signs, values on the rounding ties of x * id + 0.5 / + 8.5 / + 16.5, code-book midpoints, random rows
  * kvq_T_fa_*.npz    FLASH_ATTN_EXT (ggml-cpu/ops.cpp:6686-6905) with the cache bytes the reference attended to
  * kvq_T_loop.npz    a 24-step decode: the output of every step over the growing window
  * kvq_T_long_kv8192.npz   the longest window accepted: inputs from a seed, the output and a digest of the cache bytes (IQ4_NL: the digest of the
                            rows from_float stores, no output -- see main())
Run where the reference sources exist:  python tests/golden/make_kvq_golden.py   (arrays only: loadable with allow_pickle=False)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import oracle  # noqa: E402
from kvq_ref import TYPES, KVALUES_IQ4NL  # noqa: E402

OUT = Path(__file__).resolve().parent


def store_inputs(kv: str) -> np.ndarray:
    """rows of 128 elements (4 blocks)"""
    rng = np.random.default_rng(TYPES[kv][0])
    rows = [rng.standard_normal(128).astype(np.float32) * s for s in (1.0, 1e-3, 37.5, 1e4)]
    r = rng.standard_normal(128).astype(np.float32); r[:32] = 0.0; rows.append(r)                        # an all-zero block first in the row
    r = rng.standard_normal(128).astype(np.float32); r[64:96] = 0.0; rows.append(r)                      # ... and later
    r = rng.standard_normal(128).astype(np.float32); r[:32] = rng.standard_normal(32).astype(np.float32) * 1e-17; rows.append(r)     # all tiny, first
    r = rng.standard_normal(128).astype(np.float32); r[32:64] = rng.standard_normal(32).astype(np.float32) * 1e-17; r[96:] = 3e-16; rows.append(r)
    rows.append(np.zeros(128, np.float32))
    # magnitude ties of both signs: the first holder decides the sign of the scale
    for a, b in ((2.5, -2.5), (-2.5, 2.5)):
        r = (rng.uniform(-1, 1, 128)).astype(np.float32)
        for blk, (i, j) in enumerate(((3, 20), (17, 30), (0, 31), (9, 10))):
            r[32 * blk + i] = a; r[32 * blk + j] = b
        rows.append(r)
    # exact rounding ties: a block spanning [-16, 15] / [0, 15] / [0, 31] with half-integer members (id is then exactly 1)
    r = np.zeros(128, np.float32)
    r[0:32] = np.arange(32, dtype=np.float32) - 16.0; r[5] = -3.5; r[6] = 2.5; r[7] = 14.5; r[8] = -15.5            # q5_0: d = 1 (max = -16)
    r[32:64] = np.arange(32, dtype=np.float32) % 16 - 8.0; r[32 + 16] = -8.0; r[32 + 3] = -0.5; r[32 + 4] = 6.5; r[32 + 20] = 7.5      # q4_0-like
    r[64:96] = np.arange(32, dtype=np.float32); r[64 + 3] = 2.5; r[64 + 4] = 29.5; r[64 + 20] = 30.5                # q5_1: min 0, max 31
    r[96:128] = np.arange(32, dtype=np.float32) % 16; r[96 + 3] = 2.5; r[96 + 4] = 13.5; r[96 + 20] = 14.5          # q4_1: min 0, max 15
    rows.append(r)
    # code-book midpoints (iq4_nl): a block whose extreme is -127 so that id = 1, members halfway between neighbouring entries
    kvs = KVALUES_IQ4NL.astype(np.float32)
    r = np.zeros(128, np.float32)
    for blk, sgn in enumerate((1.0, -1.0, 1.0, -1.0)):
        b = np.zeros(32, np.float32); b[0] = -127.0
        b[1:16] = (kvs[:-1] + kvs[1:]) / 2; b[16:32] = kvs
        if blk >= 2:
            b[1:16] += np.float32(0.25) * (1 if blk == 2 else -1)
        r[32 * blk:32 * blk + 32] = sgn * b
    rows.append(r)
    return np.stack(rows)


def from_float(ref, fn: str, t: int, bb: int, x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((x.shape[0], x.shape[1] // 32 * bb), np.uint8)
    for i in range(x.shape[0]):
        getattr(ref.lib, fn)(t, oracle._ptr(x[i]), oracle._ptr(out[i]), x.shape[1])
    return out


def fa(ref, t: int, bb: int, q, kf, vf, mask, scale, max_bias=0.0, softcap=0.0):
    q = np.ascontiguousarray(q, np.float32); kf = np.ascontiguousarray(kf, np.float32); vf = np.ascontiguousarray(vf, np.float32)
    ne = lambda a: np.asarray(list(a.shape)[::-1], np.int64)
    m = np.ascontiguousarray(mask, np.float32) if mask is not None else None
    out = np.empty((q.shape[0], q.shape[2], q.shape[1], vf.shape[3]), np.float32)
    kb = np.empty(kf.shape[:-1] + (kf.shape[-1] // 32 * bb,), np.uint8); vb = np.empty(vf.shape[:-1] + (vf.shape[-1] // 32 * bb,), np.uint8)
    rc = ref.lib.ref_flash_attn_ext_t(oracle._ptr(q), oracle._ptr(ne(q)), oracle._ptr(kf), oracle._ptr(ne(kf)), oracle._ptr(vf), oracle._ptr(ne(vf)),
                                      oracle._ptr(m) if m is not None else None, m.shape[0] if m is not None else 0, scale, max_bias, softcap, t,
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
    "decode_gqa_d256_kv128": (4, 2, 1, 256, 128, 100, 0.0, 0.0),
    "decode_nomask_d64_kv1": (4, 4, 1, 64, 1, None, 0.0, 0.0),
    "batch3_d96_kv40": (4, 2, 3, 96, 40, 35, 0.0, 0.0),                 # head size 96: an odd block count (IQ4_NL's scalar tail)
    "alibi_d128_kv64": (8, 8, 2, 128, 64, 60, 8.0, 0.0),
    "softcap_d96_kv64": (4, 1, 1, 96, 64, 64, 0.0, 10.0),
    "prefill_gqa_d128_kv256": (4, 2, 48, 128, 256, 200, 0.0, 0.0),      # >= 16 queries: the f16-scratch route when the workspace is given
}


def main() -> None:
    ref = oracle.Reference("avx2")
    for kv, (t, bb, _flag) in TYPES.items():
        x = store_inputs(kv)
        blocks = from_float(ref, "ref_from_float_ref", t, bb, x)
        cpu = from_float(ref, "ref_from_float_cpu", t, bb, x)
        if kv == "iq4_nl":
            # an all-small block (amax < GROUP_MAX_EPS): quantize_row_iq4_nl_impl stores d = 0 and then packs an index array it never wrote for
            # this block (ggml-quants.c:4604-4607, :4677-4681) -- the previous block's indices, or whatever the stack held for the first block
            # of a call; the two entry points differ there.  Only d = 0 is defined: the fixture keeps zero index bytes, the value either way.
            small = np.abs(x.reshape(x.shape[0], -1, 32)).max(axis=-1) < np.float32(1e-15)
            for o in (blocks, cpu):
                b3 = o.reshape(o.shape[0], -1, bb)
                assert (b3[small][:, :2] == 0).all()
                b3[small] = 0
        assert np.array_equal(blocks, cpu), kv                                                          # the CPU backend's from_float IS the _ref quantizer
        np.savez_compressed(OUT / f"kvq_{kv}_store.npz", x=x, blocks=blocks)
        for tag, (H, Hk, N, DK, n_kv, first_masked, max_bias, softcap) in FA_CASES.items():
            rng = np.random.default_rng(sum(map(ord, tag)) + t)
            q = rng.standard_normal((1, H, N, DK)).astype(np.float32)
            kf = rng.standard_normal((1, Hk, n_kv, DK)).astype(np.float32); vf = rng.standard_normal((1, Hk, n_kv, DK)).astype(np.float32)
            mask = causal_mask(N, n_kv, first_masked, rng, max_bias > 0) if first_masked is not None else None
            scale = np.float32(1.0 / np.sqrt(DK))
            y, kb, vb = fa(ref, t, bb, q, kf, vf, mask, float(scale), max_bias, softcap)
            assert np.isfinite(y).all()
            extra = {"mask": mask} if mask is not None else {}
            np.savez_compressed(OUT / f"kvq_{kv}_fa_{tag}.npz", q=q, k=kb, v=vb, scale=scale, max_bias=np.float32(max_bias), softcap=np.float32(softcap), y=y, **extra)
        rng = np.random.default_rng(8192 + t)
        q = rng.standard_normal((1, 2, 1, 64)).astype(np.float32)
        kf = rng.standard_normal((1, 1, 8192, 64)).astype(np.float32); vf = rng.standard_normal((1, 1, 8192, 64)).astype(np.float32)
        mask = causal_mask(1, 8192, 8000)
        y, kb, vb = fa(ref, t, bb, q, kf, vf, mask, 0.125)
        digest = lambda a: np.uint64(a.astype(np.uint64).sum())
        if kv == "iq4_nl":
            # the cache the reference attended to is ggml_quantize_chunk's (a seven-try search), which a CPY never writes: its output is of no use to
            # a test.  The digests are those of the rows from_float stores, what the device's CPY must write.
            kr = from_float(ref, "ref_from_float_ref", t, bb, kf.reshape(-1, 64)); vr = from_float(ref, "ref_from_float_ref", t, bb, vf.reshape(-1, 64))
            np.savez_compressed(OUT / f"kvq_{kv}_long_kv8192.npz", seed=np.int64(8192 + t), k_sum=digest(kr), v_sum=digest(vr))
        else:
            np.savez_compressed(OUT / f"kvq_{kv}_long_kv8192.npz", seed=np.int64(8192 + t), y=y, k_sum=digest(kb), v_sum=digest(vb))
        # a 24-step decode: token s attends to positions 0 .. s of a cache quantized by ggml_quantize_chunk inside fa() (the row quantizer, what CPY
        # writes, for Q4_1 / Q5_0 / Q5_1; another quantizer for IQ4_NL, whose cache bytes are therefore part of the fixture's inputs only)
        rng = np.random.default_rng(24 + t)
        H, Hk, D, steps = 4, 2, 64, 24
        qs = rng.standard_normal((steps, 1, H, 1, D)).astype(np.float32)
        kf = rng.standard_normal((1, Hk, steps, D)).astype(np.float32); vf = rng.standard_normal((1, Hk, steps, D)).astype(np.float32)
        ys = []
        for s in range(steps):
            y, kb, vb = fa(ref, t, bb, qs[s], kf[:, :, :s + 1], vf[:, :, :s + 1], causal_mask(1, s + 1, s + 1), 0.125)
            ys.append(y)
        np.savez_compressed(OUT / f"kvq_{kv}_loop.npz", q=qs, kf=kf, vf=vf, y=np.stack(ys), k=kb, v=vb)
    print("wrote kvq fixtures to", OUT)


if __name__ == "__main__":
    main()
