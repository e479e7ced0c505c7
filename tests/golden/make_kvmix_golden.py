#!/usr/bin/env python3
"""Generate tests/golden/kvmix_*.npz from the REAL reference (oracle/_ref/avx2, the x86-64-v3 build): FLASH_ATTN_EXT over a KV cache whose K and V have
different types (-ctk A -ctv B), each of f16, q8_0, q4_0, q4_1, q5_0, q5_1, iq4_nl.

oracle/refshim takes one cache type for both sides, so this file drives the reference's own C API through ctypes -- ggml_init, ggml_new_tensor_4d,
ggml_quantize_chunk / ggml_fp32_to_fp16_row, ggml_flash_attn_ext, ggml_new_graph, ggml_build_forward_expand, ggml_graph_compute_with_ctx, ggml_get_data --
on the already built libggml-base.so / libggml-cpu.so.  One thread: the op's result does not depend on the split, and the run is reproducible.

  * kvmix_all_pairs_d64_kv96.npz    all 42 ordered pairs at B = 1, H = 2, Hk = 1, N = 2, DK = DV = 64, n_kv = 96: ONE q, ONE f32 K and V, a causal-style mask
                                    with a fully masked position in the middle; per type the cache bytes as stored (k_T, v_T), per pair the output (y_K_V)
  * kvmix_<K>_<V>_<tag>.npz         the ring of seven pairs, every type once on each side, at the shapes of the same-type fixtures: q, k, v (the cache bytes as
                                    stored), mask, the scalars and y -- a file per pair, the layout of the kvq_* fixtures

Run where oracle/_ref is built:  python tests/golden/make_kvmix_golden.py   (arrays only: loadable with allow_pickle=False)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent

# name -> (ggml type id, bytes per 32 elements)
TYPES = {"f16": (1, 64), "q8_0": (8, 34), "q4_0": (2, 18), "q4_1": (3, 20), "q5_0": (6, 22), "q5_1": (7, 24), "iq4_nl": (20, 18)}
RING = [("f16", "q8_0"), ("q8_0", "q4_0"), ("q4_0", "q4_1"), ("q4_1", "q5_0"), ("q5_0", "q5_1"), ("q5_1", "iq4_nl"), ("iq4_nl", "f16")]
# tag: (n_head, n_head_kv, n_queries, DK, DV, n_kv, first masked position of query 0 (None: no mask), max_bias, logit_softcap)
RING_CASES = {
    "decode_gqa_d128_kv256": (8, 2, 1, 128, 128, 256, 201, 0.0, 0.0),
    "batch3_dk64_dv96_kv40_alibi": (4, 2, 3, 64, 96, 40, 35, 8.0, 0.0),
    "softcap_d96_kv64": (4, 1, 1, 96, 96, 64, 64, 0.0, 10.0),
    "decode_nomask_d64_kv1": (4, 4, 1, 64, 64, 1, None, 0.0, 0.0),
}
GGML_TYPE_F32 = 0


class InitParams(C.Structure):
    _fields_ = [("mem_size", C.c_size_t), ("mem_buffer", C.c_void_p), ("no_alloc", C.c_bool)]


class Ref:
    def __init__(self, variant: str = "avx2"):
        d = ROOT / "oracle" / "_ref" / variant
        self.base = C.CDLL(str(d / "libggml-base.so"), mode=C.RTLD_GLOBAL)
        self.cpu = C.CDLL(str(d / "libggml-cpu.so"), mode=C.RTLD_GLOBAL)
        b, c, vp, i64 = self.base, self.cpu, C.c_void_p, C.c_int64
        b.ggml_init.restype = vp; b.ggml_init.argtypes = [InitParams]
        b.ggml_free.argtypes = [vp]
        b.ggml_new_tensor_4d.restype = vp; b.ggml_new_tensor_4d.argtypes = [vp, C.c_int, i64, i64, i64, i64]
        b.ggml_get_data.restype = vp; b.ggml_get_data.argtypes = [vp]
        b.ggml_nbytes.restype = C.c_size_t; b.ggml_nbytes.argtypes = [vp]
        b.ggml_quantize_chunk.restype = C.c_size_t; b.ggml_quantize_chunk.argtypes = [C.c_int, vp, vp, i64, i64, i64, vp]
        b.ggml_fp32_to_fp16_row.argtypes = [vp, vp, i64]
        b.ggml_flash_attn_ext.restype = vp; b.ggml_flash_attn_ext.argtypes = [vp, vp, vp, vp, vp, C.c_float, C.c_float, C.c_float]
        b.ggml_new_graph.restype = vp; b.ggml_new_graph.argtypes = [vp]
        b.ggml_build_forward_expand.argtypes = [vp, vp]
        c.ggml_graph_compute_with_ctx.restype = C.c_int; c.ggml_graph_compute_with_ctx.argtypes = [vp, vp, C.c_int]
        if hasattr(c, "ggml_cpu_init"):
            c.ggml_cpu_init()

    def to_type(self, name: str, x: np.ndarray) -> np.ndarray:
        """f32 [..., n] -> the bytes of `name` rows, uint8 [..., n / 32 * bytes] (f16: ggml_fp32_to_fp16_row; a block type: ggml_quantize_chunk)"""
        t, bb = TYPES[name]
        x = np.ascontiguousarray(x, np.float32)
        n = x.shape[-1]; rows = x.size // n
        out = np.empty(x.shape[:-1] + (n // 32 * bb,), np.uint8)
        if name == "f16":
            self.base.ggml_fp32_to_fp16_row(x.ctypes.data, out.ctypes.data, x.size)
        else:
            got = self.base.ggml_quantize_chunk(t, x.ctypes.data, out.ctypes.data, 0, rows, n, None)
            assert got == out.size, (got, out.size)
        return out

    def flash_attn_ext(self, q, kt, kbytes, vt, vbytes, mask, scale, max_bias=0.0, softcap=0.0) -> np.ndarray:
        """q f32 [B, H, N, DK]; kbytes / vbytes uint8 [B, Hk, n_kv, row bytes] of types kt / vt; mask f16 [rows >= pad(N, 64), n_kv] or None -> [B, N, H, DV]"""
        b = self.base
        B, H, N, DK = q.shape
        Hk, n_kv = kbytes.shape[1], kbytes.shape[2]
        DV = vbytes.shape[3] // TYPES[vt][1] * 32
        ctx = b.ggml_init(InitParams(64 << 20, None, False))
        assert ctx
        try:
            def tensor(t, ne, data):
                p = b.ggml_new_tensor_4d(ctx, t, *ne)
                data = np.ascontiguousarray(data)
                assert b.ggml_nbytes(p) == data.nbytes, (b.ggml_nbytes(p), data.nbytes)
                C.memmove(b.ggml_get_data(p), data.ctypes.data, data.nbytes)
                return p
            tq = tensor(GGML_TYPE_F32, (DK, N, H, B), np.asarray(q, np.float32))
            tk = tensor(TYPES[kt][0], (DK, n_kv, Hk, B), kbytes)
            tv = tensor(TYPES[vt][0], (DV, n_kv, Hk, B), vbytes)
            tm = tensor(1, (n_kv, mask.shape[0], 1, 1), np.asarray(mask, np.float16)) if mask is not None else None
            out = b.ggml_flash_attn_ext(ctx, tq, tk, tv, tm, scale, max_bias, softcap)
            g = b.ggml_new_graph(ctx)
            b.ggml_build_forward_expand(g, out)
            assert self.cpu.ggml_graph_compute_with_ctx(ctx, g, 1) == 0
            y = np.empty((B, N, H, DV), np.float32)
            assert b.ggml_nbytes(out) == y.nbytes
            C.memmove(y.ctypes.data, b.ggml_get_data(out), y.nbytes)
            return y
        finally:
            b.ggml_free(ctx)


def causal_mask(N: int, n_kv: int, first_masked: int, rng=None, alibi: bool = False) -> np.ndarray:
    mask = np.zeros((64 if N <= 64 else N, n_kv), np.float32)                                           # rows padded to GGML_KQ_MASK_PAD
    for t in range(N):
        mask[t, first_masked + t:] = -np.inf
    if alibi:
        mask[:N] += (rng.standard_normal((N, n_kv)) * 0.1).astype(np.float16).astype(np.float32)
    return mask.astype(np.float16)


def all_pairs(ref: Ref) -> None:
    rng = np.random.default_rng(4242)
    H, Hk, N, D, n_kv = 2, 1, 2, 64, 96
    q = rng.standard_normal((1, H, N, D)).astype(np.float32)
    kf = rng.standard_normal((1, Hk, n_kv, D)).astype(np.float32); vf = rng.standard_normal((1, Hk, n_kv, D)).astype(np.float32)
    mask = causal_mask(N, n_kv, 90)
    mask[:, 41] = -np.inf                                                                               # a fully masked position in the middle
    scale = np.float32(1.0 / np.sqrt(D))
    arrs = dict(q=q, mask=mask, scale=scale, max_bias=np.float32(0), softcap=np.float32(0))
    cache = {}
    for t in TYPES:
        cache[t] = (ref.to_type(t, kf), ref.to_type(t, vf))
        arrs[f"k_{t}"], arrs[f"v_{t}"] = cache[t]
    for kt in TYPES:
        for vt in TYPES:
            if kt != vt:
                arrs[f"y_{kt}_{vt}"] = ref.flash_attn_ext(q, kt, cache[kt][0], vt, cache[vt][1], mask, float(scale))
    np.savez_compressed(OUT / "kvmix_all_pairs_d64_kv96.npz", **arrs)


def ring(ref: Ref) -> None:
    for tag, (H, Hk, N, DK, DV, n_kv, first_masked, max_bias, softcap) in RING_CASES.items():
        rng = np.random.default_rng(sum((H, Hk, N, DK, DV, n_kv)))
        q = rng.standard_normal((1, H, N, DK)).astype(np.float32)
        kf = rng.standard_normal((1, Hk, n_kv, DK)).astype(np.float32); vf = rng.standard_normal((1, Hk, n_kv, DV)).astype(np.float32)
        mask = causal_mask(N, n_kv, first_masked, rng, alibi=max_bias > 0) if first_masked is not None else None
        scale = np.float32(1.0 / np.sqrt(DK))
        for kt, vt in RING:
            kb, vb = ref.to_type(kt, kf), ref.to_type(vt, vf)
            arrs = dict(q=q, k=kb, v=vb, scale=scale, max_bias=np.float32(max_bias), softcap=np.float32(softcap))
            if mask is not None:
                arrs["mask"] = mask
            arrs["y"] = ref.flash_attn_ext(q, kt, kb, vt, vb, mask, float(scale), max_bias, softcap)
            np.savez_compressed(OUT / f"kvmix_{kt}_{vt}_{tag}.npz", **arrs)


def main() -> None:
    ref = Ref("avx2")
    all_pairs(ref)
    ring(ref)
    for f in sorted(OUT.glob("kvmix_*.npz")):
        print(f.name, f.stat().st_size)


if __name__ == "__main__":
    sys.exit(main())
