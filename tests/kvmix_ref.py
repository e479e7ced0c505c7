"""tests/kvmix_ref.py -- numpy restatement of the reference CPU backend's FLASH_ATTN_EXT over a KV cache whose K and V types differ (TEST INFRASTRUCTURE ONLY).

The CPU's arithmetic is separable (ggml-cpu/ops.cpp:6767-6770, :6793, :6841, :6870): q goes to the K type's vec_dot_type and the scores are the K type's
vec_dot; an f16 V gives the F16 accumulator (ggml_vec_scale_f16 / ggml_vec_mad_f16), any other V the F32 accumulator over V's to_float.  So the pieces are
the ones the same-type restatements already have -- oracle.glue (f16, q8_0, q4_0) and tests/kvq_ref.py (q4_1, q5_0, q5_1, iq4_nl) -- and this file only pairs
them: the score side by kt, the accumulator side by vt.  With kt == vt it is those restatements again, bit for bit (tests/test_kvmix_ref_cpu.py).
powf / tanhf / expf are the C library's, as on the CPU.  Arrays use numpy order = ggml dims reversed; a cache side is an f16 array [B, Hk, n_kv, D] (or its
bytes, uint8 [..., 2 D]) for "f16" and uint8 block rows [B, Hk, n_kv, D / 32 * BB] otherwise."""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

import kvq_ref
from oracle import glue

f32 = np.float32
f64 = np.float64
TYPES = ["f16", "q8_0", "q4_0", "q4_1", "q5_0", "q5_1", "iq4_nl"]
BLOCK_BYTES = {"f16": 64, "q8_0": 34, "q4_0": 18, "q4_1": 20, "q5_0": 22, "q5_1": 24, "iq4_nl": 18}
RING = [("f16", "q8_0"), ("q8_0", "q4_0"), ("q4_0", "q4_1"), ("q4_1", "q5_0"), ("q5_0", "q5_1"), ("q5_1", "iq4_nl"), ("iq4_nl", "f16")]

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _fn, _n in (("expf", 1), ("tanhf", 1), ("powf", 2)):
    getattr(_libm, _fn).restype = ctypes.c_float; getattr(_libm, _fn).argtypes = [ctypes.c_float] * _n


def _as_f16(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.float16) if a.dtype == np.uint8 else a.astype(np.float16)


def _unpack_q80_q40(kv: str, blk: np.ndarray):
    """(d f16 [..., nb], q int8 [..., nb, 32]) as oracle.glue.flash_attn_ext_q8_0 reads block_q8_0 / block_q4_0"""
    bb = BLOCK_BYTES[kv]
    b = np.ascontiguousarray(blk).reshape(blk.shape[:-1] + (blk.shape[-1] // bb, bb))
    d = np.ascontiguousarray(b[..., :2]).view(np.float16)[..., 0]
    if kv == "q8_0":
        return d, np.ascontiguousarray(b[..., 2:]).view(np.int8)
    qs = b[..., 2:].astype(np.int16)
    return d, np.concatenate([(qs & 15) - 8, (qs >> 4) - 8], axis=-1).astype(np.int8)


class _Scores:
    """the K side of one (batch, kv head): dots(q_row) -> [n_kv] f32 before the scale"""
    def __init__(self, kt: str, k_head: np.ndarray):
        self.kt = kt
        if kt == "f16":
            self.k = _as_f16(k_head).astype(f64)
        elif kt in ("q8_0", "q4_0"):
            self.kd, self.kq = _unpack_q80_q40(kt, k_head)
        else:
            self.kd, self.km, self.kq = kvq_ref.unpack(kt, k_head)

    def dots(self, q_row: np.ndarray) -> np.ndarray:
        if self.kt == "f16":
            return glue.vec_dot_f16_simd(self.k, q_row.astype(np.float16).astype(f64))
        if self.kt in ("q8_0", "q4_0"):
            qd, qq = glue.quantize_row_q8_0_simd(q_row)
            return glue.vec_dot_q8_0_q8_0_simd(self.kd, self.kq, qd, qq)
        qd, qs, qq = kvq_ref.quantize_q(q_row, self.kt in ("q4_1", "q5_1"))
        return kvq_ref.vec_dot(self.kt, self.kd, self.km, self.kq, qd, qs, qq)


def v_values(vt: str, v_head: np.ndarray) -> np.ndarray:
    """the V side of one (batch, kv head) as the accumulator reads it: f16 values, or to_float's f32 -> f64 [n_kv, DV]"""
    if vt == "f16":
        return _as_f16(v_head).astype(f64)
    if vt in ("q8_0", "q4_0"):
        vd, vq = _unpack_q80_q40(vt, v_head)
        y = (vq.astype(f32) * vd.astype(f32)[..., None]).astype(f32)
        return y.reshape(y.shape[0], -1).astype(f64)
    return kvq_ref.dequantize(vt, v_head).astype(f64)


def flash_attn_ext(kt: str, vt: str, q: np.ndarray, k: np.ndarray, v: np.ndarray, mask, scale: float, max_bias: float = 0.0,
                   logit_softcap: float = 0.0) -> np.ndarray:
    """q [B, H, N, DK] f32; k of type kt, v of type vt (see the module docstring); mask [>= N, n_kv] f16 or None -> [B, N, H, DV] f32."""
    q = np.asarray(q, f32)
    B, H, N, DK = q.shape
    Hk, n_kv, Hv = k.shape[1], k.shape[2], v.shape[1]
    n_head_log2 = 1 << int(np.floor(np.log2(H)))
    m0 = f32(_libm.powf(2.0, float(f32(-(max_bias) / n_head_log2)))); m1 = f32(_libm.powf(2.0, float(f32(-(max_bias / 2.0) / n_head_log2))))
    sc = f32(scale)
    if logit_softcap != 0.0:
        sc = f32(sc / f32(logit_softcap))
    out = None
    for b in range(B):
        for h in range(H):
            slope = f32(1.0)
            if max_bias > 0.0:
                slope = f32(_libm.powf(float(m0), float(h + 1))) if h < n_head_log2 else f32(_libm.powf(float(m1), float(2 * (h - n_head_log2) + 1)))
            ks = _Scores(kt, k[b, h // (H // Hk)])
            vh = v_values(vt, v[b, h // (H // Hv)])
            DV = vh.shape[1]
            if out is None:
                out = np.zeros((B, N, H, DV), f32)
            for n in range(N):
                dots = ks.dots(q[b, h, n])
                S = f32(0.0); M = f32(-np.inf)
                acc = np.zeros(DV, np.float16 if vt == "f16" else f32)
                for j in range(n_kv):
                    mv = f32(slope * f32(mask[n, j])) if mask is not None else f32(0.0)
                    if mv == -np.inf:
                        continue                                                          # a masked position is skipped whatever its rows hold
                    s = f32(dots[j] * sc)
                    if logit_softcap != 0.0:
                        s = f32(f32(logit_softcap) * f32(_libm.tanhf(float(s))))
                    s = f32(s + mv)
                    ms = f32(1.0); vs = f32(1.0)
                    if s > M:
                        Mold = M; M = s
                        ms = f32(_libm.expf(float(f32(Mold - M))))
                        acc = (acc.astype(f32) * ms).astype(acc.dtype)                    # ggml_vec_scale_f16 / _f32
                    else:
                        vs = f32(_libm.expf(float(f32(s - M))))
                    acc = (vh[j] * f64(vs) + acc.astype(f64)).astype(f32).astype(acc.dtype)     # ggml_vec_mad_f16 / _f32: an f32 fma (then f16)
                    S = f32(f32(S * ms) + vs)
                out[b, n, h] = acc.astype(f32) * f32(f32(1.0) / S)
    return out
