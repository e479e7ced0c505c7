"""tests/kvq_ref.py -- numpy restatement of the reference CPU backend's arithmetic on a Q4_1 / Q5_0 / Q5_1 / IQ4_NL KV cache (TEST INFRASTRUCTURE ONLY).

What a cache of these types goes through on the CPU, each piece following the function it cites, in the x86-64-v3 (AVX2 + FMA) build's order:
  stores   CPY f32 -> type = the type's from_float, which is the `_ref` row quantizer (ggml-quants.c:68-190, :4573-4720)
  q        quantized to the K type's vec_dot_type by the SIMD quantizer (ggml-cpu-quants.c:738 ff. Q8_0, :1053 ff. Q8_1)
  scores   ggml_vec_dot_q4_1_q8_1 (:2749-2782), _q5_0_q8_0 (:3076-3098), _q5_1_q8_1 (:3409-3434), _iq4_nl_q8_0 (:12498-12525 + tail :12653-12661)
  softmax  the ordered walk of ggml_compute_forward_flash_attn_ext_f16 (ggml-cpu/ops.cpp:6686-6905)
  V . P    dequantize_row_* (ggml-quants.c:275-345, :2436-2452) into an F32 accumulator, ggml_vec_scale_f32 / ggml_vec_mad_f32
ggml-quants.c and ggml-cpu-quants.c are C files built as ISO C (-std=c11), where gcc contracts nothing: every scalar `a * b + c` in them is a rounded
product and a rounded sum in BOTH reference builds (only the fmadd intrinsics fuse).  ops.cpp / vec.cpp are C++, contracted in the AVX2 build (the fma of
ggml_vec_mad_f32).  Pinned bit for bit by tests/test_kvq_golden.py against tests/golden/kvq_*.npz and, where it is built, the live reference.
Arrays use numpy order = ggml dims reversed."""
from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

f32 = np.float32
f64 = np.float64

# name -> (ggml type id, bytes per 32-element block, mi355q stage flag)
TYPES = {"q4_1": (3, 20, 0x10), "q5_0": (6, 22, 0x20), "q5_1": (7, 24, 0x40), "iq4_nl": (20, 18, 0x80)}
KVALUES_IQ4NL = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int8)      # ggml-common.h kvalues_iq4nl
GROUP_MAX_EPS = f32(1e-15)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float; _libm.expf.argtypes = [ctypes.c_float]
_libm.tanhf.restype = ctypes.c_float; _libm.tanhf.argtypes = [ctypes.c_float]


def block_bytes(kv: str) -> int:
    return TYPES[kv][1]


# ---------------------------------------------------------------------------------------------------------------- stores
def _first_absmax(xb: np.ndarray) -> np.ndarray:
    """the FIRST element of largest magnitude, signed (`if (amax < fabsf(v))` / `if (ax > amax)`: a later equal magnitude does not replace it)"""
    idx = np.argmax(np.abs(xb), axis=-1)
    return np.take_along_axis(xb, idx[..., None], axis=-1)[..., 0]


def _recip(d: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore"):
        return np.where(d != 0, (f32(1.0) / d).astype(f32), f32(0.0)).astype(f32)


def best_index_int8(x: np.ndarray) -> np.ndarray:
    """ggml-quants.c:4562-4571 over kvalues_iq4nl: the nearer of the two neighbours, the upper one on a tie; the differences are f32."""
    val = KVALUES_IQ4NL.astype(f32)
    x = np.asarray(x, f32)
    ml = np.zeros(x.shape, np.int64)
    for i in range(1, 15):
        ml += ~(x < val[i])
    mu = ml + 1
    lo = (x - val[mu - 1]).astype(f32); hi = (val[mu] - x).astype(f32)
    r = np.where(lo < hi, mu - 1, mu)
    r = np.where(x >= val[15], 15, r)
    return np.where(x <= val[0], 0, r).astype(np.uint8)


def _pack_nibbles(xi: np.ndarray) -> np.ndarray:
    return ((xi[..., :16] & 15) | ((xi[..., 16:] & 15) << 4)).astype(np.uint8)


def _qh(xi: np.ndarray) -> np.ndarray:
    """the fifth bits: bit j of qh = bit 4 of element j (elements 0..15 low half, 16..31 high half) -> 4 bytes, little endian"""
    bits = ((xi.astype(np.uint32) >> 4) & 1) << np.arange(32, dtype=np.uint32)
    qh = bits.sum(axis=-1).astype("<u4")
    return np.ascontiguousarray(qh[..., None]).view(np.uint8)


def _f16_bytes(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(x, f32).astype("<f2")[..., None]).view(np.uint8)


def quantize_rows(kv: str, x: np.ndarray) -> np.ndarray:
    """f32 [..., n] -> the blocks the reference's from_float of `kv` stores, uint8 [..., n / 32 * BB]."""
    x = np.ascontiguousarray(x, f32)
    xb = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    if kv in ("q4_1", "q5_1"):                                                   # quantize_row_q4_1_ref :68-103, quantize_row_q5_1_ref :149-191
        levels = 15 if kv == "q4_1" else 31
        mn = xb.min(axis=-1); mx = xb.max(axis=-1)
        d = ((mx - mn).astype(f32) / f32(levels)).astype(f32)
        idv = _recip(d)
        t = (((xb - mn[..., None]).astype(f32) * idv[..., None]).astype(f32) + f32(0.5)).astype(f32)
        xi = t.astype(np.int32)                                                 # (int8_t) / (uint8_t) of a float in range: truncation
        if kv == "q4_1":
            xi = np.minimum(15, xi)
            parts = [_f16_bytes(d), _f16_bytes(mn), _pack_nibbles(xi)]
        else:
            xi = xi & 0xFF
            parts = [_f16_bytes(d), _f16_bytes(mn), _qh(xi), _pack_nibbles(xi)]
    elif kv == "q5_0":                                                          # quantize_row_q5_0_ref :105-147
        d = (_first_absmax(xb) / f32(-16.0)).astype(f32)
        idv = _recip(d)
        t = ((xb * idv[..., None]).astype(f32) + f32(16.5)).astype(f32)
        xi = np.minimum(31, t.astype(np.int32))
        parts = [_f16_bytes(d), _qh(xi), _pack_nibbles(xi)]
    elif kv == "iq4_nl":                                                        # quantize_row_iq4_nl_ref :4707 -> quantize_row_iq4_nl_impl, ntry = -1, no weights
        mxv = _first_absmax(xb)
        small = np.abs(mxv) < GROUP_MAX_EPS
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            d0 = (mxv / f32(-127.0)).astype(f32)                                # max / values[0]
            idv = (f32(1.0) / d0).astype(f32)
            L = best_index_int8((idv[..., None] * xb).astype(f32))
            qv = KVALUES_IQ4NL[L].astype(f32)
            w = (xb * xb).astype(f32)
            wq = (w * qv).astype(f32)
            tx = (wq * xb).astype(f32); t2 = (wq * qv).astype(f32)
            sumqx = np.zeros(xb.shape[:-1], f32); sumq2 = np.zeros(xb.shape[:-1], f32)
            for j in range(32):                                                 # sequential f32 sums, not contracted (see the module docstring)
                sumqx = (sumqx + tx[..., j]).astype(f32); sumq2 = (sumq2 + t2[..., j]).astype(f32)
            d = (sumqx / sumq2).astype(f32)
        d = np.where(small, f32(0.0), d).astype(f32)
        L = np.where(small[..., None], 0, L).astype(np.uint8)                   # memset(q4, 0) and no index written
        parts = [_f16_bytes(d), _pack_nibbles(L)]
    else:
        raise ValueError(kv)
    out = np.concatenate(parts, axis=-1)
    return np.ascontiguousarray(out.reshape(x.shape[:-1] + (-1,)))


# ---------------------------------------------------------------------------------------------------------------- reading blocks
def unpack(kv: str, blk: np.ndarray):
    """uint8 [..., nb * BB] -> (d f32 [..., nb], m f32 [..., nb] or None, q int32 [..., nb, 32]): q is the value the dot product multiplies
    (Q4_1 / Q5_1: unsigned 0..15 / 0..31; Q5_0: nibble | bit << 4, minus 16; IQ4_NL: kvalues_iq4nl[nibble])."""
    bb = block_bytes(kv)
    b = np.ascontiguousarray(blk).reshape(blk.shape[:-1] + (blk.shape[-1] // bb, bb))
    h = lambda o: np.ascontiguousarray(b[..., o:o + 2]).view("<f2")[..., 0].astype(f32)
    d = h(0)
    m = h(2) if kv in ("q4_1", "q5_1") else None
    qo = {"q4_1": 4, "q5_0": 6, "q5_1": 8, "iq4_nl": 2}[kv]
    qs = b[..., qo:qo + 16].astype(np.int32)
    q = np.concatenate([qs & 15, qs >> 4], axis=-1)
    if kv in ("q5_0", "q5_1"):
        qh = np.ascontiguousarray(b[..., qo - 4:qo]).view("<u4")[..., 0].astype(np.uint32)
        q = q | ((((qh[..., None] >> np.arange(32, dtype=np.uint32)) & 1) << 4).astype(np.int32))
        if kv == "q5_0":
            q = q - 16
    elif kv == "iq4_nl":
        q = KVALUES_IQ4NL[q].astype(np.int32)
    return d, m, q


def dequantize(kv: str, blk: np.ndarray) -> np.ndarray:
    """dequantize_row_q4_1 / _q5_0 / _q5_1 / _iq4_nl: q * d + m (product and sum each rounded), (q - 16) * d, d * kvalues[q]."""
    d, m, q = unpack(kv, blk)
    y = (q.astype(f32) * d[..., None]).astype(f32)
    if m is not None:
        y = (y + m[..., None]).astype(f32)
    return y.reshape(y.shape[:-2] + (-1,))


# ---------------------------------------------------------------------------------------------------------------- q and the scores
def quantize_q(x: np.ndarray, with_sum: bool):
    """the SIMD quantize_row_q8_0 / _q8_1: d = amax / 127, id = 127 / amax (0 for an all-zero block), q = round-half-even(x * id); the stored
    scale is f16(d); Q8_1 adds s = f16(d * sum(q)) with the UNROUNDED d.  x [n] -> (d f32 [nb] (f16 values), s f32 [nb] or None, q int32 [nb, 32])."""
    xb = np.asarray(x, f32).reshape(-1, 32)
    amax = np.abs(xb).max(axis=-1)
    d = (amax / f32(127.0)).astype(f32)
    with np.errstate(divide="ignore"):
        idv = np.where(amax != 0, (f32(127.0) / amax).astype(f32), f32(0.0)).astype(f32)
    q = np.rint((xb * idv[:, None]).astype(f32)).astype(np.int32)
    s = (d * q.sum(axis=-1).astype(f32)).astype(f32).astype(np.float16).astype(f32) if with_sum else None
    return d.astype(np.float16).astype(f32), s, q


def _fma(a, b, c):
    """f32 fma: the product of an f16-by-f16 scale (<= 22 significant bits) or an f32 and a small integer is exact in f64; one rounding remains
    double (f64 then f32), a 2^-29 coincidence"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _hsum8(acc: np.ndarray) -> np.ndarray:
    t = (acc[:, :4] + acc[:, 4:]).astype(f32)                                    # hsum_float_8
    return ((t[:, 0] + t[:, 2]).astype(f32) + (t[:, 1] + t[:, 3]).astype(f32)).astype(f32)


def vec_dot(kv: str, kd, km, kq, qd, qs, qq) -> np.ndarray:
    """rows (kd [R, nb], km, kq [R, nb, 32]) against one quantized vector (qd [nb], qs [nb], qq [nb, 32]) -> [R] f32, the AVX2 order."""
    R, nb = kd.shape
    lanes = lambda b: (kq[:, b] * qq[b]).reshape(R, 8, 4).sum(axis=-1).astype(f32)          # eight lanes of four int8 products each
    if kv in ("q4_1", "q5_1"):
        acc = np.zeros((R, 8), f32); summs = np.zeros(R, f32)
        for b in range(nb):
            summs = (summs + (km[:, b] * qs[b]).astype(f32)).astype(f32)         # summs += m_k * s_q (rounded product, rounded sum)
            acc = _fma((kd[:, b] * qd[b]).astype(f32)[:, None], lanes(b), acc)
        return (_hsum8(acc) + summs).astype(f32)
    if kv == "q5_0":
        acc = np.zeros((R, 8), f32)
        for b in range(nb):
            acc = _fma((kd[:, b] * qd[b]).astype(f32)[:, None], lanes(b), acc)
        return _hsum8(acc)
    a1 = np.zeros((R, 8), f32); a2 = np.zeros((R, 8), f32)                        # iq4_nl: pairs of blocks into two accumulators
    for b in range(0, nb - 1, 2):
        a1 = _fma((qd[b] * kd[:, b]).astype(f32)[:, None], lanes(b), a1)
        a2 = _fma((qd[b + 1] * kd[:, b + 1]).astype(f32)[:, None], lanes(b + 1), a2)
    sumf = _hsum8((a1 + a2).astype(f32))
    if nb & 1:                                                                  # the scalar tail: sumf += d * (sumi1 + sumi2)
        b = nb - 1
        dd = (qd[b] * kd[:, b]).astype(f32)
        sumf = (sumf + (dd * (kq[:, b] * qq[b]).sum(axis=-1).astype(f32)).astype(f32)).astype(f32)
    return sumf


# ---------------------------------------------------------------------------------------------------------------- FLASH_ATTN_EXT
def flash_attn_ext(kv: str, q: np.ndarray, k_blocks: np.ndarray, v_blocks: np.ndarray, mask, scale: float, max_bias: float = 0.0,
                   logit_softcap: float = 0.0) -> np.ndarray:
    """q [B, H, N, DK] f32; k_blocks / v_blocks uint8 [B, Hk, n_kv, D / 32 * BB]; mask [>= N, n_kv] f16 or None -> [B, N, H, DV] f32."""
    q = np.asarray(q, f32)
    B, H, N, DK = q.shape
    Hk, n_kv = k_blocks.shape[1], k_blocks.shape[2]
    kd, km, kq = unpack(kv, k_blocks)
    vdeq_all = dequantize(kv, v_blocks)
    DV = vdeq_all.shape[-1]
    n_head_log2 = 1 << int(np.floor(np.log2(H)))
    m0 = f32(2.0) ** f32(-(max_bias) / n_head_log2); m1 = f32(2.0) ** f32(-(max_bias / 2.0) / n_head_log2)
    sc = f32(scale)
    if logit_softcap != 0.0:
        sc = f32(sc / f32(logit_softcap))
    out = np.zeros((B, N, H, DV), f32)
    for b in range(B):
        for h in range(H):
            slope = f32(1.0)
            if max_bias > 0.0:
                slope = f32(m0 ** f32(h + 1)) if h < n_head_log2 else f32(m1 ** f32(2 * (h - n_head_log2) + 1))
            hk = h // (H // Hk)
            vdeq = vdeq_all[b, hk].astype(f64)
            for n in range(N):
                qd, qs, qq = quantize_q(q[b, h, n], kv in ("q4_1", "q5_1"))
                dots = vec_dot(kv, kd[b, hk], km[b, hk] if km is not None else None, kq[b, hk], qd, qs, qq)
                S = f32(0.0); M = f32(-np.inf)
                acc = np.zeros(DV, f32)
                for j in range(n_kv):
                    mv = f32(slope * f32(mask[n, j])) if mask is not None else f32(0.0)
                    if mv == -np.inf:
                        continue
                    s = f32(dots[j] * sc)
                    if logit_softcap != 0.0:
                        s = f32(f32(logit_softcap) * f32(_libm.tanhf(float(s))))
                    s = f32(s + mv)
                    ms = f32(1.0); vs = f32(1.0)
                    if s > M:
                        Mold = M; M = s
                        ms = f32(_libm.expf(float(f32(Mold - M))))
                        acc = (acc * ms).astype(f32)                                              # ggml_vec_scale_f32
                    else:
                        vs = f32(_libm.expf(float(f32(s - M))))
                    acc = (vdeq[j] * f64(vs) + acc.astype(f64)).astype(f32)                       # ggml_vec_mad_f32 (fma)
                    S = f32(f32(S * ms) + vs)
                out[b, n, h] = acc * f32(f32(1.0) / S)
    return out
