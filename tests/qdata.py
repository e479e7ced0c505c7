"""Seeded synthetic quantized data for the tests (works with or without oracle/_ref).

`random_blocks` makes VALID packed rows straight from random bytes: any byte pattern is a legal
block as long as its f16 scale fields are finite, so those fields are overwritten with small finite
halfs.  `quantized_weights` prefers the real reference quantizer (ggml_quantize_chunk through
oracle/_ref) when it is present, as tests/test-backend-ops.cpp:39-128 does."""
from __future__ import annotations

import numpy as np

import oracle

# (block bytes, [byte offsets of f16 scale fields inside a block])
_F16_FIELDS = {
    oracle.Q4_0: (18, [0]), oracle.Q4_1: (20, [0, 2]), oracle.Q5_0: (22, [0]), oracle.Q5_1: (24, [0, 2]),
    oracle.Q8_0: (34, [0]), oracle.Q2_K: (84, [80, 82]), oracle.Q3_K: (110, [108]), oracle.Q4_K: (144, [0, 2]),
    oracle.Q5_K: (176, [0, 2]), oracle.Q6_K: (210, [208]), oracle.IQ4_NL: (18, [0]), oracle.IQ4_XS: (136, [0]),
    oracle.IQ2_XXS: (66, [0]), oracle.IQ2_XS: (74, [0]), oracle.IQ2_S: (82, [0]), oracle.IQ3_XXS: (98, [0]),
    oracle.IQ3_S: (110, [0]), oracle.IQ1_S: (50, [0]),
    oracle.IQ1_M: (56, []),      # its f16 super-scale is scattered over the top nibbles of scales[4] (u16 at 48..55)
}
BLCK = {t: (32 if t in (oracle.Q4_0, oracle.Q4_1, oracle.Q5_0, oracle.Q5_1, oracle.Q8_0, oracle.IQ4_NL) else 256)
        for t in _F16_FIELDS}


def row_size(t: int, k: int) -> int:
    return k // BLCK[t] * _F16_FIELDS[t][0]


def random_blocks(t: int, nrows: int, k: int, rng: np.random.Generator, scale: float = 1.0) -> np.ndarray:
    bs, fields = _F16_FIELDS[t]
    nb = k // BLCK[t]
    w = rng.integers(0, 256, (nrows, nb, bs), dtype=np.uint8)
    for off in fields:
        d = (rng.uniform(1e-3, 5e-2, (nrows, nb)) * scale).astype(np.float16)
        if rng.random() < 0.5:
            d = -d if off == 0 and t in (oracle.Q6_K, oracle.Q3_K) else d   # signed super-scales occur in practice
        w[:, :, off:off + 2] = d.view(np.uint8).reshape(nrows, nb, 2)
    if t == oracle.IQ1_M:
        h = (rng.uniform(1e-3, 5e-2, (nrows, nb)) * scale).astype(np.float16).view(np.uint16)
        for i in range(4):       # nibble i of the half lives in bits 12..15 of scales[i]
            w[:, :, 49 + 2 * i] = (w[:, :, 49 + 2 * i] & 0x0f) | ((((h >> (4 * i)) & 0xf) << 4).astype(np.uint8))
    return w.reshape(nrows, nb * bs)


def quantized_weights(t: int, nrows: int, k: int, rng: np.random.Generator, scale: float = 1.0) -> np.ndarray:
    if oracle.ref_available("scalar") and nrows * k <= (1 << 24):
        ref = _ref()
        return ref.quantize(t, (rng.uniform(-1, 1, (nrows, k)) * scale).astype(np.float32))
    return random_blocks(t, nrows, k, rng, scale)       # (scale shrinks the block scales alike: chained products stay finite)


_REF = None


def _ref():
    global _REF
    if _REF is None:
        _REF = oracle.Reference("scalar")
    return _REF


# ------------------------------------------------------------------------------------------------
# exact data: inputs whose product is an exact f32 number, whatever the order of the additions
# ------------------------------------------------------------------------------------------------
# Every dequantized weight of exact_blocks is  EXACT_UNIT[t] * integer  with |integer| < 256 (so it is a bf16 number), every activation of
# exact_acts an integer of magnitude <= 127 (a bf16 number too).  A product is then UNIT * integer, and as long as  sum |w| |x| < 2^24 UNITs
# every partial sum of every summation order is an exact f32: a kernel's answer can be held to equality with the float64 product.
# The payload (quants, signs, grid indices) stays random over all its values; only the scale fields are restricted.  Limits, from the
# dequantization formulas (oracle/orc_core.c, oracle/orc_iq.c; layouts oracle/orc_formats.h), largest |integer| in brackets:
#   Q4_0 d (q-8), d in {1,2,4} D [32]       Q5_0 d (q-16), d in {1,2,4} D [64]     Q8_0 d q, d = D [128]
#   Q4_1 d q + m, d = D, m in -{4,8,16} D [16]                                       Q5_1 d q + m, m in -{8,16,32} D [32]
#   Q2_K d sc q - dmin m: 4-bit fields, any value [45]                                Q3_K d (sc-32)(q-4|q): any 6-bit sc [128]
#   Q4_K d sc q - dmin m: sc, m <= 15 [225]    Q5_K sc <= 8, m <= 15 [248]          Q6_K d sc (q-32): |sc| <= 7 [224]
#   IQ4_NL d kv, d in {+-1,+-2} D [254]        IQ4_XS d (ls-32) kv: ls-32 in {+-1,+-2} [254]
#   IQ3_S d (1+2s) g, g <= 15: s <= 7 [225]    IQ3_XXS d/4 (1+2s) g, g <= 62: s <= 1 [186]
#   IQ2_XXS / IQ2_XS / IQ2_S d/8 (1+2s) g, g <= 43: s <= 2 [215]
#   IQ1_S / IQ1_M d/8 (1+2s) (8g +- 1), |g| <= 1, 3-bit s: any value [135]
_EXACT_D = 2.0 ** -6             # D: the one power of two behind every f16 scale field
EXACT_UNIT = {t: _EXACT_D for t in _F16_FIELDS}
EXACT_UNIT.update({oracle.IQ3_XXS: _EXACT_D / 4, oracle.IQ2_XXS: _EXACT_D / 8, oracle.IQ2_XS: _EXACT_D / 8, oracle.IQ2_S: _EXACT_D / 8,
                   oracle.IQ1_S: _EXACT_D / 8, oracle.IQ1_M: _EXACT_D / 8})


def _f16_bytes(v: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(v.astype(np.float16)).view(np.uint8).reshape(v.shape + (2,))


def _pack_k4_scales(sc: np.ndarray, mn: np.ndarray) -> np.ndarray:
    """8 six-bit (scale, min) pairs -> the 12 scale bytes of a Q4_K / Q5_K block (the inverse of get_scale_min_k4)."""
    out = np.zeros(sc.shape[:-1] + (12,), np.uint8)
    out[..., 0:4] = (sc[..., 0:4] & 63) | ((sc[..., 4:8] >> 4) << 6)
    out[..., 4:8] = (mn[..., 0:4] & 63) | ((mn[..., 4:8] >> 4) << 6)
    out[..., 8:12] = (sc[..., 4:8] & 15) | ((mn[..., 4:8] & 15) << 4)
    return out


def exact_blocks(t: int, nrows: int, k: int, rng: np.random.Generator) -> np.ndarray:
    """Packed rows of type t with random payloads whose every dequantized weight is EXACT_UNIT[t] * integer, |integer| < 256."""
    bs, fields = _F16_FIELDS[t]
    nb = k // BLCK[t]
    w = rng.integers(0, 256, (nrows, nb, bs), dtype=np.uint8)
    D = _EXACT_D
    shp = (nrows, nb)
    u8 = lambda lo, hi, *tail: rng.integers(lo, hi, shp + tail).astype(np.uint8)
    d = np.full(shp, D)
    if t in (oracle.Q4_0, oracle.Q5_0):
        d = D * rng.choice([1.0, 2.0, 4.0], shp)
    elif t == oracle.IQ4_NL:
        d = D * rng.choice([-2.0, -1.0, 1.0, 2.0], shp)
    for off in fields:
        w[:, :, off:off + 2] = _f16_bytes(d)
    if t in (oracle.Q4_1, oracle.Q5_1):                       # m: a negative multiple of d, so both signs occur
        w[:, :, 2:4] = _f16_bytes(-D * rng.choice([4.0, 8.0, 16.0] if t == oracle.Q4_1 else [8.0, 16.0, 32.0], shp))
    elif t in (oracle.Q4_K, oracle.Q5_K):
        sc = rng.integers(0, 16 if t == oracle.Q4_K else 9, shp + (8,)).astype(np.uint8)
        w[:, :, 4:16] = _pack_k4_scales(sc, u8(0, 16, 8))
    elif t == oracle.Q6_K:
        w[:, :, 192:208] = rng.integers(-7, 8, shp + (16,)).astype(np.int8).view(np.uint8)
    elif t == oracle.IQ4_XS:
        ls = rng.choice(np.array([30, 31, 33, 34], np.uint16), shp + (8,))
        sh = np.zeros(shp, np.uint16)
        for ib in range(8):
            sh |= (ls[..., ib] >> 4) << (2 * ib)
        w[:, :, 2:4] = np.ascontiguousarray(sh).view(np.uint8).reshape(shp + (2,))
        w[:, :, 4:8] = ((ls[..., 0::2] & 15) | ((ls[..., 1::2] & 15) << 4)).astype(np.uint8)
    elif t == oracle.IQ3_S:                                   # scales[4] at 106: two 4-bit scales per byte
        w[:, :, 106:110] = u8(0, 8, 4) | (u8(0, 8, 4) << 4)
    elif t == oracle.IQ3_XXS:                                 # top nibble of each of the 8 scales_and_signs words (2 + 64 + 4 ib + 3)
        top = w[:, :, 69:98:4]
        w[:, :, 69:98:4] = (top & 0x0F) | (u8(0, 2, 8) << 4)
    elif t == oracle.IQ2_XXS:                                 # top nibble of the second word of each 8-byte group (2 + 8 ib + 7)
        top = w[:, :, 9:66:8]
        w[:, :, 9:66:8] = (top & 0x0F) | (u8(0, 3, 8) << 4)
    elif t in (oracle.IQ2_XS, oracle.IQ2_S):                  # scales[8] behind the payload: two 4-bit scales per byte
        off = 66 if t == oracle.IQ2_XS else 74
        w[:, :, off:off + 8] = u8(0, 3, 8) | (u8(0, 3, 8) << 4)
    elif t == oracle.IQ1_M:                                   # the f16 super-scale is scattered over the top nibbles of scales[4] (u16 at 48..55)
        h = int(np.float16(D).view(np.uint16))
        for i in range(4):
            w[:, :, 49 + 2 * i] = (w[:, :, 49 + 2 * i] & 0x0f) | (((h >> (4 * i)) & 0xf) << 4)
    return w.reshape(nrows, nb * bs)


def exact_acts(n: int, k: int, rng: np.random.Generator, kind: str = "bf16", amp: int = 16, factors=None) -> np.ndarray:
    """Integer activations in [-amp, amp] as f32 [n, k].  kind "q8_0" / "q8_k" adds the one element per 32- / 256-block that makes the CPU's
    activation quantizer the identity (amax = 127: d = 1, quants == x), placed as tests/test_gpu_parity.py places it.
    factors: exponents e to draw from, one per activation block (32 elements, 256 for "q8_k"): the block is multiplied by 2^e, its sentinel
    becomes +-127 * 2^e, so the CPU's quantizer gives d = 2^e exactly and the same integer quants -- a kernel that pairs a block with
    another block's d is then wrong, which d = 1 everywhere cannot show."""
    x = rng.integers(-amp, amp + 1, (n, k)).astype(np.float32)
    if kind == "q8_0":
        x.reshape(n, k // 32, 32)[:, :, 0] = 127.0
    elif kind == "q8_k":
        x.reshape(n, k // 256, 256)[:, :, 3] = -127.0
    else:
        assert kind == "bf16", kind
    if factors is not None:
        blk = 256 if kind == "q8_k" else 32
        e = rng.choice(np.asarray(factors, np.float32), (n, k // blk))
        x = (x.reshape(n, k // blk, blk) * np.exp2(e)[:, :, None]).reshape(n, k).astype(np.float32)
    return x


def exact_product(orc, t: int, w: np.ndarray, x: np.ndarray, K: int, dq: np.ndarray | None = None) -> np.ndarray:
    """The float64 product of the dequantized weights and the activations, as f32 [n, nrows]: the only reference of the exact tests.
    (dq: orc.dequantize(t, w, K) where the caller already has it.)"""
    dq = orc.dequantize(t, w, K) if dq is None else dq
    return (x.astype(np.float64) @ dq.astype(np.float64).T).astype(np.float32)


def exact_sum_bound(orc, t: int, w: np.ndarray, x: np.ndarray, K: int, dq: np.ndarray | None = None) -> float:
    """An upper bound, in EXACT_UNITs, of sum |w| |x| over every (row, token) of the product and of the partial terms a kernel may form on the
    way: max over rows of sum_k (|w[k]| + 2 mins) * max over tokens |x[k]|, where `mins` (15 for Q4_K / Q5_K / Q2_K, else 0) covers the
    integer tiers, which add d sc sum(q x) and dmin m sum(x) separately.  Below 2^24 every partial sum is an exact f32."""
    wi = np.abs((orc.dequantize(t, w, K) if dq is None else dq).astype(np.float64)) / EXACT_UNIT[t]
    mins = 15.0 if t in (oracle.Q4_K, oracle.Q5_K, oracle.Q2_K) else 0.0
    return float(((wi + 2.0 * mins) @ np.abs(x).max(axis=0).astype(np.float64)).max())


# K values of tests/test_gpu_mmq_forms.py (tests/test_exact_data_cpu.py proves the 2^24 precondition for them without a GPU):
# the type's smallest planar K, then the K of the split-K forms (4 pieces, 8 pieces; uneven step counts where the type's planar K allow them)
_Q = oracle
EXACT_FORM_KS = {
    _Q.Q4_K: (256, 4096, 4352, 8192, 8448), _Q.Q5_K: (256, 4096, 4352, 8448), _Q.Q4_0: (256, 4096, 4352, 8448), _Q.IQ4_NL: (256, 4096, 4352, 8448),
    _Q.Q8_0: (256, 4096, 4352, 8448), _Q.IQ4_XS: (512, 4096, 8704), _Q.Q6_K: (2048, 4096, 8192), _Q.IQ3_S: (2048, 4096, 8192),
    _Q.IQ3_XXS: (2048, 4096, 8192),
}
EXACT_CANONICAL_K = {t: (384 if BLCK[t] == 32 else 512) for t in _F16_FIELDS}      # rows stay canonical at these K for every type that has a planar form


# ------------------------------------------------------------------------------------------------
# exact data of the per-column (GEMV) tiers: tests/test_gpu_gemv_forms.py
# ------------------------------------------------------------------------------------------------
# Those tiers restate the CPU's arithmetic: integer block sums against QUANTIZED activations, one f32 product per block.  With exact_acts'
# identity-quantized activations (d = 2^e per block, integer quants) every block term is a power of two times an integer, and the terms a
# kernel may form separately are bounded per element by (|w| + 2 EXACT_MINS) |x|:
#   Q4_K / Q5_K / Q2_K  d sc sum(q x) and dmin m sum(x), m <= 15        Q4_1 / Q5_1  d sum(q x) and m s, |m| <= 16 / 32 (s = d_x sum(x) as f16)
#   IQ1_S / IQ1_M       d (2s+1) sum(8 g x) / 8 and d (2s+1) delta sum(x) / 8, 2s+1 <= 15 (in EXACT_UNITs of d / 8)
# every other type folds its offset into the integer sum.
EXACT_MINS = {_Q.Q4_K: 15.0, _Q.Q5_K: 15.0, _Q.Q2_K: 15.0, _Q.Q4_1: 16.0, _Q.Q5_1: 32.0, _Q.IQ1_S: 15.0, _Q.IQ1_M: 15.0}


def exact_x_unit(x: np.ndarray) -> float:
    """The largest power of two (<= 1) that every activation is an integer multiple of."""
    u = 1.0
    while not np.array_equal(x / u, np.round(x / u)):
        u /= 2.0
        assert u >= 2.0 ** -16, "activations are not small dyadic numbers"
    return u


def exact_output_bound(orc, t: int, w: np.ndarray, x: np.ndarray, K: int, dq: np.ndarray | None = None) -> float:
    """max over (row, token) of sum_k (|w[row, k]| + 2 EXACT_MINS) |x[token, k]|, in units of EXACT_UNIT[t] * exact_x_unit(x).  Every partial
    sum of ONE output, in any order, is bounded by that output's own sum, so below 2^24 each is an exact f32 -- the per-output form of
    exact_sum_bound, which takes the maximum over tokens before it sums and is looser for it."""
    dq = orc.dequantize(t, w, K) if dq is None else dq
    xi = (np.abs(x).astype(np.float64) / exact_x_unit(x)).T
    mins = 2.0 * EXACT_MINS.get(t, 0.0)
    worst = 0.0
    for r0 in range(0, dq.shape[0], 2048):                    # (row chunks: the float64 copy of a large matrix is never held whole)
        wi = np.abs(dq[r0:r0 + 2048].astype(np.float64)) / EXACT_UNIT[t] + mins
        worst = max(worst, float((wi @ xi).max()))
    return worst


def exact_product_rows(orc, t: int, w: np.ndarray, x: np.ndarray, K: int, dq: np.ndarray | None = None) -> np.ndarray:
    """exact_product in row chunks (the same numbers; for matrices of ten thousand rows)."""
    dq = orc.dequantize(t, w, K) if dq is None else dq
    x64 = x.astype(np.float64)
    return np.concatenate([(x64 @ dq[r0:r0 + 2048].astype(np.float64).T).astype(np.float32) for r0 in range(0, dq.shape[0], 2048)], axis=1)


GEMV_PLANAR_TYPES = (_Q.Q4_K, _Q.Q5_K, _Q.Q6_K, _Q.IQ4_XS, _Q.IQ3_S, _Q.IQ3_XXS, _Q.Q8_0, _Q.Q4_0, _Q.IQ4_NL)
GEMV_ACT_KIND = {t: ("q8_0" if BLCK[t] == 32 else "q8_k") for t in _F16_FIELDS}      # block size of the activation format the CPU pairs with t


# canonical rows that N > 8 sends to the batched canonical tier unless MI355Q_FLAG_FORCE_GEMV is set (csrc/mmq_generic.hip)
GEMV_CANONICAL_BATCH_TYPES = (_Q.Q4_0, _Q.Q4_1, _Q.Q5_0, _Q.Q5_1, _Q.Q8_0, _Q.IQ4_NL, _Q.Q2_K, _Q.Q3_K, _Q.IQ2_XXS, _Q.IQ2_XS, _Q.IQ2_S, _Q.IQ3_XXS,
                              _Q.IQ3_S, _Q.IQ1_S, _Q.IQ1_M)


def gemv_small_k(t: int) -> int:
    """The type's smallest planar K: a row is a single partial step of the streaming kernel."""
    return {_Q.Q6_K: 2048, _Q.IQ3_S: 2048, _Q.IQ3_XXS: 2048, _Q.IQ4_XS: 512}.get(t, 256)


def gemv_ring_k(t: int, steps: int) -> int:
    """A planar K of `steps` steps per row (2048 elements a step, 1024 for Q8_0) whose last step is partial where the type has such a K."""
    if t in (_Q.Q6_K, _Q.IQ3_S, _Q.IQ3_XXS):
        return 2048 * steps
    if t == _Q.Q8_0:
        return 1024 * (steps - 1) + 256
    return 2048 * (steps - 1) + (512 if t == _Q.IQ4_XS else 256)


def gemv_canonical_ks(t: int) -> tuple:
    """(smallest K, a K of 65..127 sub-blocks of 32: a lane's second trip is ragged) at which rows of t are canonical."""
    if BLCK[t] == 32:
        return 384, 3104                                      # K % 256 != 0; 97 sub-blocks
    return (768 if t == _Q.IQ4_XS else 512), 2304             # IQ4_XS: 3 / 9 blocks (odd); Q6_K, IQ3_*: K % 2048 != 0; 72 sub-blocks


def gemv_amplitude(k: int, scaled: bool) -> tuple:
    """(amplitude, factor exponents) of the activations at K = k: chosen from the sizes of the formats' integers (largest |w| 254 units, a
    sentinel of 127 per activation block) so that sum (|w| + 2 mins) |x| of one output stays below 2^24 smallest units -- proven entry by
    entry in tests/test_exact_data_cpu.py, never read off a kernel's answer."""
    if k <= 1024:
        return 16, ((-2, -1, 0, 1, 2) if scaled else None)
    if k <= 4608:
        return 8, ((-1, 0, 1) if scaled else None)
    if k <= 8192:
        return 4, ((-1, 0) if scaled else None)
    return 2, ((0, 1) if scaled else None)


def _gemv_form_data():
    ks = {t: set() for t in _F16_FIELDS}
    for t in GEMV_PLANAR_TYPES:
        ks[t] |= {gemv_small_k(t), gemv_ring_k(t, 2), gemv_ring_k(t, 3), 2048}
    for t in (_Q.Q4_K, _Q.Q4_0):
        ks[t] |= {6144, 12288, 16640, 16384}                  # activation passes 1, 2, 3 of the prologue; column tiles 7 + 1
    ks[_Q.Q4_K] |= {28672}                                    # column tiles 4 + 3
    for t in _F16_FIELDS:
        if t not in (_Q.Q4_K, _Q.Q5_K):                       # (planar at every valid K)
            ks[t] |= set(gemv_canonical_ks(t))
    ks[_Q.Q5_0] |= {64}                                       # the row loop above 32768 rows
    ks[_Q.Q2_K] |= {2048}                                     # a canonical matrix next to planar ones
    return tuple((t, k) + gemv_amplitude(k, scaled) for t in sorted(ks) for k in sorted(ks[t]) for scaled in (False, True))


# (type, K, amplitude, factor exponents or None) of every data set tests/test_gpu_gemv_forms.py draws; tests/test_exact_data_cpu.py proves
# the 2^24 precondition and the exactness of the CPU arithmetic for each without a GPU
GEMV_FORM_DATA = _gemv_form_data()
