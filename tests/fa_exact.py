"""tests/fa_exact.py -- "selector" data for FLASH_ATTN_EXT: inputs on which every path must return the same bits (TEST INFRASTRUCTURE ONLY, plain numpy).

Every probability is exactly 0 or exactly 1 / n:
  * q, K and V are integers (times a power of two), `scale` is a power of two and the finite mask values are integers, so every score
    scale * q.k + slope * mask is an exact f32 in any summation order -- also after q is rounded to f16 / bf16 or quantized to Q8_0 / Q8_1
    (every 32-block of a q row holds +-127 only: d = 1 and the integers survive);
  * per query row a tie set A of n in {1, 2, 4, .., 64} live positions shares the maximum score and every other live position scores at least
    GAP = 128 below it.  expf underflows to +0 below about -103.98 (the smallest f32 subnormal is 1.4e-45, exp(-128) = 2.6e-56), so every expf of
    the project returns exactly 1 on A and exactly +0 elsewhere, and every rescale factor is exactly 0 or 1;
  * n * max|v| <= 2048 on A, so even an f16 accumulator sums A exactly, and the output is (sum_{j in A} v_j) / n bit for bit;
  * every V row outside all tie sets holds large "poison" values of both signs: a leaked probability, a wrong row, a missed rescale or a stale
    LDS row changes bits.

How a row selects its tie set: position j of kv head hk carries a code word (a row of the Sylvester-Hadamard matrix or its negation, +-1 per head
element) times an amplitude, the query row carries 127 times the code word of its target, so a matching position scores scale * 127 * amp * DK and
every other one at most half of that; a "decoy" is a matching position whose finite mask value puts it exactly GAP below.  exact_expectation() takes
none of this on trust: it recomputes the scores in float64 from the values as the kernel sees them and asserts every condition above on the case's own data.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import kvq_ref

f32 = np.float32
f64 = np.float64
GAP = 128.0                                      # against expf's underflow threshold of about -103.98
TILE = 64                                        # positions per tile and query rows per workgroup of k_flash_attn_mfma
BLOCK_TYPES = ["q8_0", "q4_0", "q4_1", "q5_0", "q5_1", "iq4_nl"]
BLOCK_BYTES = {"q8_0": 34, "q4_0": 18, "q4_1": 20, "q5_0": 22, "q5_1": 24, "iq4_nl": 18}
KVALUES = kvq_ref.KVALUES_IQ4NL.astype(np.int64)
BIG = 2.0 ** 18                                  # the bf16 forms beyond f16's range: K and V are 2^18 times small integers
Q_AMP = 127                                      # every non-zero q element is +-127: a Q8_0 / Q8_1 block of them has d = 1

# the K levels of a +1 / -1 code element (a, b): K = a or -b times the amplitude; asymmetric where the type's range is
K_LEVELS = {"f16": (1, 1), "bf16": (1, 1), "q8_0": (127, 127), "q4_0": (7, 8), "q4_1": (7, 8), "q5_0": (15, 16), "q5_1": (15, 16), "iq4_nl": (113, 127)}


# ---------------------------------------------------------------------------------------------------------------- number formats
def bf16_bits(x: np.ndarray) -> np.ndarray:
    """f32 values that bf16 holds exactly -> uint16 bits (asserted)"""
    u = np.ascontiguousarray(x, f32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not a bf16 value"
    return (u >> 16).astype(np.uint16)


def bf16_values(bits: np.ndarray) -> np.ndarray:
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(f32).astype(f64)


def bf16_round(x: np.ndarray) -> np.ndarray:
    """round to nearest even on the bits (ggml_compute_fp32_to_bf16) -> f32"""
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(f32)


def pack_rows(kv: str, x: np.ndarray, d: np.ndarray) -> np.ndarray:
    """rows of a block cache from chosen integers: x int [..., D] in the type's own range (q8_0 -127..127, the 4-bit types -8..7, the 5-bit types
    -16..15, iq4_nl a value of its table), d [...] a power of two (or 0) per ROW -> uint8 [..., D / 32 * BB]; value = d * x.  q4_1 / q5_1 store
    x + 8 / x + 16 with m = -8 d / -16 d.  tests/kvq_ref.py's packing."""
    x = np.asarray(x, np.int64)
    xb = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    db = np.broadcast_to(np.asarray(d, f32)[..., None], xb.shape[:-1])
    dbytes = kvq_ref._f16_bytes(db)
    if kv == "q8_0":
        assert np.abs(xb).max() <= 127
        parts = [dbytes, xb.astype(np.int8).view(np.uint8)]
    elif kv in ("q4_0", "q4_1"):
        assert xb.min() >= -8 and xb.max() <= 7
        parts = [dbytes] + ([kvq_ref._f16_bytes(db * f32(-8.0))] if kv == "q4_1" else []) + [kvq_ref._pack_nibbles(xb + 8)]
    elif kv in ("q5_0", "q5_1"):
        assert xb.min() >= -16 and xb.max() <= 15
        parts = [dbytes] + ([kvq_ref._f16_bytes(db * f32(-16.0))] if kv == "q5_1" else []) + [kvq_ref._qh(xb + 16), kvq_ref._pack_nibbles(xb + 16)]
    elif kv == "iq4_nl":
        idx = np.searchsorted(KVALUES, xb)
        assert (KVALUES[np.minimum(idx, 15)] == xb).all(), "not a value of kvalues_iq4nl"
        parts = [dbytes, kvq_ref._pack_nibbles(idx)]
    else:
        raise ValueError(kv)
    out = np.concatenate(parts, axis=-1)
    return np.ascontiguousarray(out.reshape(x.shape[:-1] + (-1,)))


def dequantize(kv: str, blk: np.ndarray) -> np.ndarray:
    """uint8 [..., nb * BB] -> float64 [..., 32 nb]: dequantize_row_<type>"""
    if kv in kvq_ref.TYPES:
        return kvq_ref.dequantize(kv, blk).astype(f64)
    bb = BLOCK_BYTES[kv]
    b = np.ascontiguousarray(blk).reshape(blk.shape[:-1] + (blk.shape[-1] // bb, bb))
    d = np.ascontiguousarray(b[..., 0:2]).view("<f2")[..., 0].astype(f32)
    if kv == "q8_0":
        q = np.ascontiguousarray(b[..., 2:34]).view(np.int8).astype(f32)
    else:
        qs = b[..., 2:18].astype(np.int32)
        q = (np.concatenate([qs & 15, qs >> 4], axis=-1) - 8).astype(f32)
    return (q * d[..., None]).astype(f32).reshape(blk.shape[:-1] + (-1,)).astype(f64)


def cache_values(cache: str, a: np.ndarray) -> np.ndarray:
    """the cache as the kernels read it, float64"""
    if cache == "f16":
        return np.asarray(a, np.float16).astype(f64)
    if cache == "bf16":
        return bf16_values(a)
    return dequantize(cache, a)


def q_as_seen(cache: str, q: np.ndarray) -> np.ndarray:
    """q as the kernels of this cache type take it: rounded to f16 (an f16 cache, and the fused kernel on a block cache), to bf16, or quantized to
    Q8_0 / Q8_1 (the row kernel of a block cache) -- the design makes all of them the identity, which is asserted"""
    q = np.asarray(q, f32)
    if cache == "bf16":
        seen = bf16_round(q)
    else:
        seen = q.astype(np.float16).astype(f32)
        if cache in BLOCK_TYPES:
            flat = q.reshape(-1, q.shape[-1])
            deq = np.stack([(lambda d, s, qq: (qq.astype(f32) * d[:, None]).reshape(-1))(*kvq_ref.quantize_q(r, False)) for r in flat]).reshape(q.shape)
            assert np.array_equal(deq, seen), "q does not survive the Q8_0 quantizer"
    assert np.array_equal(seen, q), "q does not survive its rounding"
    return seen.astype(f64)


# ---------------------------------------------------------------------------------------------------------------- the expectation
def alibi_slopes(H: int, max_bias: float) -> list:
    n2 = 1
    while 2 * n2 <= H:
        n2 *= 2
    m0, m1 = 2.0 ** (-max_bias / n2), 2.0 ** (-(max_bias / 2.0) / n2)
    return [(m0 ** (h + 1) if h < n2 else m1 ** (2 * (h - n2) + 1)) if max_bias > 0 else 1.0 for h in range(H)]


def _pow2(x: float) -> bool:
    return x > 0 and np.frexp(x)[0] == 0.5


def tie_sets(q, k, mask, scale, max_bias=0.0, softcap=0.0, allow_dead_rows=False):
    """float64 scores from the values as the kernel sees them (q [B, H, N, DK], k [Bk, Hk, n_kv, DK]); asserts that the finite scores are exact f32
    (before the soft-cap), that per row the maximum is shared by n = 2^i <= 64 positions and every other live position lies GAP or more below (after
    soft-cap and mask) -> {(b, h, t): positions of the tie set}"""
    q = np.asarray(q, f64); k = np.asarray(k, f64)
    B, H, N, _ = q.shape
    Bk, Hk, n_kv, _ = k.shape
    assert _pow2(scale), "scale must be a power of two"
    slopes = alibi_slopes(H, max_bias)
    assert all(_pow2(s) for s in slopes), "ALiBi slopes must be powers of two"
    assert (q == np.rint(q)).all() and (k == np.rint(k)).all(), "q and K must be integers"
    k_gcd = int(np.gcd.reduce(np.abs(k).astype(np.int64).ravel()))
    k_unit = float(k_gcd & -k_gcd) if k_gcd else 1.0                        # the power of two every K value is a multiple of
    mm = None
    if mask is not None:
        mm = np.asarray(mask)[:N, :n_kv].astype(f64)
        fin = np.isfinite(mm)
        assert (mm[fin] == np.rint(mm[fin])).all() and not (mm == np.inf).any() and not np.isnan(mm).any(), "finite mask values must be integers"
    sets = {}
    for b in range(B):
        for h in range(H):
            dots = q[b, h] @ k[b // (B // Bk), h // (H // Hk)].T
            assert ((np.abs(q[b, h]) @ np.abs(k[b // (B // Bk), h // (H // Hk)]).T) < 2.0 ** 24 * k_unit).all(), "a partial sum may round"
            s = dots * scale
            assert (s.astype(f32).astype(f64) == s).all(), "a score is not an exact f32"
            if softcap:
                s = softcap * np.tanh(s / softcap)
            if mm is not None:
                with np.errstate(invalid="ignore"):
                    s = np.where(fin, s + slopes[h] * np.where(fin, mm, 0.0), -np.inf)
                if not softcap:
                    assert (s[fin].astype(f32).astype(f64) == s[fin]).all(), "a masked score is not an exact f32"
            for t in range(N):
                row = s[t]
                M = row.max()
                if M == -np.inf:
                    assert allow_dead_rows, f"row {(b, h, t)} is fully masked"
                    sets[b, h, t] = np.zeros(0, np.int64)
                    continue
                A = np.flatnonzero(row == M)
                rest = row[row < M]
                assert rest.size == 0 or rest.max() <= M - GAP, f"row {(b, h, t)}: the runner-up lies {M - rest.max()} below the maximum, not {GAP}"
                assert A.size <= 64 and A.size & (A.size - 1) == 0, f"row {(b, h, t)}: a tie set of {A.size}"
                sets[b, h, t] = A
    return sets


def exact_expectation(q, k, v, mask, scale, max_bias=0.0, softcap=0.0, v_unit=1.0, allow_dead_rows=False) -> np.ndarray:
    """q [B, H, N, DK], k [Bk, Hk, n_kv, DK], v [Bk, Hk, n_kv, DV] in float64 AS THE KERNEL SEES THEM (q rounded, the cache dequantized); asserts the
    determinacy conditions of the module docstring on this data (tie_sets, and n * max|v| <= 2048 v_unit with v whole multiples of v_unit on every tie
    set) -> mean(V[A]) as f32 [B, N, H, DV]; a fully masked row (only with allow_dead_rows) gives zeros."""
    v = np.asarray(v, f64)
    B, H, N, _ = np.shape(q)
    Bk, Hk = v.shape[0], v.shape[1]
    sets = tie_sets(q, k, mask, scale, max_bias, softcap, allow_dead_rows)
    out = np.zeros((B, N, H, v.shape[3]), f32)
    for (b, h, t), A in sets.items():
        if A.size == 0:
            continue
        va = v[b // (B // Bk), h // (H // Hk)][A]
        assert (va / v_unit == np.rint(va / v_unit)).all() and A.size * np.abs(va).max() <= 2048 * v_unit, f"row {(b, h, t)}: n * max|v| beyond 2048"
        mean = va.sum(axis=0) / A.size
        out[b, t, h] = mean.astype(f32)
        assert (out[b, t, h].astype(f64) == mean).all()
    return out


# ---------------------------------------------------------------------------------------------------------------- masks
def piece_bounds(n_kv: int, n_split: int):
    """the pieces of the split row kernel: chunks of ceil(n_kv / n_split), the last one short"""
    chunk = (n_kv + n_split - 1) // n_split
    return [(i * chunk, min(n_kv, (i + 1) * chunk)) for i in range(n_split)]


def dead_mask(patterns, N: int, n_kv: int, n_split: int = 1) -> np.ndarray:
    """bool [N, n_kv]: the -inf positions of the named patterns together.  "none"; "causal" (the batch is the last N positions of the window);
    ("swa", W): the row at position p sees (p - W, p]; ("dead_tile", i): tile i for all rows; ("piece_dead", i): piece i of n_split"""
    dead = np.zeros((N, n_kv), bool)
    for p in patterns:
        kind = p if isinstance(p, str) else p[0]
        if kind == "none":
            continue
        for t in range(N):
            pos = n_kv - N + t
            if kind == "causal":
                dead[t, pos + 1:] = True
            elif kind == "swa":
                dead[t, pos + 1:] = True
                dead[t, :max(0, pos - p[1] + 1)] = True
            elif kind == "dead_tile":
                dead[t, TILE * p[1]:TILE * (p[1] + 1)] = True
            elif kind == "piece_dead":
                lo, hi = piece_bounds(n_kv, n_split)[p[1]]
                dead[t, lo:hi] = True
            else:
                raise ValueError(p)
    return dead


# ---------------------------------------------------------------------------------------------------------------- code words
def hadamard(n: int) -> np.ndarray:
    h = np.ones((1, 1), np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def code_words(Dc: int, DK: int, bias: int) -> np.ndarray:
    """[2 Dc, DK]: code c < Dc is row c of the Hadamard matrix, c >= Dc its negation; head elements past Dc repeat the word from its start (DK - Dc
    <= Dc), unless `bias` (the soft-cap form, DK = 2 Dc): then they are left to the caller"""
    h = hadamard(Dc)
    w = np.concatenate([h, -h])
    if bias:
        return np.concatenate([w, np.zeros((2 * Dc, DK - Dc), np.int64)], axis=1)
    return np.concatenate([w, w[:, :DK - Dc]], axis=1)


# ---------------------------------------------------------------------------------------------------------------- the case builder
def selector_case(name: str, *, N: int, n_kv: int, DK: int = 64, DV: int = 64, H: int = 4, Hk: int = 2, B: int = 1, Bk: int = 1, cache: str = "f16",
                  pattern="none", placement: str = "window", n_tie: int = 1, softcap: float = 0.0, max_bias: float = 0.0, big: bool = False,
                  seed: int = 0, n_split: int = 1, piece: int = 0, zones=None) -> SimpleNamespace:
    """Inputs and the expected output of one selector case.  cache: "f16", "bf16" (k / v are uint16 bits) or a block type (uint8 rows).
    pattern: a mask pattern of dead_mask() or a list of them.  placement -- where each row's maximum sits:
      "window"            (a sliding window of W <= number of codes) row t at position p selects p - (7 t + 13 h + 5 b + seed) % W
      "late_after_decoy"  code c: a decoy in tile 0 whose mask value puts it exactly GAP below, the maximum at position n_kv - N + c (the last, partial
                          tile; under a causal mask the diagonal, so the last row selects n_kv - 1)
      "walk"              every position its own code: row t selects the (37 t + ..)-th position it sees, so every one of the 64 positions of a tile is
                          selected by some row; with fewer codes than positions (DK = 32) the codes repeat per tile and kv head hk's tile hk % 2
                          carries twice the amplitude: rows of that head select there, past (or before) a half-score match in the other tile
      "ties_across"       tie sets of n_tie in {2, 4} split evenly over the two `zones` ((start, length) each; default tiles 0 and 1); n_tie = 64: one
                          set of 32 + 32 positions around the zone boundary (even kv heads) or every second position of both zones (odd kv heads)
      "mixed"             per row one of: first position, last position, late maximum after a decoy, a tie of 2, a tie of 4 (both ends of the window)
      "piece_max"         (split rows) head h's maximum in piece `piece` of n_split, decoys GAP below in every other piece
    softcap: DK = 2 Dc; the second half of the head is a common negative bias so that scores outside the tie set are negative and the gap survives
    the cap.  big: the cache values are 2^18 times the integers (bf16 only) and `scale` is reduced to match."""
    patterns = pattern if isinstance(pattern, list) else [pattern]
    dead = dead_mask(patterns, N, n_kv, n_split)
    live = ~dead
    assert cache in K_LEVELS and (not big or cache == "bf16")
    Dc = 1 << (int(DK).bit_length() - 1)
    if softcap:
        assert DK % 2 == 0 and Dc == DK
        Dc = DK // 2
    C = 2 * Dc
    words = code_words(Dc, DK, bias=bool(softcap))
    code = -np.ones((Hk, n_kv), np.int64); amp = np.ones((Hk, n_kv), np.int64)
    target = np.zeros((B, H, N), np.int64)
    decoys = []
    rows = [(b, h, t) for b in range(B) for h in range(H) for t in range(N)]
    if placement == "window":
        W = [p[1] for p in patterns if not isinstance(p, str) and p[0] == "swa"][0]
        assert W <= C and n_kv - N - W + 1 >= 0
        code[:] = np.arange(n_kv) % C
        for b, h, t in rows:
            target[b, h, t] = code[0, n_kv - N + t - (7 * t + 13 * h + 5 * b + seed) % W]
    elif placement == "late_after_decoy":
        assert N <= 16 and n_kv >= TILE + N
        causal = bool(dead[0, n_kv - 1])
        for c in range(N):
            code[:, n_kv - N + c] = c; code[:, (7 * c + 5) % TILE] = c
            decoys.append((7 * c + 5) % TILE)
        for b, h, t in rows:
            target[b, h, t] = (t if h % 2 == 0 else t // 2) if causal else (t + 3 * h + 7 * b + seed) % N
    elif placement == "walk":
        vis_any = np.flatnonzero(live.any(axis=0))
        if vis_any.size <= C:
            code[:] = np.arange(n_kv) % C                  # (a position no row sees repeats a code: a tie, and poison, should its mask be ignored)
            code[:, vis_any] = np.arange(vis_any.size)
            for b, h, t in rows:
                vis = np.flatnonzero(live[t])
                target[b, h, t] = code[0, vis[(37 * t + 23 * h + TILE * b + 5 + seed) % vis.size]]
        else:
            assert not dead.any() and n_kv % C == 0
            code[:] = np.arange(n_kv) % C
            for hk in range(Hk):
                amp[hk, (np.arange(n_kv) // C) == hk % (n_kv // C)] = 2
            for b, h, t in rows:
                target[b, h, t] = (37 * t + 23 * h + 5 + seed) % C
    elif placement == "ties_across":
        (s0, l0), (s1, l1) = zones or ((0, TILE), (TILE, TILE))
        if n_tie == 64:
            assert s0 + l0 == s1 and l0 >= 64 and l1 >= 64
            for hk in range(Hk):
                if hk % 2 == 0:
                    code[hk, s1 - 32:s1 + 32] = 0
                else:
                    code[hk, s1 - 63:s1 + 64:2] = 0
        else:
            assert n_tie in (2, 4)
            G = min(16, l0 // 4, l1 // 4)
            assert G % 5 != 0
            for c in range(G):
                for u in range(n_tie // 2):
                    code[:, s0 + 4 * c + u] = c; code[:, s1 + 4 * ((5 * c + 3) % G) + u] = c
            for b, h, t in rows:
                target[b, h, t] = (t + 5 * h + 3 * b + seed) % G
    elif placement == "mixed":
        assert not dead.any() and n_kv >= 64
        code[:, 0] = 0
        code[:, n_kv - 1] = 1
        code[:, 3] = 2; code[:, n_kv - 2] = 2; decoys.append(3)
        code[:, 10] = 3; code[:, n_kv - 10] = 3
        for j in (20, 21, n_kv - 20, n_kv - 21):
            code[:, j] = 4
        for b, h, t in rows:
            target[b, h, t] = (h * N + t + b + seed) % 5
    elif placement == "piece_max":
        pieces = piece_bounds(n_kv, n_split)
        for c in range(H):
            for i, (lo, hi) in enumerate(pieces):
                if i == piece:
                    code[:, lo + (13 * c + 7 + seed) % (hi - lo)] = c
                else:
                    code[:, lo + (5 * c + 2) % (hi - lo)] = c; decoys.append(lo + (5 * c + 2) % (hi - lo))
        for b, h, t in rows:
            target[b, h, t] = h
    else:
        raise ValueError(placement)
    assert code.max() < C and target.max() < C

    # ---- the mask: -inf where the pattern says, the decoys' finite value, zero elsewhere; none at all where nothing asks for one
    mask = None
    if dead.any() or decoys or max_bias > 0:
        mask = np.zeros((N, n_kv), np.float16)
        if decoys:
            mask[:, decoys] = -GAP / min(alibi_slopes(H, max_bias))        # (exactly GAP below for the head of the smallest slope, more for the others)
        mask[dead] = -np.inf

    # ---- q and K
    unit = BIG if big else 1.0
    scale = 2.0 ** -4 / unit
    a, bneg = K_LEVELS[cache]
    q = np.zeros((B, H, N, DK), f32)
    for b, h, t in rows:
        q[b, h, t] = Q_AMP * words[target[b, h, t]]
    sk = np.where(code[..., None] >= 0, words[np.maximum(code, 0)], 0)                    # [Hk, n_kv, DK] in {-1, 0, 1}
    if softcap:
        q[..., Dc:] = Q_AMP
        sk[..., Dc:Dc + DK // 8] = -1                                                     # every position, background rows included
    xk = np.where(sk > 0, a, np.where(sk < 0, -bneg, 0))
    if cache in BLOCK_TYPES:
        dk = np.where(code >= 0, amp, 0).astype(f32)                                      # a background row: d = 0 (iq4_nl has no zero level)
        xk = np.where(xk == 0, a, xk)
        k = pack_rows(cache, xk, dk)[None]
    else:
        kval = (xk * amp[..., None] * unit).astype(f32)[None]
        k = kval.astype(np.float16) if cache == "f16" else bf16_bits(kval)
    k = np.ascontiguousarray(np.broadcast_to(k, (Bk,) + k.shape[1:]))
    q_seen, k_seen = q_as_seen(cache, q), cache_values(cache, k)
    sets = tie_sets(q_seen, k_seen, mask, scale, max_bias, softcap)
    n_max = max(A.size for A in sets.values())

    # ---- V: small integers on every row that some tie set holds, poison elsewhere
    small = np.zeros((Hk, n_kv), bool)
    for (b, h, t), A in sets.items():
        small[h // (H // Hk), A] = True
    lim = min(31, 2048 // n_max)
    if cache in ("f16", "bf16", "q8_0"):
        pal_s = np.arange(-lim, lim + 1)
    elif cache == "iq4_nl":
        pal_s = KVALUES[np.abs(KVALUES) * n_max <= 2048]
    else:
        top = 8 if cache in ("q4_0", "q4_1") else 16
        pal_s = np.arange(-top, top)
    if cache == "f16":                                  # the CPU's f16 accumulator must stay finite while it still holds poison: n_kv * max|v| < 65504
        P = min(1024, 60000 // n_kv)
        pal_p, d_p = np.concatenate([np.arange(-P, -P // 2), np.arange(P // 2 + 1, P + 1)]), 1.0
    elif cache == "bf16":
        pal_p, d_p = np.concatenate([np.arange(-255, -127), np.arange(128, 256)]), 1.0
    elif cache == "q8_0":
        pal_p, d_p = np.concatenate([np.arange(-127, -63), np.arange(64, 128)]), 16.0
    elif cache == "iq4_nl":
        pal_p, d_p = KVALUES[np.abs(KVALUES) >= 49], 16.0
    else:
        top = 8 if cache in ("q4_0", "q4_1") else 16
        pal_p, d_p = np.concatenate([np.arange(-top, -top // 2), np.arange(top // 2, top)]), (128.0 if top == 8 else 64.0)
    hk_i, j_i, c_i = np.meshgrid(np.arange(Hk), np.arange(n_kv), np.arange(DV), indexing="ij")
    mix = lambda m: ((j_i * 2654435761 + c_i * 40503 + hk_i * 9973 + seed * 131 + m) >> 5)          # a fixed scramble of (position, column, head)
    xs = pal_s[mix(0) % pal_s.size]
    xp = pal_p[mix(77) % pal_p.size]
    xv = np.where(small[..., None], xs, xp)
    if cache in BLOCK_TYPES:
        v = pack_rows(cache, xv, np.where(small, 1.0, d_p))[None]
    else:
        vval = (xv * unit).astype(f32)[None]
        v = vval.astype(np.float16) if cache == "f16" else bf16_bits(vval)
    v = np.ascontiguousarray(np.broadcast_to(v, (Bk,) + v.shape[1:]))
    v_seen = cache_values(cache, v)
    expect = exact_expectation(q_seen, k_seen, v_seen, mask, scale, max_bias, softcap, v_unit=unit)
    assert expect.any()
    return SimpleNamespace(name=name, cache=cache, q=q, k=k, v=v, mask=mask, scale=float(scale), max_bias=float(max_bias), softcap=float(softcap),
                           expect=expect, sets=sets, dead=dead, N=N, n_kv=n_kv, DK=DK, DV=DV, H=H, Hk=Hk, B=B, Bk=Bk, n_max=n_max, unit=unit)


# ---------------------------------------------------------------------------------------------------------------- the cases of the device file
# id -> (what runs it, selector_case arguments).  run: path = the FA_PATH_* name the call must take; fused = MI355Q_FA_FUSED ("1", "0" or None: unset);
# split = a workspace is passed; kv_direct; layout = "contig", "heads" (K / V as head views of one [n_kv, Hk, row] buffer: f16 strided views, the
# llama layout of a block cache)
SWA = dict(N=80, n_kv=208, pattern=("swa", 40), placement="window")
DECOY = dict(N=16, n_kv=208, pattern="causal", placement="late_after_decoy")
DEAD_MIDDLE = dict(N=64, n_kv=256, pattern=[("dead_tile", 1), ("dead_tile", 2)], placement="walk")
WALK = dict(N=64, n_kv=128, placement="walk")


def _cases():
    c = {}
    fused = dict(path="fused", fused="1", split=True, kv_direct=False, layout="contig")
    # ---- fused f16
    c["fused-f16-swa"] = (fused, dict(SWA))
    c["fused-f16-late_after_decoy"] = (fused, dict(DECOY))
    c["fused-f16-dead_middle"] = (fused, dict(DEAD_MIDDLE))
    c["fused-f16-walk"] = (fused, dict(WALK))
    c["fused-f16-walk-dk192-dv80"] = (fused, dict(WALK, DK=192, DV=80))
    for n in (2, 4, 64):
        c[f"fused-f16-ties_across-{n}"] = (fused, dict(N=16, n_kv=128, placement="ties_across", n_tie=n))
    c["fused-f16-gqa"] = (fused, dict(N=16, n_kv=208, H=8, Hk=2, B=2, Bk=1, max_bias=8.0, placement="late_after_decoy"))
    c["fused-f16-softcap"] = (fused, dict(SWA, softcap=200.0))
    c["fused-f16-strided"] = (dict(fused, layout="heads"), dict(N=48, n_kv=256, DK=128, DV=128, pattern="causal", placement="walk"))
    # ---- fused on the cache's own rows: bf16 beyond f16's range, the six block types
    direct = dict(path="fused_kv", fused="1", split=True, kv_direct=True, layout="contig")
    c["fused-bf16-big-swa"] = (direct, dict(SWA, cache="bf16", big=True))
    c["fused-bf16-big-late_after_decoy"] = (direct, dict(DECOY, cache="bf16", big=True))
    c["fused-bf16-big-walk"] = (direct, dict(WALK, cache="bf16", big=True))
    for kv in BLOCK_TYPES:
        c[f"fused-{kv}-swa"] = (direct, dict(SWA, cache=kv))
        c[f"fused-{kv}-walk-d32"] = (direct, dict(WALK, cache=kv, DK=32, DV=32))
        c[f"fused-{kv}-walk-d32-llama"] = (dict(direct, layout="heads"), dict(WALK, cache=kv, DK=32, DV=32, H=3, Hk=3, seed=1))
    # ---- the three-step matrix-core path
    three = dict(path="mfma3", fused="0", split=True, kv_direct=False, layout="contig")
    for cache in ("f16", "bf16"):
        for nm, spec in (("swa", SWA), ("dead_middle", DEAD_MIDDLE), ("late_after_decoy", DECOY)):
            c[f"mfma3-{cache}-{nm}"] = (three, dict(spec, cache=cache))
    # ---- the row kernels on an f16 cache
    row = dict(fused=None, split=True, kv_direct=False, layout="contig")
    c["seq-f16-mixed"] = (dict(row, path="row_seq"), dict(N=3, n_kv=200, DK=128, DV=128, placement="mixed"))
    split3 = dict(N=1, n_kv=300, DK=80, DV=80, n_split=3)                 # (three pieces of 100; a head size of whole 32s would take the seq kernel at n_kv <= 1024)
    for i in range(3):
        c[f"split3-f16-max-piece{i}"] = (dict(row, path="row_split"), dict(split3, placement="piece_max", piece=i))
    for n in (2, 4):
        c[f"split3-f16-ties_across-{n}"] = (dict(row, path="row_split"), dict(split3, placement="ties_across", n_tie=n, zones=((0, 100), (200, 100))))
    c["split3-f16-piece_dead0"] = (dict(row, path="row_split"), dict(split3, pattern=("piece_dead", 0), placement="piece_max", piece=1))
    c["split3-f16-piece_dead2"] = (dict(row, path="row_split"), dict(split3, pattern=("piece_dead", 2), placement="piece_max", piece=0))
    c["split8-f16-kv1025-last-piece"] = (dict(row, path="row_split"), dict(N=1, n_kv=1025, DK=128, DV=128, n_split=8, placement="piece_max", piece=7))
    c["split8-f16-kv1025-mixed"] = (dict(row, path="row_split"), dict(N=1, n_kv=1025, DK=128, DV=128, placement="mixed", seed=1))
    c["f32-f16-mixed-d80"] = (dict(row, path="row_f32", split=False), dict(N=2, n_kv=300, DK=80, DV=80, placement="mixed"))
    # ---- the row kernel of a block or bf16 cache
    kvrow = dict(row, path="kv_row")
    for kv in BLOCK_TYPES + ["bf16"]:
        c[f"kvrow-{kv}-swa"] = (kvrow, dict(N=2, n_kv=200, cache=kv, pattern=("swa", 40), placement="window"))
        c[f"kvrow-{kv}-late_after_decoy"] = (kvrow, dict(N=2, n_kv=200, cache=kv, pattern="causal", placement="late_after_decoy"))
        c[f"kvrow-{kv}-ties_across"] = (kvrow, dict(N=2, n_kv=200, cache=kv, placement="ties_across", n_tie=2 if kv in ("q4_1", "q5_0", "bf16") else 4,
                                                    zones=((0, 64), (128, 64))))
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def case(cid: str) -> SimpleNamespace:
    """the case, built once per process and never changed by the tests that share it"""
    run, kw = CASES[cid]
    s = selector_case(cid, **kw)
    s.run = SimpleNamespace(**run)
    for a in (s.q, s.k, s.v, s.expect) + ((s.mask,) if s.mask is not None else ()):
        a.setflags(write=False)
    return s
