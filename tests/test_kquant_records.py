"""The planar Q4_K / Q5_K scale field as four 24-bit records, restated in numpy (no GPU).

ggml's get_scale_min_k4 (oracle/orc_core.c, k4_scale_min) reads the 6-bit scale and min of sub-block j out of three bytes of the canonical
12-byte field.  At load time the device rows store the same 96 bits as record g = sub-blocks (2g, 2g+1) at bytes 3g..3g+2:
    r_g = sc(2g) | sc(2g+1) << 6 | mn(2g) << 12 | mn(2g+1) << 18
and a consumer lane reads its record with one byte permute of a dword pair (k4_record, csrc/mi355q_common.h).  Checked here: for random
fields every sub-block decodes to the same (sc, mn) both ways, the lane's byte selection finds its record, and the packing is a bijection
(planar -> canonical gives the original bytes back, as get_tensor needs)."""
import numpy as np


def get_scale_min_k4(q: np.ndarray, j: int):
    """oracle/orc_core.c k4_scale_min over a batch of fields q [n, 12] (uint8)."""
    q = q.astype(np.int64)
    if j < 4:
        return q[:, j] & 63, q[:, j + 4] & 63
    return (q[:, j + 4] & 0x0F) | ((q[:, j - 4] >> 6) << 4), (q[:, j + 4] >> 4) | ((q[:, j] >> 6) << 4)


def to_records(q: np.ndarray) -> np.ndarray:
    """k4_field_to_records: canonical fields [n, 12] -> planar fields [n, 12]."""
    out = np.zeros_like(q)
    for g in range(4):
        sc0, mn0 = get_scale_min_k4(q, 2 * g)
        sc1, mn1 = get_scale_min_k4(q, 2 * g + 1)
        r = sc0 | sc1 << 6 | mn0 << 12 | mn1 << 18
        for b in range(3):
            out[:, 3 * g + b] = (r >> (8 * b)) & 0xFF
    return out


def from_records(p: np.ndarray) -> np.ndarray:
    """k4_records_to_field: planar fields -> canonical fields."""
    p = p.astype(np.int64)
    sc, mn = np.zeros((p.shape[0], 8), np.int64), np.zeros((p.shape[0], 8), np.int64)
    for g in range(4):
        r = p[:, 3 * g] | p[:, 3 * g + 1] << 8 | p[:, 3 * g + 2] << 16
        sc[:, 2 * g], sc[:, 2 * g + 1], mn[:, 2 * g], mn[:, 2 * g + 1] = r & 63, (r >> 6) & 63, (r >> 12) & 63, (r >> 18) & 63
    q = np.zeros(p.shape, np.int64)
    for j in range(4):
        q[:, j] = sc[:, j] | (sc[:, j + 4] >> 4) << 6
        q[:, j + 4] = mn[:, j] | (mn[:, j + 4] >> 4) << 6
        q[:, j + 8] = (sc[:, j + 4] & 0x0F) | (mn[:, j + 4] & 0x0F) << 4
    return q.astype(np.uint8)


def lane_record(p: np.ndarray, g: int) -> np.ndarray:
    """k4_record: v_perm_b32(hi, lo, sel) with (lo, hi) = (w0, w1) for g < 2, (w1, w2) otherwise; selector bytes o, o+1, o+2 and 0x0C (zero)."""
    w = p.astype(np.uint32).reshape(-1, 3, 4)
    words = w[:, :, 0] | w[:, :, 1] << 8 | w[:, :, 2] << 16 | w[:, :, 3] << 24             # w0, w1, w2
    lo, hi = (words[:, 0], words[:, 1]) if g < 2 else (words[:, 1], words[:, 2])
    pair = lo.astype(np.uint64) | hi.astype(np.uint64) << np.uint64(32)
    o = 3 * g if g < 2 else 3 * g - 4
    return (pair >> np.uint64(8 * o)) & np.uint64(0xFFFFFF)


def test_records_decode_like_get_scale_min_k4():
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, (20000, 12), dtype=np.uint8)
    q[:8] = [0x00] * 12, [0xFF] * 12, [0x3F] * 12, [0xC0] * 12, [0x0F] * 12, [0xF0] * 12, list(range(12)), list(range(255, 243, -1))
    p = to_records(q)
    for g in range(4):
        r = lane_record(p, g).astype(np.int64)
        assert np.all(r >> 24 == 0)
        for t in range(2):
            sc, mn = get_scale_min_k4(q, 2 * g + t)
            assert np.array_equal((r >> (6 * t)) & 63, sc), (g, t)
            assert np.array_equal((r >> (12 + 6 * t)) & 63, mn), (g, t)
    # the prefill tiers: mmq_bf16's k4_scale_min (record j >> 1, field j & 1) and mmq_i8's records h and h + 2 are the same records


def test_records_are_a_bijection():
    rng = np.random.default_rng(6)
    q = rng.integers(0, 256, (20000, 12), dtype=np.uint8)
    assert np.array_equal(from_records(to_records(q)), q)
    p = rng.integers(0, 256, (20000, 12), dtype=np.uint8)
    assert np.array_equal(to_records(from_records(p)), p)
    # all 96 bits move: a single set bit of the canonical field lands on a single bit of the planar one
    for bit in range(96):
        f = np.zeros((1, 12), np.uint8)
        f[0, bit // 8] = 1 << (bit % 8)
        assert int(np.unpackbits(to_records(f)).sum()) == 1, bit
