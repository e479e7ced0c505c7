"""mi355q_mul_mat_fw on the device: the streaming GEMV over f16 / bf16 weight matrices gives the reference CPU backend's bits (tests/fw_ref.py,
oracle.glue.vec_dot_f16_simd) for every chunk count, row count around the rows-per-wave and rows-per-workgroup boundaries of each launch form,
column count, pitch, and special value; it touches nothing beyond its rows; and what it refuses it leaves alone."""
import numpy as np
import pytest
import torch

import ggml_mi355 as G
from fw_ref import bf16_to_f32, f32_to_bf16, mul_mat_bf16, mul_mat_f16, same_bits

pytestmark = pytest.mark.gpu

# chunks of 32: one, two, an odd count, many (65: whole pairs of load groups and a remainder; two LDS tiles at 8 columns) -- and 5 and 9 chunks, where
# the kernel's odd whole group of 4 (above two columns) / of 8 (one or two columns) chunks is followed by a remainder
KS = (32, 64, 96, 2080, 160, 288)
MS = (1, 3, 15, 16, 17, 65, 1031)
NS = (1, 2, 3, 5, 8)
GUARD = 64
TYPES = ("f16", "bf16")
FORMS = (G.FW_ROWS_AUTO, G.FW_ROWS_4, G.FW_ROWS_8, G.FW_ROWS_16)

# the boundaries MS walks: rows per wave 4 / 8 / 16 (3 | 15, 16, 17 across), rows per workgroup 16 / 32 / 64 (15, 16, 17 | 65 across); a short matrix's AUTO form is 4 rows per wave
assert G.FW_WAVES == 4 and G.FW_ROWS_PER_WAVE == {G.FW_ROWS_4: 4, G.FW_ROWS_8: 8, G.FW_ROWS_16: 16}
for rpw in G.FW_ROWS_PER_WAVE.values():
    assert any(m < rpw for m in MS) and any(m > rpw for m in MS)
    assert any(m < G.FW_WAVES * rpw for m in MS) and any(m > G.FW_WAVES * rpw for m in MS)
assert {15, 16, 17} <= set(MS) and 65 in MS                                  # at and across 16 rows (a full wave; a workgroup of 4-row waves) and 64 (a full workgroup)

_ref_cache = {}


def _dt(t):
    return torch.float16 if t == "f16" else torch.bfloat16


def _w_host(t, M, K, seed):
    """weights as the 16-bit patterns [M, K] of type t"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((M, K)).astype(np.float32)
    return v.astype(np.float16).view(np.uint16) if t == "f16" else f32_to_bf16(v)


def _ref(t, w_bits, x):
    if t == "f16":
        return mul_mat_f16(w_bits.view(np.float16), x)
    return mul_mat_bf16(w_bits, x)


def _sweep_case(t, K):
    """(w bits [1031, K], x [8, K], reference [8, 1031]) -- computed once per (type, K); rows and columns are independent, the cases slice it"""
    if (t, K) not in _ref_cache:
        w = _w_host(t, max(MS), K, 1000 + K)
        x = np.random.default_rng(K).standard_normal((max(NS), K)).astype(np.float32)
        _ref_cache[(t, K)] = (w, x, _ref(t, w, x))
    return _ref_cache[(t, K)]


def _dev_w(t, bits, rows_alloc, pitch_elems, fill):
    """a [rows_alloc, pitch] device buffer of byte `fill` with `bits` in its first rows; returns (buffer, the [M, K] view)"""
    M, K = bits.shape
    buf = torch.full((rows_alloc, pitch_elems), 0, dtype=torch.int16, device="cuda").view(torch.uint8).fill_(fill).view(torch.int16)
    buf[:M, :K] = torch.from_numpy(bits.view(np.int16)).cuda()
    return buf, buf.view(_dt(t))[:M, :K]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("t", TYPES)
def test_sweep_bits_and_guards(t, form):
    for K in KS:
        w_all, x_all, ref_all = _sweep_case(t, K)
        xd = torch.from_numpy(x_all).cuda()
        for M in MS:
            outs = []
            for fill in (0xFF, 0x00):                                         # guard rows behind W and guard columns behind y: once 0xFF bytes, once zeros
                _, wv = _dev_w(t, w_all[:M], M + GUARD, K, fill)
                for N in NS:
                    ybuf = torch.full((N, M + GUARD), 0, dtype=torch.int32, device="cuda").view(torch.uint8).fill_(fill).view(torch.float32)
                    G.mul_mat_fw(wv, xd[:N], out=ybuf[:, :M], flags=form)
                    y = ybuf.cpu().numpy()
                    assert same_bits(y[:, :M], ref_all[:N, :M]), (t, form, K, M, N, fill)
                    assert np.all(y[:, M:].view(np.uint8) == fill), (t, form, K, M, N, "guard written")
                    outs.append(y[:, :M].copy())
            half = len(outs) // 2
            for a, b in zip(outs[:half], outs[half:]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (t, form, K, M, "the guard's bytes changed the result")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("t", TYPES)
def test_strided_operands(t, form):
    K, M, N = 96, 65, 5
    w_all, x_all, ref_all = _sweep_case(t, K)
    _, wv = _dev_w(t, w_all[:M], M + GUARD, K + 8, 0xFF)                      # a W pitch of 2 K + 16 bytes
    assert wv.stride(0) * 2 == 2 * K + 16
    xb = torch.full((N, K + 1), float("nan"), device="cuda"); xb[:, :K] = torch.from_numpy(x_all[:N]).cuda()      # x and y one element wider than dense
    yb = torch.full((N, M + 1), 7.0, device="cuda")
    G.mul_mat_fw(wv, xb[:, :K], out=yb[:, :M], flags=form)
    y = yb.cpu().numpy()
    assert same_bits(y[:, :M], ref_all[:N, :M]) and np.all(y[:, M] == 7.0)


def _specials(t):
    """x values: infinities, NaNs (quiet, signalling, payload in the low half only), subnormals of f32 and of the 16-bit type, exact ties of the conversion"""
    if t == "f16":
        ties = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 65504.0 + 16.0, 65504.0 + 15.9, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -25]
    else:
        ties = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 3.3895313892515355e38, 2.0 ** -127, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -149]
    v = np.array(ties + [0.0, -0.0, 1.0, -2.5], np.float32)
    bits = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFA00000, 0x7F80FFFF, 0x00000001, 0x807FFFFF], np.uint32).view(np.float32)
    return v, bits


@pytest.mark.parametrize("t", TYPES)
def test_conversion_of_x_through_an_identity_matrix(t):
    """W = the identity on K = 32: y[n][m] = the rounded x[n][m] exactly (every other product is a signed zero), so the output shows the conversion's bits
    on ties and subnormals.  Finite values only here: 0 * inf is a NaN."""
    v, _ = _specials(t)
    with np.errstate(all="ignore"):
        v = v[np.isfinite(v.astype(np.float16).astype(np.float32) if t == "f16" else bf16_to_f32(f32_to_bf16(v)))]      # (the tie that rounds up to inf: test_special_values)
    K = 32
    x = np.zeros((2, K), np.float32); x[0, :len(v)] = v; x[1, :len(v)] = -v
    eye = np.eye(K, dtype=np.float32)
    w_bits = eye.astype(np.float16).view(np.uint16) if t == "f16" else f32_to_bf16(eye)
    _, wv = _dev_w(t, w_bits, K, K, 0)
    y = G.mul_mat_fw(wv, torch.from_numpy(x).cuda()).cpu().numpy()
    with np.errstate(all="ignore"):
        want = x.astype(np.float16).astype(np.float32) if t == "f16" else bf16_to_f32(f32_to_bf16(x))
    want = want + np.float32(0.0)                                              # (a rounded -0 summed with the +0 products is +0)
    assert same_bits(y, want), (y.view(np.uint32), want.view(np.uint32))
    assert same_bits(y, _ref(t, w_bits, x))


@pytest.mark.parametrize("t", TYPES)
def test_special_values(t):
    """infinities, NaNs, subnormals and ties in x AND in W, against the restatements (a NaN must be a NaN; every other value bit for bit)"""
    K, M, N = 96, 17, 3
    rng = np.random.default_rng(5)
    v, bits = _specials(t)
    x = rng.standard_normal((N, K)).astype(np.float32)
    x[0, 3:3 + len(v)] = v                                                   # column 0: finite specials
    x[1, 40:40 + len(bits)] = bits                                           # column 1: inf / NaN
    w_bits = _w_host(t, M, K, 77)
    sub = np.array([0x0001, 0x8001, 0x03FF, 0x0200] if t == "f16" else [0x0001, 0x8001, 0x007F, 0x0040], np.uint16)
    w_bits[2, 5:9] = sub                                                      # subnormal weights
    w_bits[3, 10] = 0x7C00 if t == "f16" else 0x7F80                          # +inf
    w_bits[4, 11] = 0xFC00 if t == "f16" else 0xFF80                          # -inf
    w_bits[5, 12] = 0x7E01 if t == "f16" else 0x7FC1                          # NaN
    w_bits[6, 10] = 0x7C00 if t == "f16" else 0x7F80; w_bits[6, 42] = 0xFC00 if t == "f16" else 0xFF80      # inf - inf in one accumulator chain
    w_bits[7, :] = np.float16(60000.0).view(np.uint16) if t == "f16" else 0x7F00                             # sums that overflow to inf
    _, wv = _dev_w(t, w_bits, M, K, 0)
    y = G.mul_mat_fw(wv, torch.from_numpy(x).cuda()).cpu().numpy()
    want = _ref(t, w_bits, x)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    assert same_bits(y, want), (y, want)


@pytest.mark.parametrize("t", TYPES)
def test_exact_data_against_float64(t):
    """small integers times powers of two: every summation order gives the same f32, so the float64 product is the answer -- an indexing slip shows
    here whatever the order restatement says"""
    M, K, N = 1031, 2080, 8
    rng = np.random.default_rng(11)
    w = (rng.integers(-4, 5, (M, K)) * (2.0 ** rng.integers(-3, 3, (M, 1)))).astype(np.float32)
    x = (rng.integers(-4, 5, (N, K)) * (2.0 ** rng.integers(-3, 3, (N, 1)))).astype(np.float32)
    w_bits = w.astype(np.float16).view(np.uint16) if t == "f16" else f32_to_bf16(w)
    want = (x.astype(np.float64) @ w.astype(np.float64).T).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), x.astype(np.float64) @ w.astype(np.float64).T)          # exactly representable
    _, wv = _dev_w(t, w_bits, M, K, 0)
    xd = torch.from_numpy(x).cuda()
    for form in FORMS:
        y1 = G.mul_mat_fw(wv, xd, flags=form).cpu().numpy()
        y2 = G.mul_mat_fw(wv, xd, flags=form).cpu().numpy()
        assert np.array_equal(y1, want), (t, form)
        assert np.array_equal(y1.view(np.uint32), y2.view(np.uint32))          # two launches, identical bits


def test_bf16_same_bits_as_op_mul_mat_f():
    K, M, N = 2080, 65, 5
    w_all, x_all, ref_all = _sweep_case("bf16", K)
    _, wv = _dev_w("bf16", w_all[:M], M, K, 0)
    xd = torch.from_numpy(x_all[:N]).cuda()
    new = G.mul_mat_fw(wv, xd).cpu().numpy()
    old = G.op_mul_mat_f(wv, xd).cpu().numpy()
    assert np.array_equal(new.view(np.uint32), old.view(np.uint32)) and same_bits(new, ref_all[:N, :M])


@pytest.mark.parametrize("t", TYPES)
def test_refusals_leave_y_alone(t):
    M, N = 17, 2

    def refused(wv, xd, still=True, **kw):
        yb = torch.full((xd.shape[0], wv.shape[0]), 7.0, device="cuda")
        with pytest.raises(G.Mi355qError):
            G.mul_mat_fw(wv, xd, out=yb, **kw)
        torch.cuda.synchronize()
        assert bool((yb == 7.0).all())
        if still:                                                             # the old entry still computes it
            got = G.op_mul_mat_f(wv, xd).cpu().numpy()
            bits = wv.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
            want = _ref(t, bits, xd.cpu().numpy())
            if t == "bf16":
                assert same_bits(got, want)                                   # (bf16: the CPU's bits there too, tail in double included)
            else:
                assert np.allclose(got, want, rtol=1e-3, atol=1e-3)            # (f16: op_mul_mat_f sums lane-strided partials)

    for K in (100, 8):                                                        # K % 32, K < 32
        _, wv = _dev_w(t, _w_host(t, M, K, K), M, K + (-K) % 8, 0)
        refused(wv, torch.randn(N, K, device="cuda"))
    K = 64
    bits = _w_host(t, M, K, 3)
    _, wv = _dev_w(t, bits, M, K, 0)
    xd = torch.randn(9, K, device="cuda")
    refused(wv, xd)                                                           # N = 9
    refused(wv, xd[:0], still=False)                                          # N = 0
    flat = torch.zeros(4 + (M + 1) * (K + 8), dtype=torch.int16, device="cuda")
    off = flat[4:4 + M * K].view(M, K); off.copy_(torch.from_numpy(bits.view(np.int16)).cuda())
    assert off.data_ptr() % 16 == 8
    refused(off.view(_dt(t)), xd[:N])                                         # bit 3 of W's address
    torch.as_strided(flat, (M, K), (K + 4, 1)).copy_(torch.from_numpy(bits.view(np.int16)).cuda())
    refused(torch.as_strided(flat.view(_dt(t)), (M, K), (K + 4, 1)), xd[:N])                  # a W pitch of 2 K + 8
    refused(torch.as_strided(flat.view(_dt(t)), (M, K), (K - 8, 1)), xd[:N], still=False)       # a pitch below 2 K
    refused(wv, xd[:N], still=False, x_stride_bytes=4 * K + 2)               # an x pitch of 4 K + 2
    for other in (torch.zeros(M, K, device="cuda"), torch.zeros(M, K, dtype=torch.uint8, device="cuda")):      # type 0 (f32), a block type's bytes
        refused(other, xd[:N], still=False)
