"""Every tile form of the batched (N > 8) MUL_MAT / MUL_MAT_ID tiers, held to BIT EQUALITY.

The inputs are tests/qdata.py's exact data: every dequantized weight is a power of two times an integer below 256 (a bf16 number), every
activation a small integer, and sum |w| |x| stays below 2^24 units (asserted on each case's own data).  Every partial sum of every
summation order is then an exact f32, so the float64 product of the dequantized weights and the activations (qdata.exact_product -- the
only reference here) is what a correct kernel returns bit for bit, whatever its tile shape, K pieces or reduction order: one wrong row in
a tile, a tail row reading row 0, a dropped K-step of one split-K piece or a token stored to the wrong pair all show.

Which kernel form a shape gets is decided by the library from m, n, k and the CU count.  bf16_form / i8_form below mirror those rules
(csrc/mmq_bf16.hip launch_mmq_bf16, csrc/mmq_i8.hip launch_mmq_i8_multi) and tier() mirrors csrc/api.hip; every case first asserts that
its shape reaches the form it is named after ON THIS DEVICE -- another CU count fails loudly instead of testing something else.

Forms left out, and why: the planar K of Q6_K, IQ3_S and IQ3_XXS are multiples of 2048, of IQ4_XS multiples of 512, so their 128-k step
counts always divide by 4 (IQ4_XS) or by 4 and 8 (the other three): those types run the 4- / 8-piece forms at K = 4096 / 8192 with even
pieces (IQ4_XS: 8 uneven pieces at K = 8704), and meet an uneven step count in the 3-piece form (32 steps)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from qdata import (EXACT_CANONICAL_K, EXACT_FORM_KS, exact_acts, exact_blocks, exact_product, exact_sum_bound)
from test_gpu_parity import BLOCK32_TYPES, CANONICAL_BATCH_TYPES, check_close

pytestmark = pytest.mark.gpu
ids_t = lambda t: oracle.TYPE_NAMES[t]
Q = oracle

BF16_KERNEL_TYPES = (Q.Q4_K, Q.Q5_K, Q.Q6_K, Q.Q8_0, Q.Q4_0, Q.IQ4_NL, Q.IQ4_XS, Q.IQ3_S, Q.IQ3_XXS)      # instantiations of k_mmq_bf16
BF16_TIER_TYPES = (Q.Q5_K, Q.Q6_K, Q.Q4_0, Q.IQ4_NL, Q.IQ4_XS, Q.IQ3_S, Q.IQ3_XXS)                         # ... that land there with aligned operands


@pytest.fixture(scope="module")
def G():
    import torch
    import ggml_mi355 as g
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    assert g.lib().mi355q_device_count() >= 1, "libmi355q.so found no gfx950 device"
    return g


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def n_cu(G):
    cu = C.c_int(0)
    assert G.lib().mi355q_device_info(0, None, 0, None, None, C.byref(cu)) == 0
    assert cu.value > 0
    return cu.value


# ------------------------------------------------------------------------------------------------
# mirrors of the library's choices
# ------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def mmq_supported(t, k):
    if t in (Q.Q4_K, Q.Q5_K, Q.Q6_K, Q.IQ4_XS):
        return k % 256 == 0
    if t in (Q.IQ3_S, Q.IQ3_XXS):
        return k % 2048 == 0
    return t in (Q.Q8_0, Q.Q4_0, Q.IQ4_NL) and k % 128 == 0


def tier(G, t, k, n, x_aligned=True, y_aligned=True):
    """csrc/api.hip mi355q_mul_mat_multi for one matrix: "i8" | "q80" | "bf16" (matrix cores, planar rows), "canonical" (matrix cores,
    canonical rows), "gemv".  x_aligned / y_aligned: pointer and row stride are multiples of 16 bytes."""
    if G.is_planar(t, k):
        if n > 8 and mmq_supported(t, k) and y_aligned:
            if t == Q.Q4_K and x_aligned:
                return "i8"
            if t == Q.Q8_0 and k % 256 == 0 and x_aligned:
                return "q80"
            return "bf16"
        return "gemv"
    if n > 8 and t in CANONICAL_BATCH_TYPES and k % (128 if t in BLOCK32_TYPES else 256) == 0:
        return "canonical"
    return "gemv"


def bf16_splits(m, n, k, n_cu):
    t128 = cdiv(m, 128) * cdiv(n, 128)
    if 2 * t128 >= 3 * n_cu or k < 4096 or m % 4:
        return 1
    s = min(cdiv(2 * n_cu, t128), k // 128 // 8, 8)
    return s if s >= 2 else 1


def bf16_form(t, m, n, k, n_cu):
    """launch_mmq_bf16 with a workspace that holds the partial sums: (rows per tile, tokens per tile, K pieces)."""
    tiles = lambda bm, bn: cdiv(m, bm) * cdiv(n, bn)
    bm, bn = 64, 64
    if 2 * tiles(128, 128) >= 3 * n_cu:
        bm, bn = 128, 128
    elif tiles(128, 64) >= 2 * n_cu:
        bm, bn = 128, 64
    splits = bf16_splits(m, n, k, n_cu)
    if splits > 1:
        bm, bn = 128, 128
    if bm == 128 and bn == 128 and n >= 256 and t == Q.Q6_K and cdiv(m, 128) * cdiv(n, 256) * splits >= n_cu:
        bn = 256
    return bm, bn, splits


def i8_form(ms, n, k, n_cu):
    """launch_mmq_i8_multi for the row counts ms of one call: (cfg, K pieces); cfg 14 = 64 x 64 tiles, 28 = 128 x 128."""
    n_pad = cdiv(n, 128) * 128
    splits = 1
    if len(ms) == 1:
        m = ms[0]
        t128 = cdiv(m, 128) * (n_pad // 128)
        if not (2 * t128 >= 3 * n_cu or k < 8192 or m % 4):
            s = min((2 * n_cu + t128 - 1) // t128, k // 256 // 4, 8)
            splits = s if s >= 2 else 1
    wide = splits > 1 or 2 * sum(cdiv(m, 128) for m in ms) * (n_pad // 128) >= 3 * n_cu
    return (28 if wide else 14), splits


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
_WS = {}


def run_mul_mat(G, torch, w, x, y=None, flags=0):
    """mi355q_mul_mat with a scratch buffer that always has room for the partial sums of up to 8 K pieces, so the form depends on the
    shape alone (the library falls back to unsplit tiles when the caller's buffer is smaller)."""
    n = x.shape[0]
    y = y if y is not None else torch.empty((n, w.M), dtype=torch.float32, device="cuda")
    lib = G.lib()
    need = int(lib.mi355q_mul_mat_workspace(w.type, w.M, n, w.K)) + 8 * n * w.M * 4 + 1024
    if "buf" not in _WS or _WS["buf"].numel() < need:
        _WS["buf"] = torch.empty(need, dtype=torch.uint8, device="cuda")
    ws = _WS["buf"]
    rc = lib.mi355q_mul_mat(w.type, w.data.data_ptr(), w.row_bytes, x.data_ptr(), x.stride(0) * 4, y.data_ptr(), y.stride(0) * 4,
                            w.M, n, w.K, ws.data_ptr(), ws.numel(), flags, int(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mi355q_last_error().decode(errors="replace")
    torch.cuda.synchronize()
    return y


def assert_bits(y, exact, what, bm=64, bn=64):
    y = np.ascontiguousarray(y, np.float32); exact = np.ascontiguousarray(exact, np.float32)
    assert y.shape == exact.shape, (y.shape, exact.shape)
    bad = y.view(np.uint32) != exact.view(np.uint32)
    if bad.any():
        tok, row = map(int, np.argwhere(bad)[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} outputs differ; first at token {tok}, row {row} (row tile {row // bm} of {bm} rows, "
                    f"row {row % bm} in it; token tile {tok // bn} of {bn} tokens, token {tok % bn} in it): got {y[tok, row]!r}, exact {exact[tok, row]!r}; "
                    f"rows touched {np.unique(np.argwhere(bad)[:, 1])[:8]}, tokens touched {np.unique(np.argwhere(bad)[:, 0])[:8]}")


def exact_case(orc, t, M, N, K, kind, seed):
    rng = np.random.default_rng(seed)
    w = exact_blocks(t, M, K, rng)
    x = exact_acts(N, K, rng, kind)
    dq = orc.dequantize(t, w, K)
    b = exact_sum_bound(orc, t, w, x, K, dq)
    assert b < 2 ** 24, f"{ids_t(t)} {M}x{N}x{K}: sum |w||x| up to {b:.0f} units: the product is not order-independent"
    return w, x, exact_product(orc, t, w, x, K, dq)


def misaligned_rows(torch, x):
    """x as a device view whose row stride is K + 1 floats: 4-byte aligned, not 16."""
    n, k = x.shape
    wide = torch.zeros((n, k + 1), dtype=torch.float32, device="cuda")
    wide[:, :k] = torch.from_numpy(x).cuda()
    return wide[:, :k]


# ------------------------------------------------------------------------------------------------
# bf16 tier (csrc/mmq_bf16.hip): every form, for the seven types of the tier and for Q4_K / Q8_0 behind a misaligned x
# ------------------------------------------------------------------------------------------------
def k_small(t):
    return EXACT_FORM_KS[t][0]


def k_pieces(t, pieces):
    """K of the 4- / 8-piece forms: an uneven step count where the type's planar K allow one (module docstring)."""
    if t in (Q.Q6_K, Q.IQ3_S, Q.IQ3_XXS):
        return 1024 * pieces
    if t == Q.IQ4_XS:
        return 4096 if pieces == 4 else 8704
    return 4352 if pieces == 4 else 8448


# name -> (M, N, K(t), (bm, bn, pieces) expected; Q6_K's 256-token tile where n >= 256 covers the chip is named in Q6K_FORMS)
BF16_FORMS = {
    "64x64":   (200, 70, k_small, (64, 64, 1)),
    "128x64":  (12200, 330, k_small, (128, 64, 1)),
    "128x128": (12200, 400, k_small, (128, 128, 1)),
    "split4":  (512, 130, lambda t: k_pieces(t, 4), (128, 128, 4)),
    "split8":  (512, 130, lambda t: k_pieces(t, 8), (128, 128, 8)),
    "split2":  (12200, 330, lambda t: 4096, (128, 128, 2)),
    "split3":  (12200, 200, lambda t: 4096, (128, 128, 3)),
}
Q6K_FORMS = {"split2": (128, 256, 2)}          # 12200 x 330: 96 row tiles x 2 token tiles x 2 pieces >= 256 CUs


def run_bf16_form(G, torch, orc, n_cu, t, M, N, K, want, misalign, what):
    assert G.is_planar(t, K) and K in EXACT_FORM_KS[t], (ids_t(t), K)
    assert tier(G, t, K, N, x_aligned=not misalign) == "bf16", f"{what}: not on the bf16 tier"
    form = bf16_form(t, M, N, K, n_cu)
    assert form == want, f"{what}: on {n_cu} CUs the shape takes form {form}, the case is named after {want}"
    if want[2] > 1 and K // 128 % want[2]:
        assert K // 128 // want[2] >= 8                       # uneven pieces, each of at least 8 steps
    w, x, exact = exact_case(orc, t, M, N, K, "bf16", 1000 * t + M + N + K)
    wq = G.QWeight.from_host(t, w, M, K)
    xd = misaligned_rows(torch, x) if misalign else torch.from_numpy(x).cuda()
    assert (xd.stride(0) * 4) % 16 == (4 if misalign else 0) and xd.data_ptr() % 16 == 0
    y = run_mul_mat(G, torch, wq, xd).cpu().numpy()
    assert_bits(y, exact, what, want[0], want[1])
    y2 = run_mul_mat(G, torch, wq, xd).cpu().numpy()
    assert np.array_equal(y2.view(np.uint32), y.view(np.uint32)), f"{what}: a second launch differs"


@pytest.mark.parametrize("form", list(BF16_FORMS), ids=str)
@pytest.mark.parametrize("t", BF16_TIER_TYPES, ids=ids_t)
def test_bf16_forms(G, torch, orc, n_cu, t, form):
    M, N, kf, want = BF16_FORMS[form]
    if t == Q.Q6_K:
        want = Q6K_FORMS.get(form, want)
    run_bf16_form(G, torch, orc, n_cu, t, M, N, kf(t), want, False, f"{ids_t(t)} {form}")


@pytest.mark.parametrize("form", list(BF16_FORMS), ids=str)
@pytest.mark.parametrize("t", [Q.Q4_K, Q.Q8_0], ids=ids_t)
def test_bf16_forms_behind_misaligned_x(G, torch, orc, n_cu, t, form):
    """Q4_K and Q8_0 have integer tiers of their own; an x whose row stride is not a multiple of 16 bytes sends them to k_mmq_bf16."""
    M, N, kf, want = BF16_FORMS[form]
    assert tier(G, t, kf(t), N) in ("i8", "q80")
    run_bf16_form(G, torch, orc, n_cu, t, M, N, kf(t), want, True, f"{ids_t(t)} (x stride K+1) {form}")


@pytest.mark.parametrize("shape", [(16300, 300, 2048, (128, 256, 1)), (4096, 300, 4096, (128, 256, 4))], ids=["128x256", "128x256_split4"])
def test_bf16_q6_k_wide_token_tile(G, torch, orc, n_cu, shape):
    M, N, K, want = shape
    run_bf16_form(G, torch, orc, n_cu, Q.Q6_K, M, N, K, want, False, f"q6_K {want}")


# ------------------------------------------------------------------------------------------------
# integer tiers: Q4_K (csrc/mmq_i8.hip) and Q8_0 (csrc/mmq_q80.hip)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(200, 70, 256, (14, 1)), (12200, 400, 256, (28, 1)), (512, 130, 8192, (28, 8)), (512, 130, 8448, (28, 8))],
                         ids=["64x64", "128x128", "split8", "split8_uneven"])
def test_i8_forms_one_matrix(G, torch, orc, n_cu, shape):
    M, N, K, want = shape
    t = Q.Q4_K
    assert tier(G, t, K, N) == "i8"
    assert i8_form([M], N, K, n_cu) == want, f"on {n_cu} CUs the shape takes form {i8_form([M], N, K, n_cu)}, not {want}"
    w, x, exact = exact_case(orc, t, M, N, K, "q8_k", 31 + M + N + K)
    wq = G.QWeight.from_host(t, w, M, K); xd = torch.from_numpy(x).cuda()
    tile = 128 if want[0] == 28 else 64
    y = run_mul_mat(G, torch, wq, xd).cpu().numpy()
    assert_bits(y, exact, f"q4_K i8 {want}", tile, tile)
    assert np.array_equal(run_mul_mat(G, torch, wq, xd).cpu().numpy().view(np.uint32), y.view(np.uint32))


@pytest.mark.parametrize("case", [((96, 40, 24), 70, 14), ((6100, 4030, 2200), 400, 28)], ids=["64x64", "128x128"])
def test_i8_forms_three_matrices(G, torch, orc, n_cu, case):
    """Several matrices in ONE grid: their row blocks are concatenated (rb_begin), none a multiple of the tile's rows."""
    ms, N, cfg = case
    t, K = Q.Q4_K, 256
    assert tier(G, t, K, N) == "i8" and i8_form(list(ms), N, K, n_cu) == (cfg, 1), i8_form(list(ms), N, K, n_cu)
    tile = 128 if cfg == 28 else 64
    assert all(m % tile for m in ms)
    rng = np.random.default_rng(55 + N)
    hosts = [exact_blocks(t, m, K, rng) for m in ms]
    x = exact_acts(N, K, rng, "q8_k")
    ws = [G.QWeight.from_host(t, h, m, K) for h, m in zip(hosts, ms)]
    xd = torch.from_numpy(x).cuda()
    for rep in range(2):
        ys = G.mul_mat_multi(ws, xd)
        torch.cuda.synchronize()
        for i, (h, m, y) in enumerate(zip(hosts, ms, ys)):
            assert exact_sum_bound(orc, t, h, x, K) < 2 ** 24
            assert_bits(y.cpu().numpy(), exact_product(orc, t, h, x, K), f"q4_K matrix {i} of {ms}, launch {rep}", tile, tile)


@pytest.mark.parametrize("round_even", [False, True], ids=["round_away", "round_even"])
def test_q80_forms(G, torch, orc, round_even):
    t, K = Q.Q8_0, 256
    flags = 0x1 if round_even else 0x0
    w, x, exact = exact_case(orc, t, 200, 70, K, "q8_0", 66)
    assert tier(G, t, K, 70) == "q80"
    wq = G.QWeight.from_host(t, w, 200, K); xd = torch.from_numpy(x).cuda()
    y = run_mul_mat(G, torch, wq, xd, flags=flags).cpu().numpy()
    assert_bits(y, exact, "q8_0 q80 one matrix")
    assert np.array_equal(run_mul_mat(G, torch, wq, xd, flags=flags).cpu().numpy().view(np.uint32), y.view(np.uint32))
    ms = (96, 40, 200)
    rng = np.random.default_rng(67)
    hosts = [exact_blocks(t, m, K, rng) for m in ms]
    ws = [G.QWeight.from_host(t, h, m, K) for h, m in zip(hosts, ms)]
    ys = G.mul_mat_multi(ws, xd, flags=flags)
    torch.cuda.synchronize()
    for i, (h, y) in enumerate(zip(hosts, ys)):
        assert exact_sum_bound(orc, t, h, x, K) < 2 ** 24
        assert_bits(y.cpu().numpy(), exact_product(orc, t, h, x, K), f"q8_0 matrix {i} of {ms}")


# ------------------------------------------------------------------------------------------------
# canonical rows (csrc/mmq_generic.hip)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(200, 70), (67, 9)], ids=str)
@pytest.mark.parametrize("t", CANONICAL_BATCH_TYPES, ids=ids_t)
def test_canonical_rows_exact(G, torch, orc, t, shape):
    M, N = shape
    K = EXACT_CANONICAL_K[t]
    assert tier(G, t, K, N) == "canonical"
    w, x, exact = exact_case(orc, t, M, N, K, "bf16", 7 * t + M)
    wq = G.QWeight.from_host(t, w, M, K); xd = torch.from_numpy(x).cuda()
    y = run_mul_mat(G, torch, wq, xd).cpu().numpy()
    assert_bits(y, exact, f"{ids_t(t)} canonical {M}x{N}x{K}")
    assert np.array_equal(run_mul_mat(G, torch, wq, xd).cpu().numpy().view(np.uint32), y.view(np.uint32))


# ------------------------------------------------------------------------------------------------
# strided operands, one representative per tier
# ------------------------------------------------------------------------------------------------
STRIDED = [(Q.Q4_K, 256, "q8_k", "i8"), (Q.Q8_0, 256, "q8_0", "q80"), (Q.Q6_K, 2048, "bf16", "bf16"), (Q.IQ3_S, 2048, "bf16", "bf16"),
           (Q.Q2_K, 256, "bf16", "canonical")]
SENTINEL = -12345.5


@pytest.mark.parametrize("rep", STRIDED, ids=lambda r: ids_t(r[0]))
def test_strided_operands(G, torch, orc, rep):
    t, K, kind, want_tier = rep
    # (1) x rows K + 4 floats apart, y rows M + 4 floats apart behind out=: both strides are multiples of 16 bytes, the tier is kept
    M, N = 200, 70
    assert tier(G, t, K, N) == want_tier
    w, x, exact = exact_case(orc, t, M, N, K, kind, 90 + t)
    wq = G.QWeight.from_host(t, w, M, K)
    xw = torch.full((N, K + 4), 3.0e30, dtype=torch.float32, device="cuda")           # (a kernel reading past a row's K meets this)
    xw[:, :K] = torch.from_numpy(x).cuda()
    yw = torch.full((N, M + 4), SENTINEL, dtype=torch.float32, device="cuda")
    run_mul_mat(G, torch, wq, xw[:, :K], y=yw[:, :M])
    got = yw.cpu().numpy()
    assert_bits(got[:, :M], exact, f"{ids_t(t)} strided x and y")
    assert (got[:, M:] == SENTINEL).all(), "padding floats behind the result rows were written"
    # (2) M = 131 behind a y stride of 132 floats: still 16-byte aligned rows, so the matrix cores keep the call and the f32x4 epilogue
    # runs its scalar tail; the padding column stays untouched
    M = 131
    assert tier(G, t, K, N, y_aligned=True) == want_tier
    w, x, exact = exact_case(orc, t, M, N, K, kind, 91 + t)
    wq = G.QWeight.from_host(t, w, M, K)
    yw = torch.full((N, 132), SENTINEL, dtype=torch.float32, device="cuda")
    assert yw.data_ptr() % 16 == 0
    run_mul_mat(G, torch, wq, torch.from_numpy(x).cuda(), y=yw[:, :M])
    got = yw.cpu().numpy()
    assert_bits(got[:, :M], exact, f"{ids_t(t)} M=131 behind a 132-float stride")
    assert (got[:, M:] == SENTINEL).all(), "the padding column was written"
    # (3) y rows 133 floats apart: not 16-byte aligned.  Planar types must drop to the GEMV tier (the CPU's arithmetic with quantized
    # activations: the oracle's tolerance, not equality); canonical rows have no alignment contract and stay exact
    yw = torch.full((N, 133), SENTINEL, dtype=torch.float32, device="cuda")
    run_mul_mat(G, torch, wq, torch.from_numpy(x).cuda(), y=yw[:, :M])
    got = yw.cpu().numpy()
    assert tier(G, t, K, N, y_aligned=False) == ("canonical" if want_tier == "canonical" else "gemv")
    if want_tier == "canonical":
        assert_bits(got[:, :M], exact, f"{ids_t(t)} unaligned y rows")
    else:
        check_close(got[:, :M], orc.mul_mat(t, w, x, M, N, K), f"{ids_t(t)} unaligned y rows (GEMV tier)")
    assert (got[:, M:] == SENTINEL).all()


# ------------------------------------------------------------------------------------------------
# grouped MUL_MAT_ID: segment edges built by hand
# ------------------------------------------------------------------------------------------------
N_EXPERT, N_USED = 8, 2
MOE_LAYOUTS = {
    "edges":     ([0, 2, 63, 64, 65, 127, 128, 129], 0),       # per-expert pair counts: empty, tiny, one short of / exactly / one past a 64- and a 128-token tile
    "one":       ([0, 0, 0, 0, 0, 578, 0, 0], 0),              # every pair on one expert
    "edges_bad": ([0, 1, 63, 64, 65, 127, 128, 129], 1),       # ... and one id out of range among them
}
# (type, K, activation kind, token tile of the segments)
MOE_TYPES = [(Q.Q4_K, 256, "q8_k", 64), (Q.Q8_0, 256, "q8_0", 64), (Q.Q6_K, 2048, "bf16", 128), (Q.IQ4_XS, 512, "bf16", 128),
             (Q.Q4_1, 128, "bf16", 64), (Q.IQ2_XS, 256, "bf16", 64)]


def moe_ids(counts, n_bad, rng):
    flat = np.concatenate([np.full(c, e, np.int32) for e, c in enumerate(counts)] + [np.full(n_bad, N_EXPERT, np.int32)])
    assert flat.size % N_USED == 0
    rng.shuffle(flat)
    return flat.reshape(-1, N_USED)


def moe_tile_mirror(G, t, k):
    """csrc/api.hip moe_tile: 64-token segments on the integer tiers and for canonical rows, 128 on the bf16 tier."""
    if not G.is_planar(t, k):
        return 64
    return 64 if tier(G, t, k, 9) in ("i8", "q80") else 128


@pytest.mark.parametrize("layout", list(MOE_LAYOUTS), ids=str)
@pytest.mark.parametrize("spec", MOE_TYPES, ids=lambda s: ids_t(s[0]))
def test_grouped_mul_mat_id_segment_edges(G, torch, orc, spec, layout):
    t, K, kind, tile = spec
    counts, n_bad = MOE_LAYOUTS[layout]
    assert moe_tile_mirror(G, t, K) == tile and tier(G, t, K, 64) != "gemv"
    if tile == 128 and layout.startswith("edges"):
        assert any(0 < c % 128 <= 64 for c in counts if c)    # a half-empty 128-token tile: its upper waves skip their MFMAs
    rng = np.random.default_rng(400 + t + len(layout))
    ids = moe_ids(counts, n_bad, rng)
    n_tok = ids.shape[0]
    assert n_tok * N_USED >= 17                               # the grouped form
    for M in ((64, 66) if not G.is_planar(t, K) else (64,)):  # canonical rows: also result rows that are not 16-byte aligned
        as_ = exact_blocks(t, N_EXPERT * M, K, rng)
        w = G.QWeight.from_host(t, as_, M, K, n_expert=N_EXPERT)
        for x_ne1 in (1, N_USED):
            x = exact_acts(n_tok * x_ne1, K, rng, kind)
            assert exact_sum_bound(orc, t, as_, x, K) < 2 ** 24
            x3 = x.reshape(n_tok, x_ne1, K)
            wide = torch.full((n_tok, 5), 7777, dtype=torch.int32, device="cuda")      # ids as a strided view of a wider tensor
            wide[:, 1:3] = torch.from_numpy(ids).cuda()
            for ids_d in (torch.from_numpy(ids).cuda(), wide[:, 1:3]) if x_ne1 == 1 else (torch.from_numpy(ids).cuda(),):
                y = G.mul_mat_id(w, torch.from_numpy(x3).cuda(), ids_d)
                torch.cuda.synchronize()
                y = y.cpu().numpy().reshape(n_tok * N_USED, M)
                flat = ids.reshape(-1)
                xp = x3[np.arange(flat.size) // N_USED, (np.arange(flat.size) % N_USED) % x_ne1]
                ref = np.full((flat.size, M), np.nan, np.float32)
                rows = as_.reshape(N_EXPERT, M, -1)
                for e in range(N_EXPERT):
                    sel = np.flatnonzero(flat == e)
                    assert len(sel) == counts[e]
                    if len(sel):
                        ref[sel] = exact_product(orc, t, rows[e], xp[sel], K)
                bad = flat >= N_EXPERT
                assert bad.sum() == n_bad
                what = f"{ids_t(t)} {layout} M={M} x_ne1={x_ne1} ids stride {ids_d.stride(0)}"
                assert np.isnan(y[bad]).all(), f"{what}: an out-of-range id did not give a NaN row"
                assert not np.isnan(y[~bad]).any(), f"{what}: NaN in the row of a valid pair"
                assert_bits(y[~bad], ref[~bad], what)
