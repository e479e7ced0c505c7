"""Every form of the per-column (GEMV) tiers of MUL_MAT / MUL_MAT_ID, held to BIT EQUALITY: k_gemv_fast on planar rows (csrc/gemv_fast.hip)
and k_gemv_generic on canonical rows (csrc/gemv_generic.hip).  They run for N <= 8, for MUL_MAT_ID up to 16 pairs and for planar IQ3 at
every pair count -- every generated token -- and the decode plan's GEMV stages are checked against them, so an error here carries on.

The inputs are tests/qdata.py's exact data: every dequantized weight is a power of two times an integer below 256, every activation block
is identity-quantized by the CPU's quantizer (integer quants, d = 1, or d = 2^e with per-block factors: a kernel that reads another block's
d is then wrong), and sum (|w| + 2 mins) |x| of each output stays below 2^24 smallest units (asserted on each case's own data; proven for
every (type, K, amplitude, factors) of qdata.GEMV_FORM_DATA on the CPU in tests/test_exact_data_cpu.py).  Every partial sum of every order
is then an exact f32, so the float64 product (qdata.exact_product -- the only reference here) is what a correct kernel returns bit for bit:
one wrong lane, the wrong block's scale, a ring item consumed against the wrong row or a dropped step all show.

Which kernel and which launch geometry a shape gets is decided by the library from the type, n, k and the CU count.  The helpers below
mirror that arithmetic (csrc/gemv_fast.hip gemv_fast_max_cols / launch_cols / launch_gemv_fast_typed, csrc/api.hip mi355q_mul_mat_multi)
and every case first asserts that its shape has the property it is named after ON THIS DEVICE: another CU count fails loudly instead of
testing something else.  Every output buffer is filled with a canary beforehand (the gaps between rows of a strided y and a guard in front
of and behind the buffer included) and everything outside the expected elements must come back untouched; every case runs twice.
The mirrors are checked against the expected constants only -- the library exports none of that arithmetic -- so a change of the library's
ring depths, LDS budget or grid rule has to be carried into them by hand, or a case would run another form than the one it is named after.

Left out: k_gemv_generic<Q4_K> and k_gemv_generic<Q5_K> cannot be reached through the C ABI -- rows of those types are planar at every
valid K (multiples of 256), and no flag sends planar rows to the generic kernel (MI355Q_FLAG_FORCE_GENERIC only keeps canonical rows off
the batched canonical tier)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from qdata import (GEMV_ACT_KIND, GEMV_FORM_DATA, GEMV_PLANAR_TYPES, exact_acts, exact_blocks, exact_output_bound, exact_product,
                   exact_product_rows, GEMV_CANONICAL_BATCH_TYPES, gemv_amplitude, gemv_canonical_ks, gemv_ring_k, gemv_small_k)

pytestmark = pytest.mark.gpu
ids_t = lambda t: oracle.TYPE_NAMES[t]
Q = oracle

ROUND_EVEN, FORCE_GEMV = 0x1, 0x4                         # MI355Q_FLAG_*
Q80_FAMILY = (Q.Q8_0, Q.Q4_0, Q.IQ4_NL)                   # Q8_0 activations: one kernel per rounding flag
GENERIC_TYPES = tuple(t for t in GEMV_ACT_KIND if t not in (Q.Q4_K, Q.Q5_K))
CANARY = 0x7FA5A5A5                                       # a NaN no kernel writes (the row of an out-of-range id is 0x7FC00000)
NAN_FILL = 0x7FC00000                                     # what both kernels store for such a row
GUARD = 64                                                # floats in front of and behind every output buffer
_TABLE = set(GEMV_FORM_DATA)


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


@pytest.fixture(scope="module", autouse=True)
def release_device_buffers():
    """The shared data sets and the scratch buffer live for this module only."""
    yield
    _SHARED.clear()
    _WS.clear()


@pytest.fixture(scope="module")
def n_cu(G):
    cu = C.c_int(0)
    assert G.lib().mi355q_device_info(0, None, 0, None, None, C.byref(cu)) == 0
    assert cu.value > 0
    return cu.value


# ------------------------------------------------------------------------------------------------
# mirrors of the library's launch arithmetic
# ------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return (a + b - 1) // b


def col_bytes(t, k):
    """LDS bytes of one quantized activation column (csrc/gemv_stream.cuh lds_col_bytes, rounded up to 16)."""
    b = k + (k // 32) * 8 if t in Q80_FAMILY else k + (k // 256) * 4 + (k // 16) * 4
    return (b + 15) & ~15


def max_cols(t, k):
    """gemv_fast_max_cols: columns whose LDS image fits beside the IQ3 code book."""
    book = {Q.IQ3_S: 2048, Q.IQ3_XXS: 1024}.get(t, 0)
    return min(8, (160 * 1024 - 1024 - book) // col_bytes(t, k))


def steps_per_row(t, k):
    return cdiv(k // 16 if t == Q.Q8_0 else k // 32, 64)


def last_step_chunks(t, k):
    c = k // 16 if t == Q.Q8_0 else k // 32
    return c - 64 * (steps_per_row(t, k) - 1)


def ring_depth(t, ncols):
    """launch_cols: steps in flight per wave."""
    if ncols == 1:
        return 6 if t == Q.Q5_K else 8
    if ncols == 2:
        return 4 if t == Q.Q5_K else 6
    return 3 if ncols <= 4 else 2


def fast_grid(rows, n_cu, pairs=1):
    """launch_gemv_fast_typed: (rows per workgroup, workgroups along x)."""
    grid = max(n_cu // pairs, 1)
    rpw = max(cdiv(rows, grid), 1)
    return rpw, cdiv(rows, rpw)


def col_tiles(t, k, n):
    """mi355q_mul_mat_multi: the column counts of the launches that cover n columns."""
    mc = max_cols(t, k)
    return [min(mc, n - n0) for n0 in range(0, n, mc)]


def act_passes(k):
    """quantize_columns_to_lds: 16 waves take two 256-element spans each per pass."""
    return cdiv(k, 8192)


# ------------------------------------------------------------------------------------------------
# data
# ------------------------------------------------------------------------------------------------
def form_data(t, k, scaled):
    amp, fac = gemv_amplitude(k, scaled)
    assert (t, k, amp, fac) in _TABLE, f"({ids_t(t)}, K={k}, {'factors' if scaled else 'identity'}) is not in qdata.GEMV_FORM_DATA"
    return amp, fac


def make_acts(t, n, k, rng, scaled):
    amp, fac = form_data(t, k, scaled)
    return exact_acts(n, k, rng, GEMV_ACT_KIND[t], amp, fac)


def assert_bound(orc, t, w, x, k, dq, what):
    b = exact_output_bound(orc, t, w, x, k, dq)
    assert b < 2 ** 24, f"{what}: sum (|w| + 2 mins) |x| up to {b:.0f} units: the product is not order-independent"


def exact_case(orc, t, M, N, K, scaled, seed):
    rng = np.random.default_rng(seed)
    w = exact_blocks(t, M, K, rng)
    x = make_acts(t, N, K, rng, scaled)
    dq = orc.dequantize(t, w, K)
    assert_bound(orc, t, w, x, K, dq, f"{ids_t(t)} {M}x{N}x{K}")
    return w, x, exact_product_rows(orc, t, w, x, K, dq)


def assert_bits(y, exact, what):
    y = np.ascontiguousarray(y, np.float32); exact = np.ascontiguousarray(exact, np.float32)
    assert y.shape == exact.shape, (y.shape, exact.shape)
    bad = y.view(np.uint32) != exact.view(np.uint32)
    if bad.any():
        col, row = map(int, np.argwhere(bad)[0])
        untouched = int((y.view(np.uint32)[bad] == CANARY).sum())
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} outputs differ ({untouched} of them never written); first at column {col}, row {row}: "
                    f"got {y[col, row]!r}, exact {exact[col, row]!r}; rows touched {np.unique(np.argwhere(bad)[:, 1])[:8]}, "
                    f"columns touched {np.unique(np.argwhere(bad)[:, 0])[:8]}")


# ------------------------------------------------------------------------------------------------
# device operands built by hand: the strides, offsets and workspaces are the test's own
# ------------------------------------------------------------------------------------------------
class DevWeights:
    """Device rows of n_expert matrices of M rows: row stride row_bytes + pad, expert stride M * row stride + expert_pad; the padding bytes
    hold 0xA5 and unchanged() checks that no byte of the buffer was written."""

    def __init__(self, G, torch, t, host, M, K, n_expert=1, pad=0, expert_pad=0):
        q = G.QWeight.from_host(t, host, M, K, n_expert)          # (rows are packed one by one: a row's planes lie inside its row_bytes)
        self.type, self.M, self.rb = t, M, q.row_bytes
        self.stride = self.rb + pad
        self.estride = self.stride * M + expert_pad
        if pad == 0 and expert_pad == 0:
            self.buf = q.data
        else:
            self.buf = torch.full((n_expert * self.estride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            dst = self.buf.as_strided((n_expert, M, self.rb), (self.estride, self.stride, 1))
            dst.copy_(q.data[:n_expert * M * self.rb].view(n_expert, M, self.rb))
        self.ptr = self.buf.data_ptr()
        self.before = self.buf.clone()
        self.torch = torch

    def unchanged(self):
        return bool(self.torch.equal(self.buf, self.before))


def dev_x(torch, x, mode):
    """(keep-alive tensor, pointer, row stride in bytes): "aligned" | "stride1" (rows K + 1 floats apart) | "off4" (base 4 bytes past a
    multiple of 16).  The last two make the kernel fetch the activations float by float (x_vec == 0)."""
    n, k = x.shape
    if mode == "aligned":
        t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        ptr, stride = t.data_ptr(), 4 * k
    elif mode == "stride1":
        t = torch.full((n, k + 1), 3.0e30, dtype=torch.float32, device="cuda")      # (a kernel reading past a row's K meets this)
        t[:, :k] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        ptr, stride = t.data_ptr(), 4 * (k + 1)
    else:
        assert mode == "off4", mode
        t = torch.full((n * k + 8,), 3.0e30, dtype=torch.float32, device="cuda")
        t[1:1 + n * k] = torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda()
        ptr, stride = t.data_ptr() + 4, 4 * k
    assert (((ptr | stride) & 15) == 0) == (mode == "aligned")
    return t, ptr, stride


class OutBuf:
    """n result rows `stride` floats apart, a guard in front and behind, everything filled with the canary."""

    def __init__(self, torch, n, m, stride):
        assert stride >= m
        self.n, self.m, self.stride = n, m, stride
        self.buf = torch.full((GUARD + n * stride + GUARD,), CANARY, dtype=torch.int32, device="cuda")
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def read(self, what):
        """The n x m results, after checking that nothing else was written."""
        bits = self.buf.cpu().numpy().view(np.uint32)
        body = bits[GUARD:GUARD + self.n * self.stride].reshape(self.n, self.stride)
        assert (bits[:GUARD] == CANARY).all(), f"{what}: floats in front of the result buffer were written"
        assert (bits[GUARD + self.n * self.stride:] == CANARY).all(), f"{what}: floats behind the result buffer were written"
        assert (body[:, self.m:] == CANARY).all(), f"{what}: the gap between result rows was written"
        return np.ascontiguousarray(body[:, :self.m]).view(np.float32)


_WS = {}


def workspace(torch, nbytes):
    if "buf" not in _WS or _WS["buf"].numel() < nbytes:
        _WS["buf"] = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device="cuda")
    return _WS["buf"]


def launch_multi(G, torch, mats, xptr, xstride, n, k, flags=0):
    """mi355q_mul_mat_multi; mats: (type, w pointer, w stride, y pointer, y stride in bytes, m)."""
    lib = G.lib()
    arr = (G._Mat * len(mats))(*[G._Mat(*m) for m in mats])
    ws = workspace(torch, max(int(lib.mi355q_mul_mat_workspace(m[0], m[5], n, k)) for m in mats) + 1024)
    rc = lib.mi355q_mul_mat_multi(arr, len(mats), xptr, xstride, n, k, ws.data_ptr(), ws.numel(), flags, int(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.mi355q_last_error().decode(errors="replace")
    torch.cuda.synchronize()


def run_single(G, torch, W, t, M, N, K, x, exact, what, flags=(0,), x_mode="aligned", y_gap=0):
    """One matrix through mi355q_mul_mat_multi, twice per flag: bits equal to `exact`, canaries intact, weights unwritten."""
    assert x.shape == (N, K) and exact.shape == (N, M)
    keep, xptr, xstride = dev_x(torch, x, x_mode)
    stride = M + y_gap
    for fl in flags:
        first = None
        for rep in range(2):
            out = OutBuf(torch, N, M, stride)
            launch_multi(G, torch, [(t, W.ptr, W.stride, out.ptr, 4 * stride, M)], xptr, xstride, N, K, fl)
            got = out.read(f"{what} flags {fl:#x} launch {rep}")
            assert_bits(got, exact, f"{what} flags {fl:#x} launch {rep}")
            if first is None:
                first = got
            assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), f"{what}: a second launch differs"
    assert W.unchanged(), f"{what}: the weight buffer was written"
    del keep


def flags_of(t):
    """Both rounding flags for the Q8_0-activation family (distinct kernels; on identity-quantized data both give the exact answer)."""
    return (0, ROUND_EVEN) if t in Q80_FAMILY else (0,)


# one data set of 8 columns per (type, K, M), shared by the column counts 1..8 (its first n columns); entries of other types are dropped.
# (The type is the outer parameter of the tests that use it: in another order the data would only be rebuilt more often, never wrong.)
_SHARED = {}


def shared_case(G, torch, orc, t, M, K):
    key = (t, K, M)
    if key not in _SHARED:
        for k_ in [k_ for k_ in _SHARED if k_[0] != t]:
            del _SHARED[k_]
        w, x, exact = exact_case(orc, t, M, 8, K, True, 5000 + 100 * t + K + M)
        _SHARED[key] = (DevWeights(G, torch, t, w, M, K), x, exact)
    return _SHARED[key]


# ------------------------------------------------------------------------------------------------
# planar streaming tier: every type x every column count
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(1, 9), ids=lambda n: f"n{n}")
@pytest.mark.parametrize("t", GEMV_PLANAR_TYPES, ids=ids_t)
def test_fast_single_step_rows(G, torch, orc, n_cu, t, n):
    """The type's smallest planar K: a row is ONE step (a partial one wherever the type has a planar K below a full step)."""
    K = gemv_small_k(t)
    M = 2 * n_cu + 19
    assert G.is_planar(t, K) and steps_per_row(t, K) == 1 and n <= max_cols(t, K)
    assert (last_step_chunks(t, K) < 64) == (t not in (Q.Q6_K, Q.IQ3_S, Q.IQ3_XXS))
    rpw, grid = fast_grid(M, n_cu)
    assert rpw == 3 and grid > 1
    W, x, exact = shared_case(G, torch, orc, t, M, K)
    run_single(G, torch, W, t, M, n, K, x[:n], exact[:n], f"{ids_t(t)} n={n} K={K} (one step)", flags=flags_of(t))


@pytest.mark.parametrize("n", range(1, 9), ids=lambda n: f"n{n}")
@pytest.mark.parametrize("t", GEMV_PLANAR_TYPES, ids=ids_t)
def test_fast_ring_across_rows(G, torch, orc, n_cu, t, n):
    """steps % D != 0 with waves that own 3 rows: ring items straddle row boundaries, the refill of the last rows' items finds the wave's
    stream exhausted, the last step is partial where the type has such a K, and the last workgroup's range is short."""
    D = ring_depth(t, n)
    steps = 2 if D == 3 else 3
    K = gemv_ring_k(t, steps)
    M = 36 * n_cu - 5
    assert G.is_planar(t, K) and steps_per_row(t, K) == steps and steps % D != 0 and n <= max_cols(t, K)
    assert (last_step_chunks(t, K) < 64) == (t not in (Q.Q6_K, Q.IQ3_S, Q.IQ3_XXS))
    rpw, grid = fast_grid(M, n_cu)
    assert rpw == 36 and rpw % 16 and cdiv(rpw, 16) == 3, "a workgroup of 36 rows: waves 0..3 own 3 rows, the others 2"
    assert 0 < M - (grid - 1) * rpw < rpw, "the last workgroup's range is short"
    W, x, exact = shared_case(G, torch, orc, t, M, K)
    run_single(G, torch, W, t, M, n, K, x[:n], exact[:n], f"{ids_t(t)} n={n} K={K} ({steps} steps, D={D})", flags=flags_of(t))


@pytest.mark.parametrize("scaled", [False, True], ids=["identity", "factors"])
@pytest.mark.parametrize("K", [6144, 12288, 16640], ids=lambda k: f"K{k}")
@pytest.mark.parametrize("t", [Q.Q4_K, Q.Q4_0], ids=ids_t)
def test_fast_activation_passes(G, torch, orc, t, K, scaled):
    """The prologue quantizes 8192 activations per pass: K in (4096, 8192], (8192, 16384] and above 16384 run 1, 2 and 3 passes (the
    second half of the last pass out of range), for a K-quant and a 32-block type."""
    M, N = 70, 2
    assert G.is_planar(t, K) and act_passes(K) == {6144: 1, 12288: 2, 16640: 3}[K] and N <= max_cols(t, K)
    w, x, exact = exact_case(orc, t, M, N, K, scaled, 6000 + t + K)
    run_single(G, torch, DevWeights(G, torch, t, w, M, K), t, M, N, K, x, exact, f"{ids_t(t)} K={K} ({act_passes(K)} passes)", flags=flags_of(t))


# (type, K, N, flags, column tiles expected)
TILE_CASES = {
    "q4_K_n8_k16384": (Q.Q4_K, 16384, 8, 0, [7, 1]),
    "q4_0_n8_k16384": (Q.Q4_0, 16384, 8, 0, [7, 1]),
    "q4_K_n7_k28672": (Q.Q4_K, 28672, 7, 0, [4, 3]),
    "q6_K_force_n9":  (Q.Q6_K, 2048, 9, FORCE_GEMV, [8, 1]),
    "q6_K_force_n17": (Q.Q6_K, 2048, 17, FORCE_GEMV, [8, 8, 1]),
    "q8_0_force_n9":  (Q.Q8_0, 256, 9, FORCE_GEMV, [8, 1]),
    "iq3_s_force_n17": (Q.IQ3_S, 2048, 17, FORCE_GEMV, [8, 8, 1]),
}


@pytest.mark.parametrize("name", list(TILE_CASES), ids=str)
def test_fast_column_tiles(G, torch, orc, name):
    """mi355q_mul_mat_multi covers n columns with launches of at most gemv_fast_max_cols columns: x and y advance by whole tiles."""
    t, K, N, flags, tiles = TILE_CASES[name]
    M = 40
    assert G.is_planar(t, K) and col_tiles(t, K, N) == tiles, (max_cols(t, K), col_tiles(t, K, N))
    assert N <= 8 or flags & FORCE_GEMV
    w, x, exact = exact_case(orc, t, M, N, K, True, 7000 + t + K + N)
    run_single(G, torch, DevWeights(G, torch, t, w, M, K), t, M, N, K, x, exact, name, flags=(flags,), y_gap=3)


def geometry_rows(name, n_cu):
    """Row counts derived from the CU count; each is asserted to have the property it is named after."""
    if name == "one_row":
        return 1
    if name == "below_a_wave_stride":
        return 13
    if name == "cu_plus_1":
        return n_cu + 1
    if name == "short_last_workgroup":                        # rows per workgroup 21 (no multiple of 16), the last workgroup holds fewer than 16
        for M in range(20 * n_cu + 1, 21 * n_cu + 1):
            rpw, grid = fast_grid(M, n_cu)
            if rpw == 21 and 0 < M - (grid - 1) * rpw < 16:
                return M
        raise AssertionError(f"no row count with 21 rows per workgroup and a last workgroup below 16 rows on {n_cu} CUs")
    assert name == "odd_rows_per_workgroup"
    return 5 * n_cu - 3


@pytest.mark.parametrize("name", ["one_row", "below_a_wave_stride", "cu_plus_1", "short_last_workgroup", "odd_rows_per_workgroup"], ids=str)
@pytest.mark.parametrize("spec", [(Q.Q4_K, 2), (Q.Q8_0, 1), (Q.IQ3_XXS, 3)], ids=lambda s: f"{ids_t(s[0])}_n{s[1]}")
def test_fast_row_geometry(G, torch, orc, n_cu, spec, name):
    t, N = spec
    K = gemv_small_k(t)
    M = geometry_rows(name, n_cu)
    rpw, grid = fast_grid(M, n_cu)
    last = M - (grid - 1) * rpw
    want = {"one_row": (rpw, grid) == (1, 1), "below_a_wave_stride": rpw == 1 and grid == M < 16, "cu_plus_1": rpw == 2 and last == 1,
            "short_last_workgroup": rpw == 21 and last < 16, "odd_rows_per_workgroup": rpw == 5 and 0 < last < rpw}[name]
    assert want, f"{name}: M={M} gives {rpw} rows per workgroup, {grid} workgroups, {last} rows in the last on {n_cu} CUs"
    w, x, exact = exact_case(orc, t, M, N, K, True, 8000 + t + M)
    run_single(G, torch, DevWeights(G, torch, t, w, M, K), t, M, N, K, x, exact, f"{ids_t(t)} {name} M={M}", flags=flags_of(t))


@pytest.mark.parametrize("layout", ["w_stride", "y_stride", "x_stride_k_plus_1", "x_base_off_4"], ids=str)
@pytest.mark.parametrize("t", [Q.Q4_K, Q.Q6_K, Q.IQ3_S, Q.Q8_0, Q.IQ4_NL], ids=ids_t)
def test_fast_operand_layout(G, torch, orc, t, layout):
    """Strided weights (padding canaried), y rows wider than an odd M, and the two x layouts that turn the float4 fetch off."""
    K = gemv_ring_k(t, 2)
    M, N = 77, 3
    assert G.is_planar(t, K)
    w, x, exact = exact_case(orc, t, M, N, K, True, 9000 + t)
    W = DevWeights(G, torch, t, w, M, K, pad=48 if layout == "w_stride" else 0)
    assert W.stride % 16 == 0 and (W.stride > W.rb) == (layout == "w_stride")
    x_mode = {"x_stride_k_plus_1": "stride1", "x_base_off_4": "off4"}.get(layout, "aligned")
    run_single(G, torch, W, t, M, N, K, x, exact, f"{ids_t(t)} {layout}", flags=flags_of(t), x_mode=x_mode, y_gap=5 if layout == "y_stride" else 0)


# ------------------------------------------------------------------------------------------------
# several matrices in one call
# ------------------------------------------------------------------------------------------------
def multi_rows(name, n_cu):
    return {"two": (3 * n_cu + 1, 7), "three": (3 * n_cu + 1, 7, 2 * n_cu - 20), "four": (n_cu + 3, 5, 2 * n_cu + 1, 33)}[name]


def run_several(G, torch, orc, types, ms, N, K, what):
    rng = np.random.default_rng(sum(ms) + N + K + sum(types))
    # the matrices of one call share x.  One activation format: blocks with factors.  Q8_0 and Q8_K weights together: a sentinel per
    # 32-block and no factors, which both quantizers take as the identity (tests/test_exact_data_cpu.py)
    one_format = len({GEMV_ACT_KIND[t] for t in types}) == 1
    for t in types:
        form_data(t, K, one_format)
    x = make_acts(types[0], N, K, rng, True) if one_format else exact_acts(N, K, rng, "q8_0", form_data(types[0], K, False)[0])
    hosts = [exact_blocks(t, m, K, rng) for t, m in zip(types, ms)]
    Ws = [DevWeights(G, torch, t, h, m, K) for t, h, m in zip(types, hosts, ms)]
    exacts = []
    for t, h, m in zip(types, hosts, ms):
        dq = orc.dequantize(t, h, K)
        assert_bound(orc, t, h, x, K, dq, f"{what}: {ids_t(t)} m={m}")
        exacts.append(exact_product_rows(orc, t, h, x, K, dq))
    keep, xptr, xstride = dev_x(torch, x, "aligned")
    first = None
    for rep in range(2):
        outs = [OutBuf(torch, N, m, m + 1) for m in ms]
        launch_multi(G, torch, [(t, W.ptr, W.stride, o.ptr, 4 * (m + 1), m) for t, W, o, m in zip(types, Ws, outs, ms)], xptr, xstride, N, K)
        gots = [o.read(f"{what} matrix {i} launch {rep}") for i, o in enumerate(outs)]
        for i, (g, e) in enumerate(zip(gots, exacts)):
            assert_bits(g, e, f"{what} matrix {i} ({ids_t(types[i])}, m={ms[i]}) launch {rep}")
        if first is None:
            first = gots
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(gots, first))
    assert all(W.unchanged() for W in Ws)
    del keep


@pytest.mark.parametrize("N", [1, 3], ids=lambda n: f"n{n}")
@pytest.mark.parametrize("name", ["two", "three", "four"], ids=str)
@pytest.mark.parametrize("t", [Q.Q4_K, Q.IQ3_S, Q.Q8_0], ids=ids_t)
def test_several_matrices_one_type(G, torch, orc, n_cu, t, name, N):
    """Row ranges concatenated in ONE launch: unequal m, one below 16 rows, and a matrix boundary inside a workgroup's row range -- a wave's
    ring crosses from one matrix into the next."""
    ms = multi_rows(name, n_cu)
    K = 2048
    rpw, grid = fast_grid(sum(ms), n_cu)
    bounds = np.cumsum(ms)[:-1]
    assert rpw >= 4 and any(b % rpw for b in bounds) and min(ms) < 16, (rpw, bounds)
    run_several(G, torch, orc, [t] * len(ms), ms, N, K, f"{ids_t(t)} x{len(ms)} n={N}")


@pytest.mark.parametrize("N", [1, 4], ids=lambda n: f"n{n}")
@pytest.mark.parametrize("name", ["interleaved_types", "mixed_families", "planar_and_canonical"], ids=str)
def test_several_matrices_mixed(G, torch, orc, n_cu, name, N):
    """[Q4_K, Q6_K, Q4_K]: one family, grouped per type (the two Q4_K matrices share a launch, out of call order); Q4_K + Q8_0: two families,
    one matrix at a time; Q4_K + Q2_K: a planar and a canonical matrix in one call.  Every output equals the exact product, hence the
    single-matrix call."""
    types = {"interleaved_types": [Q.Q4_K, Q.Q6_K, Q.Q4_K], "mixed_families": [Q.Q4_K, Q.Q8_0], "planar_and_canonical": [Q.Q4_K, Q.Q2_K]}[name]
    ms = (n_cu + 3, 150, n_cu + 38)[:len(types)]
    K = 2048
    assert [G.is_planar(t, K) for t in types] == [t != Q.Q2_K for t in types]
    run_several(G, torch, orc, types, ms, N, K, f"{name} n={N}")


# ------------------------------------------------------------------------------------------------
# MUL_MAT_ID, one column per (token, slot) pair
# ------------------------------------------------------------------------------------------------
N_EXPERT = 5


def run_moe(G, torch, orc, t, M, K, ids, x_ne1, what, ids_pad=0, plane_pad=0, expert_pad=0, x_off4=False):
    """mi355q_mul_mat_id through the C ABI with the test's own strides; ids: int32 [n_tok, n_used], ids outside [0, N_EXPERT) allowed."""
    lib = G.lib()
    n_tok, n_used = ids.shape
    pairs = n_tok * n_used
    rng = np.random.default_rng(pairs + 31 * t + K + M + x_ne1)
    as_ = exact_blocks(t, N_EXPERT * M, K, rng)
    x = make_acts(t, n_tok * x_ne1, K, rng, True)
    dq = orc.dequantize(t, as_, K)
    assert_bound(orc, t, as_, x, K, dq, what)
    x3 = x.reshape(n_tok, x_ne1, K)
    W = DevWeights(G, torch, t, as_, M, K, n_expert=N_EXPERT, expert_pad=expert_pad)
    plane = x_ne1 * K + plane_pad                             # floats between token planes
    off = 1 if x_off4 else 0
    xflat = torch.full((n_tok * plane + 8,), 3.0e30, dtype=torch.float32, device="cuda")
    xflat.as_strided((n_tok, x_ne1, K), (plane, K, 1), off).copy_(torch.from_numpy(x3).cuda())
    xptr = xflat.data_ptr() + 4 * off
    ids_w = torch.full((n_tok, n_used + ids_pad), 7777, dtype=torch.int32, device="cuda")
    ids_w[:, :n_used] = torch.from_numpy(ids).cuda()
    flat = ids.reshape(-1)
    valid = (flat >= 0) & (flat < N_EXPERT)
    ref = np.zeros((pairs, M), np.float32)
    rows = dq.reshape(N_EXPERT, M, K)
    xp = x3[np.arange(pairs) // n_used, (np.arange(pairs) % n_used) % x_ne1]
    for e in range(N_EXPERT):
        sel = np.flatnonzero(flat == e)
        if len(sel):
            ref[sel] = exact_product(orc, t, None, xp[sel], K, rows[e])
    ws = workspace(torch, int(lib.mi355q_mul_mat_id_workspace(t, M, K, n_used, n_tok, x_ne1, N_EXPERT)) + 1024)
    first = None
    for rep in range(2):
        out = OutBuf(torch, pairs, M, M)
        rc = lib.mi355q_mul_mat_id(t, W.ptr, W.stride, W.estride, N_EXPERT, xptr, x_ne1, 4 * K, 4 * plane, ids_w.data_ptr(), 4 * (n_used + ids_pad),
                                   out.ptr, M, K, n_used, n_tok, ws.data_ptr(), ws.numel(), 0, int(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.mi355q_last_error().decode(errors="replace")
        torch.cuda.synchronize()
        got = out.read(f"{what} launch {rep}")
        # (the canary is a NaN itself: the bits, not isnan, tell the kernel's NaN fill from a row that was never written)
        assert (got[~valid].view(np.uint32) == NAN_FILL).all(), f"{what}: the row of an out-of-range id is not the kernels' NaN (0x7FC00000) throughout"
        assert_bits(got[valid], ref[valid], f"{what} launch {rep} (valid pairs)")
        if first is None:
            first = got
        assert np.array_equal(got.view(np.uint32), first.view(np.uint32)), f"{what}: a second launch differs"
    assert W.unchanged(), f"{what}: the weight buffer was written"


def moe_ids(n_tok, n_used, seed):
    return np.random.default_rng(seed).integers(0, N_EXPERT, (n_tok, n_used)).astype(np.int32)


# name -> (n_tok, n_used, x_ne1, keyword arguments, ids override)
MOE_CASES = {
    "pairs1":          (1, 1, 1, {}, None),
    "pairs2_bcast":    (1, 2, 1, {}, None),
    "pairs16_bcast":   (4, 4, 1, {}, None),
    "pairs16_per_slot": (4, 4, 4, {}, None),
    "ids_stride":      (3, 2, 2, {"ids_pad": 3}, None),
    "token_stride":    (3, 2, 2, {"plane_pad": 8}, None),
    "token_stride_off_16": (3, 2, 2, {"plane_pad": 1}, None),     # planes 4 bytes off 16 apart: the float4 fetch of a later token would be misaligned
    "same_expert_twice": (2, 2, 1, {}, [[3, 3], [1, 1]]),
    "bad_ids":         (3, 2, 1, {}, [[0, -1], [N_EXPERT, 2], [4, 1]]),
    "expert_stride":   (3, 2, 1, {"expert_pad": 64}, [[4, 0], [1, 3], [2, 4]]),
}


@pytest.mark.parametrize("name", list(MOE_CASES), ids=str)
@pytest.mark.parametrize("t", [Q.Q4_K, Q.Q8_0, Q.IQ3_S, Q.IQ3_XXS], ids=ids_t)
def test_moe_streamed(G, torch, orc, n_cu, t, name):
    """Up to 16 pairs: k_gemv_fast with blockIdx.y = pair, grid.x = n_cu / pairs, the expert id read on the device."""
    n_tok, n_used, x_ne1, kw, ids = MOE_CASES[name]
    K, M = 2048, 2 * n_cu + 21
    ids = moe_ids(n_tok, n_used, 17 + len(name)) if ids is None else np.array(ids, np.int32)
    pairs = n_tok * n_used
    assert G.is_planar(t, K) and pairs <= 16 and ids.shape == (n_tok, n_used)
    rpw, grid = fast_grid(M, n_cu, pairs)
    assert grid == cdiv(M, rpw) and (pairs == 1 or rpw > 2), (rpw, grid)
    run_moe(G, torch, orc, t, M, K, ids, x_ne1, f"{ids_t(t)} {name}", **kw)


@pytest.mark.parametrize("name", ["pairs17", "few_workgroups", "more_pairs_than_cus"], ids=str)
@pytest.mark.parametrize("t", [Q.IQ3_S, Q.IQ3_XXS], ids=ids_t)
def test_moe_streamed_iq3_every_pair_count(G, torch, orc, n_cu, t, name):
    """Planar IQ3 rows are never grouped: the streamed form at 17 pairs, at a pair count that leaves 2 or 3 workgroups per pair, and at one
    above the CU count (n_cu / pairs = 0: one workgroup walks all rows of its pair).  Two ids out of range among them."""
    K, M = 2048, 70
    pairs = {"pairs17": 17, "few_workgroups": n_cu // 3 + 1, "more_pairs_than_cus": n_cu + 1}[name]
    rpw, grid = fast_grid(M, n_cu, pairs)
    want = {"pairs17": n_cu // pairs > 3, "few_workgroups": n_cu // pairs in (2, 3) and grid == n_cu // pairs, "more_pairs_than_cus": n_cu // pairs == 0 and grid == 1 and rpw == M}[name]
    assert want and G.is_planar(t, K), f"{name}: {pairs} pairs on {n_cu} CUs give {grid} workgroups of {rpw} rows"
    ids = moe_ids(pairs, 1, pairs)
    ids[3, 0], ids[pairs - 1, 0] = -2, N_EXPERT + 1
    run_moe(G, torch, orc, t, M, K, ids, 1, f"{ids_t(t)} {name}")


# ------------------------------------------------------------------------------------------------
# canonical rows: k_gemv_generic
# ------------------------------------------------------------------------------------------------
def batched_canonical(t, K):
    """csrc/mmq_generic.hip mmq_generic_supported: canonical rows that N > 8 would send to the matrix cores."""
    return t in GEMV_CANONICAL_BATCH_TYPES and K % (128 if GEMV_ACT_KIND[t] == "q8_0" else 256) == 0


@pytest.mark.parametrize("scaled", [False, True], ids=["identity", "factors"])
@pytest.mark.parametrize("N", [1, 3, 8], ids=lambda n: f"n{n}")
@pytest.mark.parametrize("t", GENERIC_TYPES, ids=ids_t)
def test_generic_types(G, torch, orc, t, N, scaled):
    """Every type at a K where its rows are canonical; M = 37 is no multiple of the 4 rows of a workgroup."""
    K = gemv_canonical_ks(t)[0]
    M = 37
    assert not G.is_planar(t, K) and M % 4
    w, x, exact = exact_case(orc, t, M, N, K, scaled, 11000 + 10 * t + N)
    run_single(G, torch, DevWeights(G, torch, t, w, M, K), t, M, N, K, x, exact, f"{ids_t(t)} canonical n={N} K={K}", flags=(0, ROUND_EVEN) if GEMV_ACT_KIND[t] == "q8_0" else (0,), y_gap=1 if N == 3 else 0)


@pytest.mark.parametrize("t", GENERIC_TYPES, ids=ids_t)
def test_generic_ragged_second_trip(G, torch, orc, t):
    """65 .. 127 sub-blocks of 32: lanes below nsub - 64 make a second trip of the sub-block loop, the others do not."""
    K = gemv_canonical_ks(t)[1]
    M, N = 21, 3
    assert not G.is_planar(t, K) and 65 <= K // 32 <= 127
    w, x, exact = exact_case(orc, t, M, N, K, True, 12000 + t)
    run_single(G, torch, DevWeights(G, torch, t, w, M, K), t, M, N, K, x, exact, f"{ids_t(t)} canonical K={K}")


def test_generic_row_loop_above_32768_rows(G, torch, orc):
    """grid.x is capped at 8192 workgroups of 4 rows: above 32768 rows a wave walks the grid-stride loop a second time."""
    t, K, M, N = Q.Q5_0, 64, 32768 + 5, 2
    assert not G.is_planar(t, K) and cdiv(M, 4) > 8192 and M % 4
    w, x, exact = exact_case(orc, t, M, N, K, True, 13000)
    run_single(G, torch, DevWeights(G, torch, t, w, M, K), t, M, N, K, x, exact, "q5_0 canonical 32773 rows")


@pytest.mark.parametrize("t", [Q.Q2_K, Q.Q4_1], ids=ids_t)
def test_generic_force_gemv_n9(G, torch, orc, t):
    """N = 9 would run on the batched canonical tier; MI355Q_FLAG_FORCE_GEMV keeps one k_gemv_generic column per token."""
    K = gemv_canonical_ks(t)[0]
    M, N = 37, 9
    assert not G.is_planar(t, K) and batched_canonical(t, K)
    w, x, exact = exact_case(orc, t, M, N, K, True, 14000 + t)
    run_single(G, torch, DevWeights(G, torch, t, w, M, K), t, M, N, K, x, exact, f"{ids_t(t)} canonical FORCE_GEMV n=9", flags=(FORCE_GEMV,), y_gap=2)


# name -> (n_tok, n_used, x_ne1, keyword arguments, ids override)
GENERIC_MOE_CASES = {
    "pairs1":          (1, 1, 1, {}, None),
    "pairs16_per_slot": (4, 4, 4, {"ids_pad": 2}, None),
    "pairs18_x_off_16": (9, 2, 1, {"x_off4": True}, None),        # grouping needs 16-byte aligned activations: refused, one column per pair
    "token_stride":    (3, 2, 2, {"plane_pad": 5}, None),
    "bad_ids":         (3, 2, 1, {"expert_pad": 32}, [[0, -1], [N_EXPERT, 2], [4, 4]]),
}


@pytest.mark.parametrize("name", list(GENERIC_MOE_CASES), ids=str)
@pytest.mark.parametrize("t", [Q.Q4_1, Q.Q5_0, Q.Q3_K, Q.IQ2_XS, Q.IQ1_M, Q.Q6_K], ids=ids_t)
def test_generic_moe(G, torch, orc, t, name):
    """MUL_MAT_ID on canonical rows: activations quantized plane by plane into the workspace, one wave per (pair, row)."""
    n_tok, n_used, x_ne1, kw, ids = GENERIC_MOE_CASES[name]
    K, M = gemv_canonical_ks(t)[0], 23
    ids = moe_ids(n_tok, n_used, 23 + len(name)) if ids is None else np.array(ids, np.int32)
    pairs = n_tok * n_used
    assert not G.is_planar(t, K) and (pairs <= 16 or kw.get("x_off4"))
    run_moe(G, torch, orc, t, M, K, ids, x_ne1, f"{ids_t(t)} canonical {name}", **kw)
