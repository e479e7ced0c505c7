"""Every dispatch branch of the residency ops and of FLASH_ATTN_EXT (csrc/ops_glue.hip) on the device.

Most mi355q_op_* entry points pick one of two or three kernels by row length, alignment, batch size or window; tests/test_gpu_glue.py
runs about one shape per op.  Here the shapes are chosen to select each branch -- the branch a case is meant to take is part of its
test id -- and both sides of every threshold are run.  References: oracle/glue.py (the CPU's arithmetic, pinned against the reference
in tests/test_oracle_glue.py) where it covers the op, a float64 restatement otherwise and for FLASH_ATTN_EXT always.  Bounds are bit
equality where the kernel claims it, otherwise relative to the magnitude of what is compared (per element, or sum |a| |b| per output
for the dot products); each constant is about 4x the largest error measured on an MI355X, which is noted beside it."""
import zlib

import numpy as np
import pytest

import oracle
from oracle import glue

pytestmark = pytest.mark.gpu

f32 = np.float32
TINY = float(np.finfo(f32).smallest_subnormal)           # one unit of the subnormal range: the floor of a relative bound, never 1


@pytest.fixture(scope="module")
def G():
    import torch
    import ggml_mi355 as g
    assert torch.cuda.is_available() and g.lib().mi355q_device_count() >= 1
    return g


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def measured(name, value):
    """The error a case measured (pytest -s shows it): the evidence behind the bounds below."""
    print(f"MEASURED {name} {value:.3e}")


def rel_err(y, ref, scale=None):
    """max |y - ref| / scale over the elements (scale = |ref| by default); NaN / Inf positions must agree exactly."""
    y = np.asarray(y, np.float64); ref = np.asarray(ref, np.float64)
    scale = np.abs(ref) if scale is None else np.broadcast_to(np.asarray(scale, np.float64), ref.shape)
    assert np.array_equal(np.isnan(y), np.isnan(ref)), "NaN positions differ"
    inf = np.isinf(ref)
    assert np.array_equal(y[inf], ref[inf]), "infinities differ"
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    return float((np.abs(y[fin] - ref[fin]) / (scale[fin] + TINY)).max())


# ================================================================================================ SOFT_MAX
# k_soft_max_reg<8> for ne0 <= 512, k_soft_max_reg<32> up to 2048, k_soft_max (three passes through memory) beyond.  Against glue.soft_max
# per element, relative: the device expf and numpy's differ by an ulp now and then.
SM_REL = 4e-6            # measured on an MI355X: 9.0e-7 at most (ALiBi over 40 heads: device powf / expf against numpy's)
SOFTMAX_NE0 = [(1, "reg8"), (7, "reg8"), (64, "reg8"), (65, "reg8"), (512, "reg8"), (513, "reg32"), (2048, "reg32"), (2049, "wide"),
               (4113, "wide"), (32768, "wide")]


def softmax_case(rng, shape, mask_rows, f16_mask):
    x = (rng.standard_normal(shape) * 3).astype(f32)
    ne0 = shape[-1]
    m = rng.standard_normal((mask_rows, ne0)).astype(f32)
    m[rng.random((mask_rows, ne0)) < 0.2] = -np.inf
    m[:, 0] = 0.0
    if f16_mask:
        m = m.astype(np.float16).astype(f32)                   # f16 values: the f32 reference stands for the f16 mask the graph uses
    return x, m


def check_soft_max(G, torch, x, m, scale, max_bias, f16_mask, name):
    md = None if m is None else (dev(torch, m.astype(np.float16)) if f16_mask else dev(torch, m))
    y = G.op_soft_max(dev(torch, x), md, scale, max_bias).cpu().numpy()
    ref = glue.soft_max(x, m, scale, max_bias)
    assert np.array_equal(y == 0, ref == 0), name               # masked entries are exactly 0, and only they
    e = rel_err(y, ref)
    measured(name, e)
    assert e <= SM_REL, (name, e)
    return y


@pytest.mark.parametrize("ne0,branch", SOFTMAX_NE0, ids=[f"{b}-ne0_{n}" for n, b in SOFTMAX_NE0])
def test_soft_max_branches(G, torch, ne0, branch):
    """[ne3 = 2, 3 heads, 5 rows]: 30 rows (not a multiple of the 4 rows of a workgroup); the mask has 8 rows (more than ne1); with 3 heads
    ALiBi takes the m1 slope for head 2."""
    rng = np.random.default_rng(100 + ne0)
    for f16_mask in (False, True):
        x, m = softmax_case(rng, (2, 3, 5, ne0), 8, f16_mask)
        for mb in (0.0, 8.0):
            check_soft_max(G, torch, x, m, 0.125, mb, f16_mask, f"softmax-{branch}-ne0_{ne0}-{'f16' if f16_mask else 'f32'}-mb{mb:g}")
    check_soft_max(G, torch, x, None, 0.125, 0.0, False, f"softmax-{branch}-ne0_{ne0}-nomask")


@pytest.mark.parametrize("heads", [12, 40])
@pytest.mark.parametrize("ne0,branch", [(300, "reg8"), (1500, "reg32"), (4113, "wide")], ids=["reg8", "reg32", "wide"])
def test_soft_max_alibi_heads_not_a_power_of_two(G, torch, heads, ne0, branch):
    """ALiBi slopes for a head count that is not a power of two: heads >= n_head_log2 take m1^(2 (h - n_head_log2) + 1)."""
    rng = np.random.default_rng(heads * 10 + ne0)
    for f16_mask in (False, True):
        x, m = softmax_case(rng, (1, heads, 3, ne0), 3, f16_mask)
        check_soft_max(G, torch, x, m, 0.0884, 8.0, f16_mask, f"softmax-alibi{heads}-{branch}-{'f16' if f16_mask else 'f32'}")


@pytest.mark.parametrize("ne0,branch", [(300, "reg8"), (1500, "reg32"), (4113, "wide")], ids=["reg8", "reg32", "wide"])
def test_soft_max_in_place(G, torch, ne0, branch):
    """out = a (how the flash-attention prefill path calls it on its scores): the same bits as out of place."""
    rng = np.random.default_rng(7 + ne0)
    x, m = softmax_case(rng, (2, 3, 5, ne0), 5, True)
    md = dev(torch, m.astype(np.float16))
    want = G.op_soft_max(dev(torch, x), md, 0.125, 8.0).cpu().numpy()
    t = dev(torch, x)
    G.op_soft_max(t, md, 0.125, 8.0, out=t)
    assert np.array_equal(bits(t.cpu().numpy()), bits(want))


# ================================================================================================ RMS_NORM and the fused forms
# k_add_rms_norm_mul_vec<4> (ne0 <= 4096), _vec<16> (<= 16384), both for ne0 % 4 == 0 and 16-byte aligned operands; k_add_rms_norm_mul otherwise.
# measured on an MI355X: every case bit-identical to the oracle, on all three kernels (only the order of the f64 sum of squares differs, and
# it moved no rounding of the mean for these seeded rows), so the check is bit equality
RMS_NE0 = [(30, "scalar"), (4096, "vec4"), (4097, "scalar"), (4100, "vec16"), (16384, "vec16"), (16388, "scalar"), (20480, "scalar")]


@pytest.mark.parametrize("ne0,branch", RMS_NE0, ids=[f"{b}-ne0_{n}" for n, b in RMS_NE0])
def test_rms_norm_branches(G, torch, ne0, branch):
    rng = np.random.default_rng(200 + ne0)
    x = (rng.standard_normal((2, 3, ne0)) * rng.uniform(0.01, 30.0, (2, 3, 1))).astype(f32)
    y = G.op_rms_norm(dev(torch, x), 1e-5).cpu().numpy()
    ref = glue.rms_norm(x, 1e-5)
    assert np.array_equal(bits(y), bits(ref)), rel_err(y, ref)


def test_rms_norm_unaligned_view_takes_the_scalar_kernel(G, torch):
    """A 4096-wide row read through a view that starts one float in (and rows 4097 floats apart): not 16-byte aligned -> k_add_rms_norm_mul."""
    rng = np.random.default_rng(21)
    big = (rng.standard_normal((5, 4097)) * 4).astype(f32)
    view = dev(torch, big)[:, 1:]
    y = G.op_rms_norm(view, 1e-5).cpu().numpy()
    ref = glue.rms_norm(big[:, 1:], 1e-5)
    assert np.array_equal(bits(y), bits(ref)), rel_err(y, ref)
    w = dev(torch, rng.uniform(0.5, 1.5, 4096).astype(f32))
    assert G.op_add_rms_norm_mul(view, 1e-5, weight=w).equal(G.op_bin_bcast(G.OP_MUL, G.op_rms_norm(view, 1e-5), w))


@pytest.mark.parametrize("ne0,branch", [(4096, "vec4"), (14336, "vec16"), (4097, "scalar"), (20480, "scalar")], ids=["vec4", "vec16", "scalar-ragged", "scalar-long"])
def test_fused_add_rms_norm_mul_each_kernel(G, torch, ne0, branch):
    """The fused [add ->] rms_norm [-> * weight] through each of the three kernels: bit-identical to the separate ops, also with dst aliasing
    a or b (the kernel's contract: row r of dst is row r of the operand, owned by one workgroup)."""
    rng = np.random.default_rng(300 + ne0)
    a = dev(torch, (rng.standard_normal((3, ne0)) * 3).astype(f32))
    b = dev(torch, rng.standard_normal((3, ne0)).astype(f32))
    w = dev(torch, rng.uniform(0.5, 1.5, (ne0,)).astype(f32))
    eps = 1e-5
    assert G.op_add_rms_norm_mul(a, eps).equal(G.op_rms_norm(a, eps))
    assert G.op_add_rms_norm_mul(a, eps, weight=w).equal(G.op_bin_bcast(G.OP_MUL, G.op_rms_norm(a, eps), w))
    s_sep = G.op_bin_bcast(G.OP_ADD, a, b)
    y_sep = G.op_bin_bcast(G.OP_MUL, G.op_rms_norm(s_sep, eps), w)
    y, s = G.op_add_rms_norm_mul(a, eps, b=b, weight=w, want_sum=True)
    assert s.equal(s_sep) and y.equal(y_sep)
    assert G.op_add_rms_norm_mul(a, eps, b=b, weight=w).equal(y_sep)
    # dst aliasing a (with and without the stored sum) and aliasing b
    a2 = a.clone()
    G.op_add_rms_norm_mul(a2, eps, b=b, weight=w, out=a2)
    assert a2.equal(y_sep)
    a3 = a.clone()
    _, s3 = G.op_add_rms_norm_mul(a3, eps, b=b, weight=w, want_sum=True, out=a3)
    assert a3.equal(y_sep) and s3.equal(s_sep)
    b2 = b.clone()
    G.op_add_rms_norm_mul(a, eps, b=b2, weight=w, out=b2)
    assert b2.equal(y_sep)
    a4 = a.clone()
    G.op_add_rms_norm_mul(a4, eps, out=a4)
    assert a4.equal(G.op_rms_norm(a, eps))


# ================================================================================================ UNARY, unary_mul, SCALE
UN_REL = 1.2e-6          # measured on an MI355X: 2.8e-7 at most (SILU / SIGMOID / TANH through the device expf / tanhf)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 88.5, -88.5, 89.0, -89.0, 104.0, -104.0, 1e3, -1e3, 1e-40, -1e-40, 1e-45, -1e-45,
                    1.1754944e-38, -1.1754944e-38, 15.0, -15.0, 9.5, -9.5, 1e-4, -1e-4, 0.5, -0.5], f32)


def unary_input(rng):
    x = (rng.standard_normal(4 * 1031) * 6).astype(f32)
    x[:SPECIAL.size] = SPECIAL
    x[SPECIAL.size:2 * SPECIAL.size] = SPECIAL * f32(0.37)
    return x.reshape(4, 1031)


def unary_ref(op, x):
    """the CPU's f32 steps (ggml-cpu/vec.h, unary-ops.cpp) with each libm call correctly rounded from float64"""
    x = np.asarray(x, f32)
    x64 = x.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if op == "silu":
            return glue.silu(x)
        if op == "sigmoid":
            return (f32(1.0) / (f32(1.0) + np.exp(-x64).astype(f32))).astype(f32)
        if op == "tanh":
            return np.tanh(x64).astype(f32)
        if op == "relu":
            return np.where(x > 0, x, f32(0.0)).astype(f32)
        if op == "neg":
            return -x
        return np.abs(x)


UNARY_OPS = ["silu", "relu", "sigmoid", "tanh", "neg", "abs"]
EXACT_UNARY = {"relu", "neg", "abs"}


@pytest.mark.parametrize("op", UNARY_OPS)
def test_unary_all_ops_special_values(G, torch, op):
    """All six unary ops over +-0, +-inf, NaN, |x| > 88 (expf overflows), subnormals and ordinary values; RELU / NEG / ABS bit for bit (NaN
    payload and sign included), the others per element; a permuted source gives the bits of its contiguous copy."""
    code = getattr(G, "UNARY_" + op.upper())
    x = unary_input(np.random.default_rng(400 + code))
    y = G.op_unary(code, dev(torch, x)).cpu().numpy()
    ref = unary_ref(op, x)
    if op in EXACT_UNARY:
        assert np.array_equal(bits(y), bits(ref)), op
    else:
        e = rel_err(y, ref)
        measured(f"unary-{op}", e)
        assert e <= UN_REL, (op, e)
    xt = dev(torch, x).t()                                                  # permuted source [1031, 4] with strides (1, 1031)
    yt = G.op_unary(code, xt).cpu().numpy()
    assert np.array_equal(bits(yt), bits(G.op_unary(code, xt.contiguous()).cpu().numpy()))


@pytest.mark.parametrize("op", ["silu", "relu", "sigmoid"])
def test_unary_mul_all_ops(G, torch, op):
    """op(a) * b fused (k_unary_mul): bit-identical to the separate UNARY and MUL, special values in both operands."""
    code = getattr(G, "UNARY_" + op.upper())
    rng = np.random.default_rng(500 + code)
    a = unary_input(rng)
    b = rng.standard_normal(a.shape).astype(f32)
    b[0, :SPECIAL.size] = SPECIAL[::-1]
    ad, bd = dev(torch, a), dev(torch, b)
    y = G.op_unary_mul(code, ad, bd)
    assert np.array_equal(bits(y.cpu().numpy()), bits(G.op_bin_bcast(G.OP_MUL, G.op_unary(code, ad), bd).cpu().numpy())), op
    with np.errstate(invalid="ignore", over="ignore"):
        ref = (unary_ref(op, a) * b).astype(f32)
    if op == "relu":
        assert np.array_equal(bits(y.cpu().numpy()), bits(ref))
    else:
        e = rel_err(y.cpu().numpy(), ref)
        measured(f"unary_mul-{op}", e)
        assert e <= UN_REL, (op, e)


def same_bits_but_nan(y, want):
    """bit equality, except that a NaN made by an invalid product (inf * 0) need only be a NaN: the host's default NaN has the other sign"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(y), nan) and np.array_equal(bits(y)[~nan], bits(want)[~nan])


def test_scale_bitexact(G, torch):
    """k_scale: dst = a * s in f32, special values, a permuted source and a 3-D strided view."""
    x = unary_input(np.random.default_rng(600))
    for s in (0.125, -3.3, 1e30, 0.0):
        with np.errstate(invalid="ignore", over="ignore"):
            want = (x * f32(s)).astype(f32)
        y = G.op_scale(dev(torch, x), s).cpu().numpy()
        assert same_bits_but_nan(y, want), s
        yt = G.op_scale(dev(torch, x).t(), s).cpu().numpy()
        assert same_bits_but_nan(yt, np.ascontiguousarray(want.T)), s
    big = dev(torch, np.tile(x, (1, 2)).reshape(2, 4, 1031))
    yv = G.op_scale(big[:, 1:3, 5:900], 0.5).cpu().numpy()
    assert np.array_equal(bits(yv), bits((big[:, 1:3, 5:900].cpu().numpy() * f32(0.5)).astype(f32)))


# ================================================================================================ GET_ROWS
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_get_rows_tables(G, torch, dtype):
    """f32 / f16 tables, 3-D ids (dst [ne00, ne10, ne11, ne12]), repeated ids, a strided ids view; out-of-range ids leave their destination row
    untouched (the documented behaviour: the reference asserts)."""
    rng = np.random.default_rng(700 if dtype == "f32" else 701)
    npt = f32 if dtype == "f32" else np.float16
    table = rng.standard_normal((2, 3, 50, 96)).astype(npt)                  # [ne03, ne02, rows, ne00]
    ids = rng.integers(0, 50, (2, 3, 7)).astype(np.int32)                    # [ne12, ne11, ne10]
    ids[0, 0, :3] = 7                                                        # repeated
    y = G.op_get_rows(dev(torch, table), dev(torch, ids)).cpu().numpy()
    want = np.stack([np.stack([table[i12, i11][ids[i12, i11]] for i11 in range(3)]) for i12 in range(2)]).astype(f32)
    assert y.shape == (2, 3, 7, 96) and np.array_equal(bits(y), bits(want))
    # strided ids: every other entry of a wider tensor
    wide = rng.integers(0, 50, (2, 3, 14)).astype(np.int32)
    y = G.op_get_rows(dev(torch, table), dev(torch, wide)[..., ::2]).cpu().numpy()
    ws = wide[..., ::2]
    want = np.stack([np.stack([table[i12, i11][ws[i12, i11]] for i11 in range(3)]) for i12 in range(2)]).astype(f32)
    assert np.array_equal(bits(y), bits(want))
    # 2-D table, 1-D ids with out-of-range entries
    t2 = rng.standard_normal((50, 96)).astype(npt)
    ids1 = np.array([3, -1, 49, 50, 0, 1000, 3], np.int32)
    out = torch.full((7, 96), 7.5, dtype=torch.float32, device="cuda")
    G.op_get_rows(dev(torch, t2), dev(torch, ids1), out=out)
    got = out.cpu().numpy()
    for r, i in enumerate(ids1):
        assert np.array_equal(bits(got[r]), bits(t2[i].astype(f32) if 0 <= i < 50 else np.full(96, 7.5, f32))), (r, i)


# ================================================================================================ ARGSORT
def argsort_row_values(rng, shape):
    x = (rng.integers(-40, 40, shape) / 4.0).astype(f32)                      # many ties
    x[..., 0] = -0.0; x[..., 1] = 0.0; x[..., 2] = -0.0; x[..., 3] = -np.inf; x[..., 5] = -np.inf
    x[..., 7] = rng.standard_normal(shape[:-1]).astype(f32)
    return x


def check_argsort(G, torch, x):
    for desc in (False, True):
        got = G.op_argsort(dev(torch, x), descending=desc).cpu().numpy()
        want = np.argsort(-x if desc else x, axis=-1, kind="stable").astype(np.int32)
        assert np.array_equal(got, want), (x.shape, desc)


def test_argsort_long_rows(G, torch):
    """Rows over 12288 entries need the 128 KiB dynamic-LDS attribute, up to the 32768 limit: run before and after a small row in one process;
    ties (index order), -0 / +0 (equal) and -inf; 32769 entries are declined."""
    rng = np.random.default_rng(800)
    check_argsort(G, torch, argsort_row_values(rng, (3, 1000)))
    check_argsort(G, torch, argsort_row_values(rng, (2, 12289)))
    check_argsort(G, torch, argsort_row_values(rng, (2, 2, 60)))
    check_argsort(G, torch, argsort_row_values(rng, (2, 32768)))
    check_argsort(G, torch, argsort_row_values(rng, (5, 12288)))
    with pytest.raises(G.Mi355qError):
        G.op_argsort(torch.zeros((1, 32769), dtype=torch.float32, device="cuda"))


# ================================================================================================ MUL_MAT f16 / f32 src0
# k_mul_mat_f (a wave per 8 src0 rows; f32 accumulation, lane-strided) for few src1 rows, an f32 src0, or operands that are not 16-byte aligned;
# k_mul_mat_f16_mfma for >= 16 src1 rows and >= 16 src0 rows, K % 16 == 0, aligned.  |y - ref| <= c * sum_k |a| |b| per output.
MM_ROW = 3e-7            # measured on an MI355X: 7.3e-8 at most
MM_MFMA = 3e-7           # measured on an MI355X: 7.9e-8


def mm_ref(a, b, f16):
    """float64 product of the operands as the CPU takes them (an f16 src0 makes it round src1 to f16), and sum |a| |b| per output."""
    a = np.asarray(a, np.float64); b = np.asarray(b, f32)
    if f16:
        b = b.astype(np.float16)
    b = b.astype(np.float64)
    r3, r2 = b.shape[0] // a.shape[0], b.shape[1] // a.shape[1]
    out = np.zeros(b.shape[:3] + (a.shape[2],)); mag = np.zeros_like(out)
    for i3 in range(b.shape[0]):
        for i2 in range(b.shape[1]):
            aa = a[i3 // r3, i2 // r2]
            out[i3, i2] = b[i3, i2] @ aa.T
            mag[i3, i2] = np.abs(b[i3, i2]) @ np.abs(aa).T
    return out, mag


MM_CASES = [(M, K) for M in (1, 7, 9, 65) for K in (48, 80, 100, 4100)]


@pytest.mark.parametrize("M,K", MM_CASES, ids=[f"rowwave-M{M}-K{K}" for M, K in MM_CASES])
def test_mul_mat_f_rows(G, torch, M, K):
    """k_mul_mat_f: M not a multiple of the 8 rows of a wave, K not a multiple of 64, src0 broadcast over dims 2 (x2) and 3 (x3); f16 and f32 src0."""
    rng = np.random.default_rng(900 + M * 7 + K)
    a = rng.standard_normal((1, 2, M, K)).astype(f32)
    b = rng.standard_normal((3, 4, 5, K)).astype(f32)
    for f16 in (True, False):
        av = a.astype(np.float16) if f16 else a
        y = G.op_mul_mat_f(dev(torch, av), dev(torch, b)).cpu().numpy()
        ref, mag = mm_ref(av, b, f16)
        e = rel_err(y, ref, mag)
        measured(f"mm-rowwave-M{M}-K{K}-{'f16' if f16 else 'f32'}", e)
        assert y.shape == (3, 4, 5, M) and e <= MM_ROW, e


def test_mul_mat_f32_src0_many_rows(G, torch):
    """an f32 src0 with >= 16 src1 rows stays on k_mul_mat_f (the matrix-core kernel is f16 / bf16 only)"""
    rng = np.random.default_rng(950)
    a = rng.standard_normal((1, 2, 65, 100)).astype(f32)
    b = rng.standard_normal((1, 4, 20, 100)).astype(f32)
    y = G.op_mul_mat_f(dev(torch, a), dev(torch, b)).cpu().numpy()
    ref, mag = mm_ref(a, b, False)
    e = rel_err(y, ref, mag)
    measured("mm-rowwave-f32-N20", e)
    assert e <= MM_ROW, e


def test_mul_mat_f16_mfma_ragged_and_unaligned_fallback(G, torch):
    """k_mul_mat_f16_mfma with M = 65 and N = 37 (ragged against the 64 x 64 tile), K = 80 (not a multiple of the 64-step), broadcast over dims 2
    and 3; then the same operands through a view 2 bytes in (alignment fallback to k_mul_mat_f): both against the reference."""
    rng = np.random.default_rng(960)
    M, N, K = 65, 37, 80
    a = rng.standard_normal((1, 2, M, K)).astype(np.float16)
    b = rng.standard_normal((3, 4, N, K)).astype(f32)
    ref, mag = mm_ref(a, b, True)
    y = G.op_mul_mat_f(dev(torch, a), dev(torch, b)).cpu().numpy()
    e = rel_err(y, ref, mag)
    measured("mm-mfma-M65-N37-K80", e)
    assert e <= MM_MFMA, e
    padded = np.zeros((1, 2, M, K + 1), np.float16)
    padded[..., 1:] = a
    av = dev(torch, padded)[..., 1:]                                        # data 2 bytes off, row pitch 162 bytes
    y2 = G.op_mul_mat_f(av, dev(torch, b)).cpu().numpy()
    e2 = rel_err(y2, ref, mag)
    measured("mm-rowwave-unaligned-M65-N37-K80", e2)
    assert e2 <= MM_ROW, e2


# ================================================================================================ FLASH_ATTN_EXT, f16 cache
# Paths (mi355q_op_flash_attn_ext): `seq` (n_kv <= 1024, DK % 32 == 0, the CPU's F16 accumulator and bits), the f32 form split in 2..8 pieces merged
# by k_flash_attn_combine (N*H*B <= 256, n_kv >= 256, with a workspace), the f32 form in one piece (N*H*B > 256, or no workspace; the whole window's
# scores in LDS: 147 KB at 36864), and the matrix-core prefill (N >= 16, n_kv % 16 == 0: K q, k_soft_max_*, P V).  Against a float64 restatement:
# |y - ref| <= c * sum_j p_j |v_j| per output (the size of what is summed: the loss of one position of a 36864 window is 3e-5 of it).
# measured on an MI355X: seq 2.0e-3 (the CPU's F16 accumulator; those cases are also the oracle's bits), f32 1.0e-7, mfma 1.3e-4 (P rounded to f16)
FA_BOUND = {"seq": 8e-3, "f32": 4e-7, "mfma": 5e-4}

# (branch, DK, DV, H, Hk, N, B, Bk, n_kv, max_bias, split)
FA_CASES = [
    ("seq-kv1024", 128, 128, 8, 2, 1, 1, 1, 1024, 0.0, True),
    ("split8-kv1025", 128, 128, 8, 2, 1, 1, 1, 1025, 0.0, True),
    ("split3-d80-kv300", 80, 80, 8, 2, 1, 1, 1, 300, 0.0, True),
    ("split6-d80-kv700", 80, 80, 8, 2, 1, 1, 1, 700, 0.0, True),
    ("split3-d112-kv300", 112, 112, 4, 4, 2, 1, 1, 300, 0.0, True),
    ("split6-d112-kv700", 112, 112, 4, 1, 1, 1, 1, 700, 0.0, True),
    ("split8-kv8192", 128, 128, 8, 8, 1, 1, 1, 8192, 0.0, True),
    ("split8-kv36864", 128, 128, 4, 1, 1, 1, 1, 36864, 0.0, True),
    ("single-nh288-kv36864", 128, 128, 32, 8, 9, 1, 1, 36864, 0.0, True),
    ("single-nosplit-d80-kv700", 80, 80, 8, 2, 1, 1, 1, 700, 0.0, False),
    ("split8-n15-kv2048", 128, 128, 4, 2, 15, 1, 1, 2048, 0.0, True),
    ("seq-prefill-n40-kv1000", 128, 128, 2, 1, 40, 1, 1, 1000, 0.0, True),
    ("mfma-n16-kv2048", 128, 128, 4, 2, 16, 1, 1, 2048, 0.0, True),
    ("mfma-widesoftmax-n64-kv4112", 128, 128, 4, 2, 64, 1, 1, 4112, 0.0, True),
    ("seq-alibi12-b2-bk1-kv700", 128, 128, 12, 4, 1, 2, 1, 700, 8.0, True),
    ("split8-alibi12-b2-bk1-kv2048", 128, 128, 12, 4, 1, 2, 1, 2048, 8.0, True),
    ("mfma-alibi12-b2-bk1-kv512", 128, 128, 12, 4, 32, 2, 1, 512, 8.0, True),
]


def fa_path(DK, N, H, B, n_kv, split):
    if N >= 16 and split and n_kv % 16 == 0:
        return "mfma"
    if n_kv <= 1024 and DK % 32 == 0:
        return "seq"
    return "f32"


def alibi_slopes(H, max_bias):
    n2 = 1
    while 2 * n2 <= H:
        n2 *= 2
    m0, m1 = 2.0 ** (-max_bias / n2), 2.0 ** (-(max_bias / 2.0) / n2)
    return [(m0 ** (h + 1) if h < n2 else m1 ** (2 * (h - n2) + 1)) if max_bias > 0 else 1.0 for h in range(H)]


def fa_ref(q, k, v, mask, scale, max_bias, qround):
    """float64 FLASH_ATTN_EXT (ggml-cpu/ops.cpp:6690-6905) with q rounded as the CPU does (`qround`); -> ref and sum_j p_j |v_j|, [B, N, H, DV]"""
    B, H, N, _ = q.shape
    Bk, Hk, Bv, Hv, DV = k.shape[0], k.shape[1], v.shape[0], v.shape[1], v.shape[3]
    qh = qround(q).astype(np.float64)
    out = np.zeros((B, N, H, DV)); mag = np.zeros_like(out)
    slopes = alibi_slopes(H, max_bias)
    for b in range(B):
        for h in range(H):
            kk = k[b // (B // Bk), h // (H // Hk)].astype(np.float64); vv = v[b // (B // Bv), h // (H // Hv)].astype(np.float64)
            s = (qh[b, h] @ kk.T) * scale
            if mask is not None:
                with np.errstate(invalid="ignore"):
                    s = s + slopes[h] * mask[:N, :kk.shape[0]].astype(np.float64)
            s = s - s.max(axis=1, keepdims=True)
            p = np.exp(s)
            p /= p.sum(axis=1, keepdims=True)
            out[b, :, h] = p @ vv
            mag[b, :, h] = p @ np.abs(vv)
    return out, mag


def fa_mask(rng, N, n_kv, max_bias, rows=None):
    mask = np.zeros((rows or N, n_kv), np.float16)
    for t in range(N):
        mask[t, n_kv - N + t + 1:] = -np.inf                                 # causal
    mask[:, rng.choice(n_kv - N, max(1, n_kv // 20), replace=False)] = -np.inf       # holes
    if max_bias > 0:
        mask[:N] += (rng.standard_normal((N, n_kv)) * 0.1).astype(np.float16)
    return mask


@pytest.mark.parametrize("case", FA_CASES, ids=[c[0] for c in FA_CASES])
def test_flash_attn_f16_branches(G, torch, case):
    name, DK, DV, H, Hk, N, B, Bk, n_kv, max_bias, split = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    q = rng.standard_normal((B, H, N, DK)).astype(f32)
    k = rng.standard_normal((Bk, Hk, n_kv, DK)).astype(np.float16)
    v = rng.standard_normal((Bk, Hk, n_kv, DV)).astype(np.float16)
    mask = fa_mask(rng, N, n_kv, max_bias)
    scale = float(f32(1.0 / np.sqrt(DK)))
    y = G.op_flash_attn_ext(dev(torch, q), dev(torch, k), dev(torch, v), dev(torch, mask), scale, max_bias, 0.0, split=split).cpu().numpy()
    assert np.isfinite(y).all()
    ref, mag = fa_ref(q, k, v, mask, scale, max_bias, lambda x: x.astype(np.float16))
    path = fa_path(DK, N, H, B, n_kv, split)
    assert name.startswith(path) or (path == "f32" and name.startswith(("split", "single"))), (name, path)
    e = rel_err(y, ref, mag)
    measured(f"fa-{name}", e)
    assert e <= FA_BOUND[path], (name, e)
    if path == "seq" and max_bias == 0.0 and B == 1:
        # the CPU's own arithmetic: every bit of the oracle that is bit-exact with the reference (tests/golden/flash_attn_*.npz)
        want = glue.flash_attn_ext(q, k, v, mask, scale)
        assert np.array_equal(bits(y), bits(want)), (np.abs(y - want).max(), (bits(y) != bits(want)).mean())


def test_flash_attn_q8_0_alibi_twelve_heads(G, torch):
    """k_flash_attn_ext_q80 with ALiBi over 12 heads (m1 slopes): within the last places of the oracle (device powf)."""
    rng = np.random.default_rng(1200)
    H, Hk, N, DK, n_kv = 12, 4, 2, 128, 200
    q = rng.standard_normal((1, H, N, DK)).astype(f32)
    kb = torch.zeros((1, Hk, n_kv, DK // 32 * 34), dtype=torch.uint8, device="cuda"); vb = torch.zeros_like(kb)
    G.op_cpy(dev(torch, rng.standard_normal((1, Hk, n_kv, DK)).astype(f32)), kb)
    G.op_cpy(dev(torch, rng.standard_normal((1, Hk, n_kv, DK)).astype(f32)), vb)
    mask = fa_mask(rng, N, n_kv, 8.0, rows=64)
    y = G.op_flash_attn_ext(dev(torch, q), kb, vb, dev(torch, mask), 0.125, 8.0, 0.0, kv="q8_0").cpu().numpy()
    want = glue.flash_attn_ext_q8_0(q, kb.cpu().numpy(), vb.cpu().numpy(), mask, 0.125, 8.0, 0.0)
    e = rel_err(y, want, np.abs(want).max(axis=-1, keepdims=True))
    measured("fa-q8_0-alibi12", e)
    assert e <= 2.5e-7, e                                                   # (measured on an MI355X: 5.6e-8)


# ================================================================================================ masked positions are never read
# The CPU skips a position whose mask is -inf and never reads its cache row (ggml-cpu/ops.cpp ggml_compute_forward_flash_attn_ext_f16).  On every
# path, finite garbage in the K / V rows of such positions must leave the output bit-identical to zeroed rows; on the decode paths NaN / Inf too.
# The matrix-core prefill paths multiply P by V inside v_mfma, where 0 * NaN is NaN: they assume finite cache rows.
# (path, cache, DK, H, Hk, N, n_kv, split, decode)
MASK_PATHS = [
    ("f16-seq", "f16", 128, 4, 2, 1, 600, True, True),
    ("f16-split", "f16", 80, 4, 2, 1, 700, True, True),
    ("f16-split8", "f16", 128, 4, 2, 2, 2048, True, True),
    ("f16-single", "f16", 128, 4, 2, 2, 1500, False, True),
    ("f16-mfma", "f16", 128, 4, 2, 32, 512, True, False),
    ("bf16-per-row", "bf16", 128, 4, 2, 1, 600, False, True),
    ("bf16-mfma", "bf16", 128, 4, 2, 32, 512, True, False),
    ("q8_0-per-row", "q8_0", 128, 4, 2, 2, 300, True, True),
    ("q8_0-prefill", "q8_0", 128, 4, 2, 32, 512, True, False),
    ("q4_0-per-row", "q4_0", 128, 4, 2, 2, 300, True, True),
    ("q4_0-prefill", "q4_0", 128, 4, 2, 32, 512, True, False),
]


def bf16_bits(x):
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def cache_rows(torch, G, rng, kind, Hk, n_kv, D):
    """a K or V cache [1, Hk, n_kv, row] on the device (f16 / bf16 values, or q8_0 / q4_0 blocks written by the device's CPY)"""
    x = rng.standard_normal((1, Hk, n_kv, D)).astype(f32)
    if kind == "f16":
        return dev(torch, x.astype(np.float16))
    if kind == "bf16":
        return dev(torch, bf16_bits(x).view(np.int16)).view(torch.bfloat16)
    bb = 34 if kind == "q8_0" else 18
    t = torch.zeros((1, Hk, n_kv, D // 32 * bb), dtype=torch.uint8, device="cuda")
    G.op_cpy(dev(torch, x), t, kind)
    return t


def fill_rows(torch, t, rows, kind, what, rng):
    """overwrite cache rows `rows` (positions) with zeros, finite garbage or NaN / Inf"""
    shape = (t.shape[0], t.shape[1], len(rows), t.shape[3])
    if kind in ("f16", "bf16"):
        if what == "zero":
            vals = np.zeros(shape, np.uint16)
        elif what == "finite":                                               # the largest finite f16 magnitude (bf16: its nearest, 65536)
            big = np.float16(65504.0).view(np.uint16) if kind == "f16" else bf16_bits(np.array(65504.0, f32))
            vals = np.where(rng.random(shape) < 0.5, big, big | 0x8000).astype(np.uint16)
        else:
            pool = np.array([0x7E00, 0x7C00, 0xFC00, 0xFE01], np.uint16) if kind == "f16" else np.array([0x7FC0, 0x7F80, 0xFF80, 0xFFC1], np.uint16)
            vals = pool[rng.integers(0, 4, shape)]
        src = torch.from_numpy(vals.view(np.int16)).cuda()
        t.view(torch.int16)[:, :, rows] = src
        return
    bb = 34 if kind == "q8_0" else 18
    nblk = t.shape[3] // bb
    vals = np.zeros(shape[:3] + (nblk, bb), np.uint8)
    if what != "zero":
        vals[...] = rng.integers(0, 256, vals.shape, dtype=np.uint8)
        if what == "finite":                                                 # |d| <= 256: the f16 copy the prefill path decodes stays finite
            d = (rng.uniform(-256, 256, shape[:3] + (nblk,))).astype(np.float16)
        else:
            d = np.array([np.nan, np.inf, -np.inf, np.nan], np.float16)[rng.integers(0, 4, shape[:3] + (nblk,))]
        vals[..., :2] = d.view(np.uint8).reshape(d.shape + (2,))
    t[:, :, rows] = torch.from_numpy(vals.reshape(shape)).cuda()


@pytest.mark.parametrize("case", MASK_PATHS, ids=[c[0] for c in MASK_PATHS])
def test_masked_positions_are_never_read(G, torch, case):
    name, kind, DK, H, Hk, N, n_kv, split, decode = case
    rng = np.random.default_rng(1300 + n_kv + N)
    q = dev(torch, rng.standard_normal((1, H, N, DK)).astype(f32))
    k = cache_rows(torch, G, rng, kind, Hk, n_kv, DK)
    v = cache_rows(torch, G, rng, kind, Hk, n_kv, DK)
    masked = np.sort(np.concatenate([np.arange(n_kv - n_kv // 4, n_kv), rng.choice(n_kv - n_kv // 4, n_kv // 10, replace=False)]))
    mask = np.zeros((N if N >= 16 else 64, n_kv), np.float16)
    mask[:, masked] = -np.inf                                                 # masked for every query row
    md = dev(torch, mask)
    rows = torch.from_numpy(masked).cuda()
    kvarg = dict(kv=kind) if kind in ("q8_0", "q4_0") else {}

    def run(what):
        fill_rows(torch, k, rows, kind, what, rng); fill_rows(torch, v, rows, kind, what, rng)
        return G.op_flash_attn_ext(q, k, v, md, 0.088, 0.0, 0.0, split=split, **kvarg).cpu().numpy()

    base = run("zero")
    assert np.isfinite(base).all()
    for what in ("finite", "nonfinite") if decode else ("finite",):
        y = run(what)
        assert np.array_equal(bits(y), bits(base)), (name, what, int((~np.isfinite(y)).sum()), int((bits(y) != bits(base)).sum()))
