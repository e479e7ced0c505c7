"""A bf16 KV cache (-ctk bf16 -ctv bf16) through the C-ABI: CPY among f32 / f16 / bf16, GET_ROWS from bf16, MUL_MAT with a bf16 src0 and
FLASH_ATTN_EXT on a bf16 K / V cache, against the reference CPU backend's own outputs (tests/golden/bf16_kv_*.npz, made by
make_bf16_kv_golden.py from the x86-64-v3 build).  DESIGN.md section 5.7d states the numerics contract these tests hold the kernels to."""
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden"


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


def dev_bf16(torch, bits):
    """uint16 bf16 bits (numpy) -> a torch.bfloat16 device tensor holding exactly those bits."""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def host_bits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def bf16_rule(x):
    """ggml_compute_fp32_to_bf16 in numpy (pinned to the reference's bits by test_conversion_is_the_reference_rule)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def nmse(y, want):
    y = np.asarray(y, np.float64); want = np.asarray(want, np.float64)
    return float(((y - want) ** 2).sum() / (want ** 2).sum())


# ---------------------------------------------------------------- conversions

def test_conversion_is_the_reference_rule():
    g = np.load(GOLDEN / "bf16_kv_convert.npz", allow_pickle=False)
    assert np.array_equal(bf16_rule(g["x"]), g["bits"])


def test_cpy_f32_to_bf16_bits(G, torch):
    """CPY f32 -> bf16 gives the reference's bits on NaNs, infinities, subnormals and exact ties: element-wise (small), permuted, the row form
    (>= 16384 elements), the transposed form (the -fa 0 V store) and the indirect form of a replayed launch graph."""
    g = np.load(GOLDEN / "bf16_kv_convert.npz", allow_pickle=False)
    x, want = g["x"].reshape(16, 256), g["bits"].reshape(16, 256)
    out = torch.empty((16, 256), dtype=torch.bfloat16, device="cuda")
    G.op_cpy(dev(torch, x), out)
    assert np.array_equal(host_bits(out), want)
    out = torch.empty((256, 16), dtype=torch.bfloat16, device="cuda")            # permuted source
    G.op_cpy(dev(torch, x).t(), out)
    assert np.array_equal(host_bits(out), want.T)
    x4, want4 = np.tile(x, (4, 1)), np.tile(want, (4, 1))                      # 16384 elements: the batch forms
    out = torch.empty((64, 256), dtype=torch.bfloat16, device="cuda")
    G.op_cpy(dev(torch, x4), out)
    assert np.array_equal(host_bits(out), want4)
    out = torch.empty((256, 64), dtype=torch.bfloat16, device="cuda")            # transposed store: source contiguous along its dim 1
    G.op_cpy(dev(torch, x4).t(), out)
    assert np.array_equal(host_bits(out), want4.T)
    cache = torch.zeros((3, 64, 256), dtype=torch.bfloat16, device="cuda")
    table = torch.tensor([0, cache[2].data_ptr()], dtype=torch.int64, device="cuda")
    G.op_cpy_indirect(dev(torch, x4), cache[0], table, 1)                       # (cache[0] gives the shape; the data goes to cache[2])
    assert np.array_equal(host_bits(cache[2]), want4) and not host_bits(cache[0]).any()


def test_cpy_bf16_f16_f32(G, torch):
    """bf16 -> f32 is exact; f16 -> bf16 and bf16 -> f16 go through f32 as the CPU's dup does; bf16 -> bf16 keeps every bit (signalling NaNs too)."""
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2**16, (64, 256), dtype=np.uint64).astype(np.uint16)
    src = dev_bf16(torch, bits)
    out = torch.empty((64, 256), dtype=torch.float32, device="cuda")
    G.op_cpy(src, out)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), bf16_value(bits).view(np.uint32))
    out = torch.empty((64, 256), dtype=torch.bfloat16, device="cuda")
    G.op_cpy(src, out); assert np.array_equal(host_bits(out), bits)
    out = torch.empty((256, 64), dtype=torch.bfloat16, device="cuda")
    G.op_cpy(src.t(), out); assert np.array_equal(host_bits(out), bits.T)
    fin = np.where(np.isfinite(bf16_value(bits)), bits, np.uint16(0x3F80))
    h = torch.empty((64, 256), dtype=torch.float16, device="cuda")
    G.op_cpy(dev_bf16(torch, fin), h)
    assert np.array_equal(h.cpu().numpy().view(np.uint16), bf16_value(fin).astype(np.float16).view(np.uint16))
    hv = rng.standard_normal((8, 40)).astype(np.float16)
    out = torch.empty((8, 40), dtype=torch.bfloat16, device="cuda")
    G.op_cpy(dev(torch, hv), out)
    assert np.array_equal(host_bits(out), bf16_rule(hv.astype(np.float32)))


def test_get_rows_bf16(G, torch):
    rng = np.random.default_rng(4)
    table = bf16_rule(rng.standard_normal((50, 96)).astype(np.float32))
    ids = np.array([7, 0, 49, 7, 13], np.int32)
    y = G.op_get_rows(dev_bf16(torch, table), dev(torch, ids)).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), bf16_value(table[ids]).view(np.uint32))


# ---------------------------------------------------------------- MUL_MAT

@pytest.mark.parametrize("K", [128, 100, 8])
def test_mul_mat_bf16_decode_is_the_cpu(G, torch, K):
    """N = 1..8: ggml_vec_dot_bf16 in its AVX2 order, src1 rounded to bf16 -- the reference's bits (K = 100 / 8: the tail in double)."""
    g = np.load(GOLDEN / "bf16_kv_mul_mat.npz", allow_pickle=False)
    w = dev_bf16(torch, g[f"w_k{K}"])
    for N in range(1, 9):
        y = G.op_mul_mat_f(w, dev(torch, g[f"x_k{K}"][:N])).cpu().numpy()
        assert np.array_equal(y.view(np.uint32), g[f"y_k{K}_n{N}"].view(np.uint32)), (K, N)


def test_mul_mat_bf16_gqa_and_transposed_v(G, torch):
    g = np.load(GOLDEN / "bf16_kv_mul_mat.npz", allow_pickle=False)
    y = G.op_mul_mat_f(dev_bf16(torch, g["w_gqa"]), dev(torch, g["x_gqa"])).cpu().numpy()          # src0 [2, 24, 64] over src1 [4, 3, 64]
    assert np.array_equal(y.view(np.uint32), g["y_gqa"].view(np.uint32))
    cache = dev_bf16(torch, g["cache_vt"])                                                            # [2, DV, n_ctx]: the -fa 0 V cache
    y = G.op_mul_mat_f(cache[:, :, :70], dev(torch, g["x_vt"])).cpu().numpy()                        # rows strided by n_ctx, k = the first 70 positions
    assert np.array_equal(y.view(np.uint32), g["y_vt"].view(np.uint32))


def test_mul_mat_bf16_batch_on_matrix_cores(G, torch):
    """N >= 16: v_mfma_f32_16x16x32_bf16 -- exact products, another summation order."""
    g = np.load(GOLDEN / "bf16_kv_mul_mat.npz", allow_pickle=False)
    y = G.op_mul_mat_f(dev_bf16(torch, g["w_batch"]), dev(torch, g["x_batch"])).cpu().numpy()
    e = nmse(y, g["y_batch"])
    print(f"bf16 MUL_MAT N=32 K=256: NMSE {e:.3e}")
    assert e <= 1e-10, e


# ---------------------------------------------------------------- FLASH_ATTN_EXT

FA = sorted(GOLDEN.glob("bf16_kv_fa_*.npz"))


@pytest.mark.parametrize("path", FA, ids=lambda p: p.stem)
def test_flash_attn_bf16_per_row_is_the_cpu(G, torch, path):
    """One workgroup per row (no workspace; the decode path): q rounded to bf16, ggml_vec_dot_bf16's order, the online softmax in order, the F32
    accumulator -- every output bit of the reference; with ALiBi / soft-capping (device powf / tanhf) within a few units of the last place."""
    g = np.load(path, allow_pickle=False)
    mask = dev(torch, g["mask"]) if "mask" in g else None
    y = G.op_flash_attn_ext(dev(torch, g["q"]), dev_bf16(torch, g["k"]), dev_bf16(torch, g["v"]), mask, float(g["scale"]), float(g["max_bias"]),
                            float(g["softcap"]), split=False).cpu().numpy()
    want = g["y"]
    assert np.isfinite(y).all()
    if float(g["max_bias"]) == 0.0 and float(g["softcap"]) == 0.0:
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), (np.abs(y - want).max(), (y != want).mean())
    else:
        d = np.abs(y.astype(np.float64) - want).max() / np.abs(want).max()
        assert d <= 3e-6, d


@pytest.mark.parametrize("path", FA, ids=lambda p: p.stem)
def test_flash_attn_bf16_with_workspace(G, torch, path):
    """With the workspace: decode-sized calls keep the CPU's bits; a batch of >= 16 queries takes the matrix cores (K q and P V on the bf16
    MFMA, P rounded to bf16) and stays within NMSE 1e-5 of the reference (DESIGN.md 5.7d gives the measured figure)."""
    g = np.load(path, allow_pickle=False)
    mask = dev(torch, g["mask"]) if "mask" in g else None
    y = G.op_flash_attn_ext(dev(torch, g["q"]), dev_bf16(torch, g["k"]), dev_bf16(torch, g["v"]), mask, float(g["scale"]), float(g["max_bias"]),
                            float(g["softcap"]), split=True).cpu().numpy()
    want = g["y"]
    assert np.isfinite(y).all()
    if g["q"].shape[2] >= 16:
        e = nmse(y, want)
        print(f"{path.stem}: NMSE {e:.3e}")
        assert e <= 1e-5, e
    elif float(g["max_bias"]) == 0.0 and float(g["softcap"]) == 0.0:
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32))


def test_flash_attn_bf16_window_8192(G, torch):
    """The longest window accepted: 8192 positions, the cache written by the device's own CPY (its bytes checked by digest), the CPU's bits."""
    g = np.load(GOLDEN / "bf16_kv_long_kv8192.npz", allow_pickle=False)
    rng = np.random.default_rng(int(g["seed"]))
    q = rng.standard_normal((1, 2, 1, 64)).astype(np.float32)
    kf = rng.standard_normal((1, 1, 8192, 64)).astype(np.float32); vf = rng.standard_normal((1, 1, 8192, 64)).astype(np.float32)
    k = torch.empty((1, 1, 8192, 64), dtype=torch.bfloat16, device="cuda"); v = torch.empty_like(k)
    G.op_cpy(dev(torch, kf), k); G.op_cpy(dev(torch, vf), v)
    assert host_bits(k).astype(np.uint64).sum() == g["k_sum"] and host_bits(v).astype(np.uint64).sum() == g["v_sum"]
    mask = np.zeros((64, 8192), np.float16); mask[0, 8000:] = -np.inf
    y = G.op_flash_attn_ext(dev(torch, q), k, v, dev(torch, mask), 0.125, split=True).cpu().numpy()
    assert np.array_equal(y.view(np.uint32), g["y"].view(np.uint32))
    k2 = torch.zeros((1, 1, 8193, 64), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(G.Mi355qError):                                          # (longer windows are declined, not computed otherwise)
        G.op_flash_attn_ext(dev(torch, q), k2, k2, None, 0.125)


def test_flash_attn_mixed_kv_types_declined(G, torch):
    q = torch.zeros((1, 2, 1, 64), dtype=torch.float32, device="cuda")
    k = torch.zeros((1, 1, 32, 64), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(G.Mi355qError):
        G.op_flash_attn_ext(q, k, k.to(torch.float16), None, 0.125)
    with pytest.raises(G.Mi355qError):                                          # a bf16 mask
        G.op_flash_attn_ext(q, k, k, torch.zeros((64, 32), dtype=torch.bfloat16, device="cuda"), 0.125)


def test_decode_loop_bf16_cache(G, torch):
    """24 decode steps at the C-ABI: token t's K / V rows go into position t of a 32-position bf16 cache through op_cpy_indirect (the
    destination read from a device table, as a replayed launch graph does), then attention over the cache with positions > t masked.
    Every step's output and the cache bytes are the reference's."""
    g = np.load(GOLDEN / "bf16_kv_loop.npz", allow_pickle=False)
    qs, kf, vf, ys, n_ctx = g["q"], g["kf"], g["vf"], g["y"], int(g["n_ctx"])
    Hk, D = kf.shape[1], kf.shape[3]
    kc = torch.zeros((1, Hk, n_ctx, D), dtype=torch.bfloat16, device="cuda"); vc = torch.zeros_like(kc)
    kd, vd = dev(torch, kf), dev(torch, vf)
    table = torch.zeros(2, dtype=torch.int64, device="cuda")
    for t in range(qs.shape[0]):
        table.copy_(torch.tensor([kc[:, :, t].data_ptr(), vc[:, :, t].data_ptr()], dtype=torch.int64))
        G.op_cpy_indirect(kd[:, :, t], kc[:, :, 0], table, 0)
        G.op_cpy_indirect(vd[:, :, t], vc[:, :, 0], table, 1)
        mask = np.zeros((64, n_ctx), np.float16); mask[0, t + 1:] = -np.inf
        y = G.op_flash_attn_ext(dev(torch, qs[t]), kc, vc, dev(torch, mask), 0.125).cpu().numpy()
        assert np.array_equal(y.view(np.uint32), ys[t].view(np.uint32)), t
        assert np.array_equal(host_bits(kc)[:, :, :t + 1], g["k"][:, :, :t + 1]) and np.array_equal(host_bits(vc)[:, :, :t + 1], g["v"][:, :, :t + 1]), t
