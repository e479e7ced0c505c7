"""IQ3_S and IQ3_XXS on planar rows (K a multiple of 2048): the layout round trip, the streaming GEMV against the oracle at every step count,
multi-matrix launches, batches on the matrix cores and MUL_MAT_ID.

Bounds are the project's: `check_close` (1e-5 * max|ref| absolute plus 1e-3 relative: the tiers that restate the CPU's integer arithmetic) and
NMSE <= 5e-4 (the reference's op bound, tests/test-backend-ops.cpp:1990: the bf16 matrix-core tier).  A streaming step is 2048 elements for these
types, so K = 2048 is one step, 4096 two, 6144 three and 14336 seven: a wave with one row of K = 2048 keeps most of its ring empty, K = 14336
fills it almost to its depth of 8."""
import numpy as np
import pytest

import oracle
from qdata import quantized_weights, random_blocks

pytestmark = pytest.mark.gpu

IQ3 = [oracle.IQ3_S, oracle.IQ3_XXS]
ids_t = lambda t: oracle.TYPE_NAMES[t]
FORCE_GEMV = 0x4                                            # MI355Q_FLAG_FORCE_GEMV


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


def check_close(y, ref, what=""):
    y = np.asarray(y, np.float32); ref = np.asarray(ref, np.float32)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    assert np.isfinite(y).all(), what
    scale = float(np.abs(ref).max()) or 1.0
    err = np.abs(y - ref)
    assert err.max() <= 1e-5 * scale, f"{what}: max err {err.max():.3e} vs scale {scale:.3e}"
    assert (err <= 1e-3 * np.abs(ref) + 1e-5 * scale).all(), what


def nmse(y, ref):
    y = np.asarray(y, np.float64); ref = np.asarray(ref, np.float64)
    return float(((y - ref) ** 2).sum() / max((ref ** 2).sum(), 1e-300))


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("t", IQ3, ids=ids_t)
def test_planar_rule(G, t):
    assert G.is_planar(t, 2048) and G.is_planar(t, 14336)
    assert not G.is_planar(t, 256)


@pytest.mark.parametrize("t", IQ3, ids=ids_t)
def test_layout_round_trip(G, torch, t):
    """upload -> download and pack_d2d -> unpack_d2d are the identity on canonical bytes; both ways of packing give the same device rows."""
    rng = np.random.default_rng(50 + t)
    L = G.lib()
    for M, K in ((3, 2048), (16, 6144), (5, 14336)):
        w = random_blocks(t, M, K, rng)
        qw = G.QWeight.from_host(t, w, M, K)
        assert np.array_equal(qw.to_host(), w), (ids_t(t), M, K)
        nbytes = w.size
        canon = dev(torch, w.reshape(-1))
        packed = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        back = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        st = int(torch.cuda.current_stream().cuda_stream)
        assert L.mi355q_weights_pack_d2d(t, packed.data_ptr(), canon.data_ptr(), M, K, st) == 0
        assert L.mi355q_weights_unpack_d2d(t, back.data_ptr(), packed.data_ptr(), M, K, st) == 0
        torch.cuda.synchronize()
        assert np.array_equal(back.cpu().numpy(), w.reshape(-1)), (ids_t(t), M, K)
        assert torch.equal(packed, qw.data[:nbytes]), (ids_t(t), M, K)
        assert not np.array_equal(packed.cpu().numpy(), w.reshape(-1))          # (the device rows ARE rearranged)


@pytest.mark.parametrize("t", IQ3, ids=ids_t)
@pytest.mark.parametrize("K", [2048, 4096, 6144, 14336])
def test_gemv_against_oracle(G, torch, orc, t, K):
    """M in {1, 37, 130} x N in {1, 3, 8}: one oracle product per weight set, the smaller shapes are its leading rows and columns (rows and
    columns are independent).  Random blocks make every code-book index, sign pattern and scale nibble occur; quantized weights are what a model holds."""
    rng = np.random.default_rng(1000 * t + K)
    x = (rng.standard_normal((8, K)) * rng.uniform(0.1, 4.0)).astype(np.float32)
    for kind, w, Ms in (("random", random_blocks(t, 130, K, rng), (1, 37, 130)), ("quantized", quantized_weights(t, 37, K, rng), (1, 37))):
        Mw = Ms[-1]
        ref = orc.mul_mat(t, w, x, Mw, 8, K)
        for M in Ms:
            qw = G.QWeight.from_host(t, w[:M], M, K)
            for N in (1, 3, 8):
                y = G.mul_mat(qw, dev(torch, x[:N])).cpu().numpy()
                check_close(y, ref[:N, :M], f"{ids_t(t)} {kind} M={M} N={N} K={K}")


def test_multi_equals_single(G, torch, orc):
    rng = np.random.default_rng(77)
    K = 2048
    specs = [(oracle.IQ3_S, 96), (oracle.Q6_K, 24), (oracle.IQ3_XXS, 40)]
    hosts = [quantized_weights(t, m, K, rng) for t, m in specs]
    ws = [G.QWeight.from_host(t, h, m, K) for (t, m), h in zip(specs, hosts)]
    for N in (1, 4):
        x = dev(torch, rng.standard_normal((N, K)).astype(np.float32))
        multi = [y.cpu().numpy() for y in G.mul_mat_multi(ws, x)]
        for (t, m), h, w, ym in zip(specs, hosts, ws, multi):
            single = G.mul_mat(w, x).cpu().numpy()
            assert np.array_equal(single.view(np.uint32), ym.view(np.uint32)), (ids_t(t), N)
            check_close(ym, orc.mul_mat(t, h, x.cpu().numpy(), m, N, K), f"multi {ids_t(t)} N={N}")


@pytest.mark.parametrize("t", IQ3, ids=ids_t)
def test_batches(G, torch, orc, t):
    """N > 8 on planar rows runs on the matrix cores (bf16 tier: NMSE bound); MI355Q_FLAG_FORCE_GEMV keeps the streaming tier and the CPU's arithmetic."""
    rng = np.random.default_rng(200 + t)
    M, K = 200, 2048
    w = quantized_weights(t, M, K, rng)
    qw = G.QWeight.from_host(t, w, M, K)
    x70 = (rng.standard_normal((70, K)) * 1.3).astype(np.float32)
    ref70 = orc.mul_mat(t, w, x70, M, 70, K)
    for N in (9, 70):
        y = G.mul_mat(qw, dev(torch, x70[:N])).cpu().numpy()
        assert np.isfinite(y).all()
        e = nmse(y, ref70[:N])
        assert e <= 5e-4, f"{ids_t(t)} N={N}: NMSE {e:.3e}"
        yg = G.mul_mat(qw, dev(torch, x70[:N]), flags=FORCE_GEMV).cpu().numpy()
        check_close(yg, ref70[:N], f"{ids_t(t)} N={N} forced GEMV")


@pytest.mark.parametrize("t", IQ3, ids=ids_t)
@pytest.mark.parametrize("n_tok", [2, 20])
def test_mul_mat_id(G, torch, orc, t, n_tok):
    """4 experts, 2 used: 4 pairs and 40 pairs.  Planar IQ3 rows are never grouped onto the matrix cores: every pair is one streamed column at
    either count, so both are held to `check_close` (which is inside the op bound NMSE <= 5e-4 asked of a grouped route, asserted as well).
    One out-of-range id gives a NaN row, every other row is unaffected."""
    rng = np.random.default_rng(300 + t + n_tok)
    ne, nu, M, K = 4, 2, 64, 2048
    as_ = quantized_weights(t, ne * M, K, rng)
    w = G.QWeight.from_host(t, as_, M, K, n_expert=ne)
    good = np.stack([rng.permutation(ne)[:nu] for _ in range(n_tok)]).astype(np.int32)
    b = rng.uniform(-1, 1, (n_tok, 1, K)).astype(np.float32)
    ref = orc.mul_mat_id(t, as_, b, good, M, K, ne)
    y = G.mul_mat_id(w, dev(torch, b), dev(torch, good)).cpu().numpy()
    check_close(y, ref, f"{ids_t(t)} {n_tok * nu} pairs")
    e = nmse(y, ref)
    assert e <= 5e-4, f"{ids_t(t)} {n_tok * nu} pairs: NMSE {e:.3e}"
    bad = good.copy(); bad[n_tok - 1, 1] = ne
    yb = G.mul_mat_id(w, dev(torch, b), dev(torch, bad)).cpu().numpy()
    assert np.isnan(yb[n_tok - 1, 1]).all()
    ok = np.ones((n_tok, nu), bool); ok[n_tok - 1, 1] = False
    assert np.array_equal(yb[ok].view(np.uint32), y[ok].view(np.uint32))
