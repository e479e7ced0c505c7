"""A Q4_1 / Q5_0 / Q5_1 / IQ4_NL KV cache on the device (-ctk T -ctv T): the stores (CPY f32 -> T, direct and through the destination table) and
FLASH_ATTN_EXT, against tests/kvq_ref.py -- pinned bit for bit to the reference CPU backend by tests/test_kvq_golden.py -- and against the
reference's own fixtures (tests/golden/kvq_*.npz).

  * stores: every byte (an all-small IQ4_NL block stores d = 0 and zero indices, where the CPU's index bytes are undefined);
  * decode-sized calls (< 16 query rows): every output bit in the plain cases; ALiBi / soft-cap (device powf / tanhf) within 1e-5 of max|want|, the
    bound the Q8_0 cache is held to (tests/test_gpu_glue.py); masked positions are never read, whatever their rows hold;
  * >= 16 query rows with a workspace: the cache is decoded once into f16 scratch and the matrix-core path runs q in f16 against it -- a deviation
    by design, measured as NMSE against the REFERENCE's output on the prefill fixture and bounded by four times the worst value.
"""
from pathlib import Path

import numpy as np
import pytest

import kvq_ref

pytestmark = pytest.mark.gpu
# q for the scores: the device quantizes with 1 / (amax / 127) (the shared GEMV-path quantizer), kvq_ref with the reference's 127 / amax; the two
# can differ by one quant step on a near-tie of x * id ("q's quantizer").  No input of this file lands on one; a new shape that
# fails by exactly one quant of q in one block has met it.

GOLDEN = Path(__file__).resolve().parent / "golden"
KVS = list(kvq_ref.TYPES)
# NMSE of the f16-scratch route against the reference on kvq_<type>_fa_prefill_gqa_d128_kv256.npz, measured on an MI355X;
# Q8_0 / Q4_0 measured the same way in the same run (same shape and mask, random K / V stored by the device's CPY): 3.05e-5 / 3.00e-5.
# Bound: four times the worst of the four (the margin covers other shapes' spread).
PREFILL_NMSE = {"q4_1": 3.325e-5, "q5_0": 3.098e-5, "q5_1": 2.837e-5, "iq4_nl": 2.677e-5}
PREFILL_NMSE_BOUND = 4 * max(PREFILL_NMSE.values())


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


def store(G, torch, x, kv):
    """op_cpy f32 [..., n] -> uint8 [..., n / 32 * BB] on the device."""
    out = torch.zeros(tuple(x.shape[:-1]) + (x.shape[-1] // 32 * kvq_ref.block_bytes(kv),), dtype=torch.uint8, device="cuda")
    G.op_cpy(x, out, kv=kv)
    return out


@pytest.mark.parametrize("kv", KVS)
def test_cpy_stores_the_reference_bytes(G, torch, kv):
    z = np.load(GOLDEN / f"kvq_{kv}_store.npz", allow_pickle=False)
    got = store(G, torch, dev(torch, z["x"]), kv).cpu().numpy()
    bad = np.argwhere(got != z["blocks"])
    assert bad.size == 0, (kv, bad[:8], got[bad[0][0], :24], z["blocks"][bad[0][0], :24])


@pytest.mark.parametrize("kv", KVS)
def test_cpy_strided_source_and_indirect_destination(G, torch, kv):
    bb = kvq_ref.block_bytes(kv)
    rng = np.random.default_rng(33 + bb)
    x = (rng.standard_normal((3, 5, 256)) * rng.uniform(0.01, 20.0, (3, 5, 1))).astype(np.float32)
    x[1, 2, 32:64] = 0.0
    x[0, 0, 3] = 7.25; x[0, 0, 17] = -7.25; x[0, 0, :32] = np.clip(x[0, 0, :32], -7.25, 7.25)
    want = kvq_ref.quantize_rows(kv, x)
    big = dev(torch, np.concatenate([x, np.zeros_like(x)], axis=-1))     # rows with a gap: source stride 512 floats
    got = store(G, torch, big[..., :256], kv).cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    # through the destination table: two rows stored at moving places of a cache, everything else untouched
    cache = torch.full((8, 256 // 32 * bb), 0xA5, dtype=torch.uint8, device="cuda")
    row = 256 // 32 * bb
    table = torch.tensor([cache.data_ptr() + 5 * row, cache.data_ptr() + 2 * row], dtype=torch.int64, device="cuda")
    view = torch.zeros((1, row), dtype=torch.uint8, device="cuda")
    G.op_cpy_indirect(big[0, 1:2, :256], view, table, 0, kv=kv)
    G.op_cpy_indirect(big[2, 4:5, :256], view, table, 1, kv=kv)
    c = cache.cpu().numpy()
    assert np.array_equal(c[5], want[0, 1]) and np.array_equal(c[2], want[2, 4])
    assert (c[[0, 1, 3, 4, 6, 7]] == 0xA5).all() and (view.cpu().numpy() == 0).all()


# (n_head, n_head_kv, n_queries, head_dim, n_kv, first masked position of query 0, max_bias, soft-cap): tests/test_gpu_glue.py's Q8_0 shapes,
# a head size of 96 (an odd block count: IQ4_NL's scalar tail) and a soft-capped one
CFGS = [(8, 2, 1, 128, 256, 201, 0.0, 0.0), (4, 4, 3, 64, 96, 60, 0.0, 0.0), (8, 8, 2, 128, 64, 55, 8.0, 0.0), (2, 1, 1, 256, 40, 30, 0.0, 0.0),
        (4, 2, 3, 96, 70, 50, 0.0, 0.0), (4, 1, 1, 96, 64, 64, 0.0, 10.0), (4, 4, 1, 32, 33, 33, 0.0, 0.0)]


@pytest.mark.parametrize("cfg", CFGS, ids=str)
@pytest.mark.parametrize("kv", KVS)
def test_flash_attn_ext_on_the_devices_own_cache(G, torch, kv, cfg):
    H, Hk, N, DK, n_kv, first_masked, max_bias, softcap = cfg
    rng = np.random.default_rng(sum(cfg[:6]) + kvq_ref.block_bytes(kv))
    q = rng.standard_normal((1, H, N, DK)).astype(np.float32)
    kf = rng.standard_normal((1, Hk, n_kv, DK)).astype(np.float32); vf = rng.standard_normal((1, Hk, n_kv, DK)).astype(np.float32)
    kb, vb = store(G, torch, dev(torch, kf), kv), store(G, torch, dev(torch, vf), kv)
    assert np.array_equal(kb.cpu().numpy(), kvq_ref.quantize_rows(kv, kf))
    mask = np.zeros((64, n_kv), np.float16)
    for t in range(N):
        mask[t, first_masked + t:] = -np.inf
    if max_bias > 0:
        mask[:N] += (rng.standard_normal((N, n_kv)) * 0.1).astype(np.float16)
    scale = float(np.float32(1.0 / np.sqrt(DK)))
    y = G.op_flash_attn_ext(dev(torch, q), kb, vb, dev(torch, mask), scale, max_bias, softcap, kv=kv).cpu().numpy()
    want = kvq_ref.flash_attn_ext(kv, q, kb.cpu().numpy(), vb.cpu().numpy(), mask, scale, max_bias, softcap)
    assert np.isfinite(y).all()
    d = np.abs(y.astype(np.float64) - want); top = np.abs(want).max()
    differ = (y.view(np.uint32) != want.view(np.uint32)).mean()
    print(f"{kv} {cfg}: max error {d.max() / top:.2e} of max|want|, {differ:.4f} of the outputs differ")
    plain = max_bias == 0.0 and softcap == 0.0
    assert d.max() <= 1e-5 * top and (differ == 0.0 if plain else True), (cfg, kv, d.max() / top, differ)
    if plain and N < 16:
        # masked positions are never read: NaN / Inf / +-65504 in their rows (scales, minima and quants alike) change no output bit
        kb2, vb2 = kb.cpu().numpy().copy(), vb.cpu().numpy().copy()
        bb = kvq_ref.block_bytes(kv)
        dead = first_masked + N - 1                                          # masked for every query row
        if dead < n_kv:
            for c, pat in ((kb2, [0x00, 0x7E]), (vb2, [0x00, 0x7C])):           # f16 NaN / +Inf scales
                blk = c[:, :, dead:].reshape(c.shape[0], c.shape[1], n_kv - dead, DK // 32, bb)
                blk[..., 0:2] = np.array(pat, np.uint8)
                blk[..., 2:4] = np.array([0xFF, 0x7B] if c is kb2 else [0xFF, 0xFB], np.uint8)     # +-65504 (the minimum of Q4_1 / Q5_1)
                blk[..., 4:] = 0xFF
            y2 = G.op_flash_attn_ext(dev(torch, q), dev(torch, kb2), dev(torch, vb2), dev(torch, mask), scale, kv=kv).cpu().numpy()
            assert np.array_equal(y2.view(np.uint32), y.view(np.uint32))


PLAIN_FIXTURES = ["decode_gqa_d128_kv256", "decode_gqa_d256_kv128", "decode_nomask_d64_kv1", "batch3_d96_kv40"]


@pytest.mark.parametrize("tag", PLAIN_FIXTURES + ["alibi_d128_kv64", "softcap_d96_kv64"])
@pytest.mark.parametrize("kv", KVS)
def test_flash_attn_ext_reference_fixtures(G, torch, kv, tag):
    z = np.load(GOLDEN / f"kvq_{kv}_fa_{tag}.npz", allow_pickle=False)
    mask = dev(torch, z["mask"]) if "mask" in z.files else None
    y = G.op_flash_attn_ext(dev(torch, z["q"]), dev(torch, z["k"]), dev(torch, z["v"]), mask, float(z["scale"]), float(z["max_bias"]), float(z["softcap"]), kv=kv).cpu().numpy()
    want = z["y"]
    d = np.abs(y.astype(np.float64) - want); top = np.abs(want).max()
    differ = (y.view(np.uint32) != want.view(np.uint32)).mean()
    print(f"{kv} {tag}: max error {d.max() / top:.2e} of max|want|, {differ:.4f} of the outputs differ")
    assert d.max() <= 1e-5 * top and (differ == 0.0 if tag in PLAIN_FIXTURES else True), (kv, tag, d.max() / top, differ)


@pytest.mark.parametrize("kv", KVS)
def test_longest_window_8192(G, torch, kv):
    z = np.load(GOLDEN / f"kvq_{kv}_long_kv8192.npz", allow_pickle=False)
    rng = np.random.default_rng(int(z["seed"]))
    q = rng.standard_normal((1, 2, 1, 64)).astype(np.float32)
    kf = rng.standard_normal((1, 1, 8192, 64)).astype(np.float32); vf = rng.standard_normal((1, 1, 8192, 64)).astype(np.float32)
    kb, vb = store(G, torch, dev(torch, kf), kv), store(G, torch, dev(torch, vf), kv)
    mask = np.zeros((64, 8192), np.float16); mask[0, 8000:] = -np.inf
    y = G.op_flash_attn_ext(dev(torch, q), kb, vb, dev(torch, mask), 0.125, kv=kv).cpu().numpy()
    want = kvq_ref.flash_attn_ext(kv, q, kb.cpu().numpy(), vb.cpu().numpy(), mask, 0.125)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), np.abs(y - want).max()
    # the device's stores have the digests of the reference's from_float rows; the output is the reference's where the fixture has one (IQ4_NL: the
    # reference's window is ggml_quantize_chunk's, not a store's)
    assert int(kb.cpu().numpy().astype(np.uint64).sum()) == int(z["k_sum"]) and int(vb.cpu().numpy().astype(np.uint64).sum()) == int(z["v_sum"])
    if "y" in z.files:
        assert np.array_equal(y.view(np.uint32), z["y"].view(np.uint32))
    with pytest.raises(G.Mi355qError):
        G.op_flash_attn_ext(dev(torch, q), torch.zeros((1, 1, 8224, 2 * kvq_ref.block_bytes(kv)), dtype=torch.uint8, device="cuda"),
                            torch.zeros((1, 1, 8224, 2 * kvq_ref.block_bytes(kv)), dtype=torch.uint8, device="cuda"), None, 0.125, kv=kv)


def _nmse(y, want):
    return float(((y.astype(np.float64) - want) ** 2).sum() / (want.astype(np.float64) ** 2).sum())


@pytest.mark.parametrize("kv", KVS + ["q8_0", "q4_0"])
def test_prefill_route_through_f16_scratch(G, torch, kv):
    """>= 16 query rows: NMSE against the reference's output.  The Q8_0 / Q4_0 figures are printed beside the new types' (their cache is the same
    f32 K / V stored by the device's CPY, the reference output comes from oracle.glue's restatement)."""
    if kv in KVS:
        z = np.load(GOLDEN / f"kvq_{kv}_fa_prefill_gqa_d128_kv256.npz", allow_pickle=False)
        q, mask, scale, want = z["q"], z["mask"], float(z["scale"]), z["y"]
        kb, vb = dev(torch, z["k"]), dev(torch, z["v"])
    else:
        from oracle import glue
        rng = np.random.default_rng(48)
        q = rng.standard_normal((1, 4, 48, 128)).astype(np.float32)
        kf = rng.standard_normal((1, 2, 256, 128)).astype(np.float32); vf = rng.standard_normal((1, 2, 256, 128)).astype(np.float32)
        bb = 34 if kv == "q8_0" else 18
        kb = torch.zeros((1, 2, 256, 128 // 32 * bb), dtype=torch.uint8, device="cuda"); vb = torch.zeros_like(kb)
        G.op_cpy(dev(torch, kf), kb, kv); G.op_cpy(dev(torch, vf), vb, kv)
        mask = np.zeros((64, 256), np.float16)
        for t in range(48):
            mask[t, 200 + t:] = -np.inf
        scale = float(np.float32(1.0 / np.sqrt(128)))
        want = glue.flash_attn_ext_q8_0(q, kb.cpu().numpy(), vb.cpu().numpy(), mask, scale, kv=kv)
    y = G.op_flash_attn_ext(dev(torch, q), kb, vb, dev(torch, mask), scale, kv=kv).cpu().numpy()
    e = _nmse(y, want)
    print(f"prefill route, {kv} cache: NMSE {e:.3e} against the reference (bound {PREFILL_NMSE_BOUND:.1e})")
    assert np.isfinite(y).all()
    if kv in KVS:
        assert e <= PREFILL_NMSE_BOUND, (kv, e)
    # without the workspace the same call walks every row with the CPU's arithmetic: the reference's bits
    y1 = G.op_flash_attn_ext(dev(torch, q), kb, vb, dev(torch, mask), scale, split=False, kv=kv).cpu().numpy()
    assert np.array_equal(y1.view(np.uint32), want.view(np.uint32)), (kv, np.abs(y1 - want).max())


@pytest.mark.parametrize("kv", KVS + ["q8_0", "q4_0"])
def test_mul_mat_over_a_cache_view(G, torch, kv):
    """The KQ product of a non-flash graph over a quantized K cache (op_mul_mat_f with block rows as src0): q quantized to the type's vec_dot_type,
    the type's vec_dot per position -- the scores of FLASH_ATTN_EXT before the scale.  Bit for bit against kvq_ref.vec_dot (the new types) and
    oracle/glue.py's Q8_0 / Q4_0 dot, both pinned to the reference."""
    bb = G.KV_BLOCK[kv][0]
    H, Hk, N, D, n_kv = 4, 2, 3, 96, 300
    rng = np.random.default_rng(bb + 7)
    q = rng.standard_normal((1, H, N, D)).astype(np.float32)
    kf = rng.standard_normal((1, Hk, n_kv, D)).astype(np.float32)
    kb = torch.zeros((1, Hk, n_kv, D // 32 * bb), dtype=torch.uint8, device="cuda")
    G.op_cpy(dev(torch, kf), kb, kv=kv)
    y = G.op_mul_mat_f(kb, dev(torch, q), kv=kv).cpu().numpy()            # [1, H, N, n_kv]
    assert y.shape == (1, H, N, n_kv) and np.isfinite(y).all()
    if kv in KVS:
        kd, km, kq = kvq_ref.unpack(kv, kb.cpu().numpy())
        for h in range(H):
            for n in range(N):
                qd, qs, qq = kvq_ref.quantize_q(q[0, h, n], kv in ("q4_1", "q5_1"))
                want = kvq_ref.vec_dot(kv, kd[0, h // 2], km[0, h // 2] if km is not None else None, kq[0, h // 2], qd, qs, qq)
                assert np.array_equal(y[0, h, n].view(np.uint32), want.view(np.uint32)), (kv, h, n, np.abs(y[0, h, n] - want).max())
    else:
        from oracle import glue
        b = kb.cpu().numpy().reshape(1, Hk, n_kv, D // 32, bb)
        kd = np.ascontiguousarray(b[..., :2]).view(np.float16)[..., 0]
        if kv == "q8_0":
            kq = np.ascontiguousarray(b[..., 2:]).view(np.int8)
        else:
            qs = b[..., 2:].astype(np.int16); kq = np.concatenate([(qs & 15) - 8, (qs >> 4) - 8], axis=-1).astype(np.int8)
        for h in range(H):
            for n in range(N):
                qdn, qqn = glue.quantize_row_q8_0_simd(q[0, h, n])
                want = glue.vec_dot_q8_0_q8_0_simd(kd[0, h // 2], kq[0, h // 2], qdn, qqn)
                assert np.array_equal(y[0, h, n].view(np.uint32), want.view(np.uint32)), (kv, h, n)


def test_mixed_cache_types_are_refused(G, torch):
    q = torch.zeros((1, 2, 1, 64), dtype=torch.float32, device="cuda")
    k = torch.zeros((1, 1, 32, 2 * 20), dtype=torch.uint8, device="cuda"); v = torch.zeros((1, 1, 32, 2 * 24), dtype=torch.uint8, device="cuda")
    import ctypes as C
    out = torch.zeros((1, 1, 2, 64), dtype=torch.float32, device="cuda")
    tq, tk, tv, to = G._td(q), G._td_q8_0(k, "q4_1"), G._td_q8_0(v, "q5_1"), G._td(out)
    rc = G.lib().mi355q_op_flash_attn_ext(C.byref(tq), C.byref(tk), C.byref(tv), None, C.byref(to), 0.125, 0.0, 0.0, None, 0, None)
    assert rc != 0
