"""FLASH_ATTN_EXT over a mixed KV cache (-ctk A -ctv B; MI355Q_FA_KV_MIXED) on the device.

  row kernel (k_flash_attn_ext_mix, csrc/fattn_mix.hip)   the CPU's bits: np.array_equal on uint32 views against the reference's own outputs
                                                           (tests/golden/kvmix_*.npz) and against the numpy restatement tests/kvmix_ref.py, which
                                                           tests/test_kvmix_ref_cpu.py pins to those fixtures
  fused kernel on the cache's own rows (FUSED_KV)          bit for bit the f16 fused kernel on the f16 copies of both sides, the method of
                                                           tests/test_gpu_fa_kv.py direct_vs_f16_copy
  f16-copy route for prompts                               bit for bit the f16 call on host-built copies
  refusals                                                 the return code only; nothing is launched
"""
import ctypes as C
import zlib
from pathlib import Path

import numpy as np
import pytest

import kvmix_ref
from test_gpu_fa_fused import G, dev, fa_mask, torch  # noqa: F401 (fixtures)
from test_gpu_fa_kv import bits, f16_copy, llama_layout

f32 = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden"
TYPES = kvmix_ref.TYPES
PAIRS = [(kt, vt) for kt in TYPES for vt in TYPES if kt != vt]
BUILT = [(kt, vt) for kt, vt in PAIRS if kt in ("f16", "q8_0") or vt in ("f16", "q8_0")]      # the fused kernel's 22 mixed pairs
NOT_BUILT = [p for p in PAIRS if p not in BUILT]
RING = kvmix_ref.RING
RING_BUILT = [p for p in RING if p in BUILT]
RING_TAGS = ["decode_gqa_d128_kv256", "batch3_dk64_dv96_kv40_alibi", "softcap_d96_kv64", "decode_nomask_d64_kv1"]
ids = lambda pairs: [f"{k}-{v}" for k, v in pairs]


def to_dev(torch, t, a):
    """one cache side as stored (uint8 bytes) -> the device tensor op_flash_attn_ext takes: f16 values or uint8 block rows"""
    d = dev(torch, a)
    return d.view(torch.float16) if t == "f16" else d


def kw(kt, vt, **more):
    return dict(kv=kt if kt != "f16" else "q8_0", kv_v=vt if vt != "f16" else "q8_0", kv_mixed=True, **more)


def side_f16(t, a):
    """the f16 copy of one side: an f16 side is its own copy"""
    return np.ascontiguousarray(a).view(np.float16) if t == "f16" else f16_copy(t, a)


_CACHE = {}


def mix_case(G, torch, kt, vt, name, DK, DV, H, Hk, N, n_kv, mask=True, first_sees=None):
    """seeded normals; a block side quantized by the device's own op_cpy, an f16 side rounded -> (q, k bytes, v bytes, k16, v16, mask, scale), once per case"""
    key = (kt, vt, name, DK, DV, H, Hk, N, n_kv, mask, first_sees)
    if key not in _CACHE:
        rng = np.random.default_rng(zlib.crc32(f"{kt}-{vt}-{name}".encode()))
        q = rng.standard_normal((1, H, N, DK)).astype(f32)
        kf = rng.standard_normal((1, Hk, n_kv, DK)).astype(f32)
        vf = rng.standard_normal((1, Hk, n_kv, DV)).astype(f32)

        def store(t, x):
            if t == "f16":
                return np.ascontiguousarray(x.astype(np.float16)).view(np.uint8)
            out = torch.zeros(x.shape[:-1] + (x.shape[-1] // 32 * G.KV_BLOCK[t][0],), dtype=torch.uint8, device="cuda")
            G.op_cpy(dev(torch, x), out, kv=t)
            return out.cpu().numpy()
        kb, vb = store(kt, kf), store(vt, vf)
        m = fa_mask(rng, N, n_kv) if mask else None
        if first_sees is not None:
            for t in range(N):
                m[t, first_sees + t:] = -np.inf
        _CACHE[key] = (q, kb, vb, side_f16(kt, kb), side_f16(vt, vb), m, float(f32(1.0 / np.sqrt(DK))))
    return _CACHE[key]


@pytest.fixture
def auto(monkeypatch):
    monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    monkeypatch.delenv("MI355Q_FA_EXACT", raising=False)


# ------------------------------------------------------------------------------------------------ the row kernel against the reference's outputs
def row_call(G, torch, kt, vt, q, k, v, mask, scale, max_bias=0.0, softcap=0.0, kd=None, vd=None):
    qd = dev(torch, q); md = dev(torch, mask) if mask is not None else None
    kd = to_dev(torch, kt, k) if kd is None else kd; vd = to_dev(torch, vt, v) if vd is None else vd
    assert G.op_flash_attn_ext_path(qd, kd, vd, md, softcap, split=False, **kw(kt, vt)) == G.FA_PATH_KV_ROW
    return G.op_flash_attn_ext(qd, kd, vd, md, scale, max_bias, softcap, split=False, **kw(kt, vt)).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", PAIRS, ids=ids(PAIRS))
def test_row_all_pairs_fixture(G, torch, auto, kt, vt):
    z = np.load(GOLDEN / "kvmix_all_pairs_d64_kv96.npz", allow_pickle=False)
    y = row_call(G, torch, kt, vt, z["q"], z[f"k_{kt}"], z[f"v_{vt}"], z["mask"], float(z["scale"]))
    want = z[f"y_{kt}_{vt}"]
    assert np.array_equal(bits(y), bits(want)), float(np.abs(y - want).max())


@pytest.mark.gpu
@pytest.mark.parametrize("tag", RING_TAGS)
@pytest.mark.parametrize("kt,vt", RING, ids=ids(RING))
def test_row_ring_fixtures(G, torch, auto, kt, vt, tag):
    """The reference's outputs bit for bit, the soft-cap and ALiBi shapes included.  The soft-cap cases hold because the kernel applies `softcap * tanhf(s)` with
    the host C library's tanhf restated (csrc/tanhf_libm.h), not the device library's, which differs from it in the last bits: with the latter these seven
    cases miss by one to a few f32 ulps (1.2e-07 .. 1.8e-07 on outputs up to 0.26), and by one f16 ulp (1.5e-04) under the F16 accumulator of iq4_nl-f16.
    The ALiBi cases hold with the device's powf: the fixture's slopes are powers of two."""
    z = np.load(GOLDEN / f"kvmix_{kt}_{vt}_{tag}.npz", allow_pickle=False)
    mask = z["mask"] if "mask" in z.files else None
    y = row_call(G, torch, kt, vt, z["q"], z["k"], z["v"], mask, float(z["scale"]), float(z["max_bias"]), float(z["softcap"]))
    assert np.array_equal(bits(y), bits(z["y"])), float(np.abs(y - z["y"]).max())


# ------------------------------------------------------------------------------------------------ the row kernel against the restatement
@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", [("q8_0", "q4_0"), ("f16", "q8_0"), ("iq4_nl", "f16")], ids=lambda p: p)
def test_row_last_decode_row_count(G, torch, auto, kt, vt):
    """N = 15 with a workspace on offer: still the row kernel (16 rows would take the f16 copy)"""
    q, kb, vb, _, _, m, scale = mix_case(G, torch, kt, vt, "n15", 64, 64, 2, 1, 15, 70)
    qd, kd, vd, md = dev(torch, q), to_dev(torch, kt, kb), to_dev(torch, vt, vb), dev(torch, m)
    assert G.op_flash_attn_ext_path(qd, kd, vd, md, kv_direct=True, **kw(kt, vt)) == G.FA_PATH_KV_ROW
    y = G.op_flash_attn_ext(qd, kd, vd, md, scale, kv_direct=True, **kw(kt, vt)).cpu().numpy()
    want = kvmix_ref.flash_attn_ext(kt, vt, q, kb, vb, m, scale)
    assert np.array_equal(bits(y), bits(want)), float(np.abs(y - want).max())


def layout_dev(torch, t, a, extra_rows=0, fill=0):
    d = llama_layout(torch, a, extra_rows, fill)
    return d.view(torch.float16) if t == "f16" else d


@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", [("q4_0", "q5_0"), ("q5_0", "f16"), ("f16", "iq4_nl")], ids=lambda p: p)
def test_row_llama_layout_blocks_at_2_mod_4(G, torch, auto, kt, vt):
    """three heads of ONE block each side by side in one cache buffer: a head's row starts at h * 18 / 22 bytes -- 2 mod 4 for the middle head"""
    q, kb, vb, _, _, m, scale = mix_case(G, torch, kt, vt, "d32-h3", 32, 32, 3, 3, 2, 96)
    kd, vd = layout_dev(torch, kt, kb), layout_dev(torch, vt, vb)
    for t, d in ((kt, kd), (vt, vd)):
        if t != "f16":
            assert d[0, 1].data_ptr() % 4 == 2
    y = row_call(G, torch, kt, vt, q, kb, vb, m, scale, kd=kd, vd=vd)
    want = kvmix_ref.flash_attn_ext(kt, vt, q, kb, vb, m, scale)
    assert np.array_equal(bits(y), bits(want)), float(np.abs(y - want).max())


@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", [("q8_0", "q4_0"), ("f16", "q4_1"), ("q5_1", "f16")], ids=lambda p: p)
def test_row_masked_rows_and_rows_behind_the_window_are_never_used(G, torch, auto, kt, vt):
    """0xFF bytes (NaN scales, NaN halves) in every row that is masked for all queries and in 16 rows behind the window: the bits of clean rows"""
    q, kb, vb, _, _, m, scale = mix_case(G, torch, kt, vt, "nan-rows", 64, 64, 2, 1, 3, 80)
    dead = np.isinf(m[:, :80]).all(axis=0)
    assert dead.sum() >= 3 and not dead.all()
    outs = []
    for fill in (0xFF, 0x00):
        k2, v2 = kb.copy(), vb.copy()
        k2[:, :, dead] = fill; v2[:, :, dead] = fill
        outs.append(row_call(G, torch, kt, vt, q, k2, v2, m, scale, kd=layout_dev(torch, kt, k2, 16, fill), vd=layout_dev(torch, vt, v2, 16, fill)))
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    want = kvmix_ref.flash_attn_ext(kt, vt, q, kb, vb, m, scale)
    assert np.array_equal(bits(outs[0]), bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", [("f16", "q8_0"), ("q8_0", "q4_0")], ids=lambda p: p)
def test_row_longest_window(G, torch, auto, kt, vt):
    """n_kv = 8192, the last window of the row kernel: 64 KiB of scores and factors in LDS, above the default dynamic limit"""
    q, kb, vb, _, _, m, scale = mix_case(G, torch, kt, vt, "kv8192", 32, 32, 1, 1, 1, 8192)
    y = row_call(G, torch, kt, vt, q, kb, vb, m, scale)
    want = kvmix_ref.flash_attn_ext(kt, vt, q, kb, vb, m, scale)
    assert np.array_equal(bits(y), bits(want)), float(np.abs(y - want).max())


# ------------------------------------------------------------------------------------------------ the fused kernel on the cache's own rows
def direct_vs_f16_copy(G, torch, monkeypatch, kt, vt, case, forced=True, layout=False, split=True, softcap=0.0):
    q, kb, vb, k16, v16, m, scale = case
    if forced:
        monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    else:
        monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    qd, md = dev(torch, q), dev(torch, m) if m is not None else None
    kd, vd = (layout_dev(torch, kt, kb), layout_dev(torch, vt, vb)) if layout else (to_dev(torch, kt, kb), to_dev(torch, vt, vb))
    assert G.op_flash_attn_ext_path(qd, kd, vd, md, softcap, split=split, kv_direct=True, **kw(kt, vt)) == G.FA_PATH_FUSED_KV
    y = G.op_flash_attn_ext(qd, kd, vd, md, scale, 0.0, softcap, split=split, kv_direct=True, **kw(kt, vt)).cpu().numpy()
    k16d, v16d = dev(torch, k16), dev(torch, v16)
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")                                 # the yardstick: the f16 fused kernel on the f16 copies
    N = q.shape[2]
    if N < 16:
        # the f16 rule sends no call of < 16 rows to the fused kernel inside 36864 positions: the same rows in a batch of 16 whose other rows are fully
        # masked (a row's result does not depend on its neighbours, and fully masked rows keep no tile alive)
        q16 = np.concatenate([q, np.zeros((1, q.shape[1], 16 - N, q.shape[3]), f32)], axis=2)
        m16 = np.concatenate([m, np.full((16 - N, m.shape[1]), -np.inf, np.float16)], axis=0)
        qd, md = dev(torch, q16), dev(torch, m16)
    assert G.op_flash_attn_ext_path(qd, k16d, v16d, md, softcap) == G.FA_PATH_FUSED
    want = G.op_flash_attn_ext(qd, k16d, v16d, md, scale, 0.0, softcap).cpu().numpy()[:, :N]
    assert np.isfinite(want).all()
    assert np.array_equal(bits(y), bits(want)), (kt, vt, float(np.abs(y - want).max()))
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", BUILT, ids=ids(BUILT))
def test_fused_one_full_tile(G, torch, monkeypatch, kt, vt):
    direct_vs_f16_copy(G, torch, monkeypatch, kt, vt, mix_case(G, torch, kt, vt, "one-tile", 64, 64, 2, 1, 64, 64, mask=False))


@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", RING_BUILT, ids=ids(RING_BUILT))
def test_fused_partial_tiles_dead_last_tile(G, torch, monkeypatch, kt, vt):
    """N = 70 over n_kv = 200 at head size 128; row t sees positions < 128 + t: the last tile is dead for the first 64 rows, live and partial for the rest"""
    case = mix_case(G, torch, kt, vt, "n70-kv200", 128, 128, 4, 2, 70, 200, first_sees=128)
    m = case[5]
    assert np.isinf(m[:64, 192:200]).all() and not np.isinf(m[64:, 192:200]).all()
    direct_vs_f16_copy(G, torch, monkeypatch, kt, vt, case)


@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", [("q8_0", "q5_1"), ("q4_1", "f16")], ids=lambda p: p)
def test_fused_head_size_256(G, torch, monkeypatch, kt, vt):
    direct_vs_f16_copy(G, torch, monkeypatch, kt, vt, mix_case(G, torch, kt, vt, "d256", 256, 256, 2, 2, 16, 128))


@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", [("q8_0", "q4_0"), ("q5_0", "q8_0"), ("f16", "q5_0")], ids=lambda p: p)
def test_fused_head_size_32_llama_layout(G, torch, monkeypatch, kt, vt):
    direct_vs_f16_copy(G, torch, monkeypatch, kt, vt, mix_case(G, torch, kt, vt, "d32-h3-n16", 32, 32, 3, 3, 16, 96), layout=True)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 15])
@pytest.mark.parametrize("kt,vt", [("q8_0", "q4_0"), ("f16", "q8_0")], ids=lambda p: p)
def test_fused_auto_decode_beyond_the_row_kernel(G, torch, monkeypatch, kt, vt, N):
    """n_kv = 8256 under `auto`: the window the row kernel refuses"""
    direct_vs_f16_copy(G, torch, monkeypatch, kt, vt, mix_case(G, torch, kt, vt, f"n{N}-kv8256", 64, 64, 2, 1, N, 8256), forced=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", [("q8_0", "q4_0"), ("iq4_nl", "f16")], ids=lambda p: p)
def test_fused_auto_prompt_softcap_no_workspace(G, torch, monkeypatch, kt, vt):
    """N = 16 with a soft-cap and no workspace under `auto`: no f16 copy, so the prompt goes to the fused kernel"""
    direct_vs_f16_copy(G, torch, monkeypatch, kt, vt, mix_case(G, torch, kt, vt, "n16-kv8256", 64, 64, 2, 1, 16, 8256), forced=False, split=False, softcap=5.0)


# ------------------------------------------------------------------------------------------------ the f16-copy route
@pytest.mark.gpu
@pytest.mark.parametrize("kt,vt", [("q8_0", "q4_0"), ("f16", "q8_0"), ("q4_0", "q4_1"), ("iq4_nl", "f16")], ids=lambda p: p)
def test_copy_route(G, torch, auto, kt, vt):
    """N = 32, n_kv = 256, d128 with a workspace: the answer is the f16 rule's about the copy, the output the f16 call's on host-built copies"""
    q, kb, vb, k16, v16, m, scale = mix_case(G, torch, kt, vt, "n32-kv256", 128, 128, 4, 2, 32, 256)
    qd, kd, vd, md = dev(torch, q), to_dev(torch, kt, kb), to_dev(torch, vt, vb), dev(torch, m)
    k16d, v16d = dev(torch, k16), dev(torch, v16)
    want_path = G.op_flash_attn_ext_path(qd, k16d, v16d, md)
    assert want_path == G.FA_PATH_MFMA3
    assert G.op_flash_attn_ext_path(qd, kd, vd, md, kv_direct=True, **kw(kt, vt)) == want_path
    y = G.op_flash_attn_ext(qd, kd, vd, md, scale, kv_direct=True, **kw(kt, vt)).cpu().numpy()
    want = G.op_flash_attn_ext(qd, k16d, v16d, md, scale).cpu().numpy()
    assert np.isfinite(want).all()
    assert np.array_equal(bits(y), bits(want)), float(np.abs(y - want).max())


# ------------------------------------------------------------------------------------------------ refusals: the return code, no launch
def raw_call(G, torch, kt, vt, kd, vd, qd, flags, old=False):
    out = torch.empty((1, qd.shape[2], qd.shape[1], 64), dtype=torch.float32, device="cuda")
    td = lambda t, x: G._td_q8_0(x, t) if x.dtype == torch.uint8 else G._td(x)
    args = (C.byref(G._td(qd)), C.byref(td(kt, kd)), C.byref(td(vt, vd)), None, C.byref(G._td(out)), 0.125, 0.0, 0.0, None, 0, None)
    return int(G.lib().mi355q_op_flash_attn_ext(*args)) if old else int(G.lib().mi355q_op_flash_attn_ext2(*args, flags))


@pytest.mark.gpu
def test_refusals(G, torch, auto):
    qd = torch.zeros((1, 2, 1, 64), dtype=torch.float32, device="cuda")
    blocks = lambda t, n_kv: torch.zeros((1, 1, n_kv, 2 * G.KV_BLOCK[t][0]), dtype=torch.uint8, device="cuda")
    both = G.FA_KV_DIRECT | G.FA_KV_MIXED
    # a pair the fused kernel is not built for, beyond the row kernel's window
    assert raw_call(G, torch, "q4_0", "q4_1", blocks("q4_0", 8256), blocks("q4_1", 8256), qd, both) == G.ERR_UNSUPPORTED
    assert raw_call(G, torch, "q8_0", "q4_0", blocks("q8_0", 8256), blocks("q4_0", 8256), qd, G.FA_KV_MIXED) == G.ERR_UNSUPPORTED      # built, but not asked for
    # a bf16 side
    bf = torch.zeros((1, 1, 32, 64), dtype=torch.bfloat16, device="cuda")
    assert raw_call(G, torch, "bf16", "q8_0", bf, blocks("q8_0", 32), qd, both) == G.ERR_UNSUPPORTED
    assert raw_call(G, torch, "q8_0", "bf16", blocks("q8_0", 32), bf, qd, both) == G.ERR_UNSUPPORTED
    assert "bf16" in G.lib().mi355q_last_error().decode()
    # the entry points without the flag
    k, v = blocks("q8_0", 32), blocks("q4_0", 32)
    assert raw_call(G, torch, "q8_0", "q4_0", k, v, qd, 0, old=True) == G.ERR_UNSUPPORTED
    assert raw_call(G, torch, "q8_0", "q4_0", k, v, qd, G.FA_KV_DIRECT) == G.ERR_UNSUPPORTED
    assert raw_call(G, torch, "q8_0", "q4_0", k, v, qd, both) == 0                                           # (the same call with the flag runs)
    torch.cuda.synchronize()
