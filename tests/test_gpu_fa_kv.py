"""k_flash_attn_mfma on a quantized or bf16 cache's own rows (MI355Q_FA_KV_DIRECT, MI355Q_FA_PATH_FUSED_KV; csrc/fattn_mfma.cuh).

Block types (q8_0, q4_0, q4_1, q5_0, q5_1, iq4_nl): the loader decodes a block to f16 on the way into LDS with the arithmetic of
k_dequant_cache_f16, so the output must equal, BIT FOR BIT, the f16 fused kernel's on the f16 copy of the cache -- the copy is built here in numpy as
float16(float32(q) * float32(d) [+ float32(m)]), one f32 rounding per operation.  In the window the row kernel refuses (n_kv > 8192) decode calls are
also held against the float64 restatement of tests/test_gpu_fa_fused.py under its bound.

bf16: against a float64 restatement with q rounded to bf16 and the bf16 K / V taken exactly, in the same metric |y - ref| <= c * sum_j p_j |v_j| with
c = 2^-8: rounding P to bf16 moves each term by at most 2^-9 p_j |v_j|, and the factor 2 covers the f32 exp and the f32 accumulation.
(`pytest -s` prints what each case measured.)
"""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import kvq_ref
from test_gpu_fa_fused import FA_BOUND_MFMA, PLUGIN, G, _harness, alibi_slopes, dev, fa_mask, fa_ref, measured, rel_err, torch  # noqa: F401 (fixtures)

f32 = np.float32
KV_TYPES = ["q8_0", "q4_0", "q4_1", "q5_0", "q5_1", "iq4_nl"]
BF16_BOUND = 2.0 ** -8
KVALUES = kvq_ref.KVALUES_IQ4NL


# ------------------------------------------------------------------------------------------------ caches
def f16_copy(kv, blk):
    """uint8 [..., nb * BB] -> float16 [..., 32 nb]: what k_dequant_cache_f16 writes (dequantize_row_<type>, then one rounding to f16)"""
    if kv in kvq_ref.TYPES:
        y = kvq_ref.dequantize(kv, blk)
    else:
        bb = {"q8_0": 34, "q4_0": 18}[kv]
        b = np.ascontiguousarray(blk).reshape(blk.shape[:-1] + (blk.shape[-1] // bb, bb))
        d = np.ascontiguousarray(b[..., 0:2]).view("<f2")[..., 0].astype(f32)
        if kv == "q8_0":
            q = b[..., 2:34].view(np.int8).astype(f32)
        else:
            qs = b[..., 2:18].astype(np.int32)
            q = (np.concatenate([qs & 15, qs >> 4], axis=-1) - 8).astype(f32)
        y = (q * d[..., None]).astype(f32).reshape(blk.shape[:-1] + (-1,))
    with np.errstate(over="ignore"):
        return y.astype(np.float16)


_CACHE = {}


def quant_case(G, torch, kv, name, DK, DV, H, Hk, N, n_kv, mask=True, first_sees=None):
    """seeded normals; K / V quantized by the device's own op_cpy -> (q, k blocks, v blocks, their f16 copies, mask, scale), computed once per case.
    first_sees: query row t sees no position from first_sees + t on (an earlier causal edge than fa_mask's)"""
    key = (kv, name, DK, DV, H, Hk, N, n_kv, mask, first_sees)
    if key not in _CACHE:
        rng = np.random.default_rng(zlib.crc32(f"{kv}-{name}".encode()))
        q = rng.standard_normal((1, H, N, DK)).astype(f32)
        kf = rng.standard_normal((1, Hk, n_kv, DK)).astype(f32)
        vf = rng.standard_normal((1, Hk, n_kv, DV)).astype(f32)
        bb = G.KV_BLOCK[kv][0]
        kb = torch.zeros((1, Hk, n_kv, DK // 32 * bb), dtype=torch.uint8, device="cuda")
        vb = torch.zeros((1, Hk, n_kv, DV // 32 * bb), dtype=torch.uint8, device="cuda")
        G.op_cpy(dev(torch, kf), kb, kv=kv); G.op_cpy(dev(torch, vf), vb, kv=kv)
        kb, vb = kb.cpu().numpy(), vb.cpu().numpy()
        m = fa_mask(rng, N, n_kv) if mask else None
        if first_sees is not None:
            for t in range(N):
                m[t, first_sees + t:] = -np.inf
        _CACHE[key] = (q, kb, vb, f16_copy(kv, kb), f16_copy(kv, vb), m, float(f32(1.0 / np.sqrt(DK))))
    return _CACHE[key]


def llama_layout(torch, blocks, extra_rows=0, fill=0):
    """[1, Hk, n_kv, row_bytes] blocks -> the head views of ONE [n_kv + extra_rows, Hk, row_bytes] cache buffer: nb[1] = Hk * row_bytes,
    nb[2] = row_bytes (a position's heads lie side by side); the extra rows behind the window hold `fill` bytes"""
    _, Hk, n_kv, rb = blocks.shape
    buf = np.full((n_kv + extra_rows, Hk, rb), fill, np.uint8)
    buf[:n_kv] = blocks[0].transpose(1, 0, 2)
    t = dev(torch, buf)
    view = t[:n_kv].permute(1, 0, 2).unsqueeze(0)
    assert view.stride(2) == Hk * rb and view.stride(1) == rb
    return view


def case_n70(G, torch, kv):
    """N = 70 over n_kv = 200, 4 heads over 2 of size 128: partial tiles in both directions; row t sees positions < 128 + t, so the last tile
    (192 .. 199) is dead for the first 64 query rows and live, and partial, for the other six"""
    case = quant_case(G, torch, kv, "n70-kv200", 128, 128, 4, 2, 70, 200, first_sees=128)
    m = case[5]
    assert np.isinf(m[:64, 192:200]).all() and not np.isinf(m[64:, 192:200]).all()
    return case


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def direct_vs_f16_copy(G, torch, monkeypatch, kv, case, forced=True, layout=False, split=True):
    q, kb, vb, k16, v16, m, scale = case
    if forced:
        monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    else:
        monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    qd, md = dev(torch, q), dev(torch, m) if m is not None else None
    kd, vd = (llama_layout(torch, kb), llama_layout(torch, vb)) if layout else (dev(torch, kb), dev(torch, vb))
    assert G.op_flash_attn_ext_path(qd, kd, vd, md, kv=kv, split=split, kv_direct=True) == G.FA_PATH_FUSED_KV
    y = G.op_flash_attn_ext(qd, kd, vd, md, scale, kv=kv, split=split, kv_direct=True).cpu().numpy()
    k16d, v16d = dev(torch, k16), dev(torch, v16)
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")                                 # the yardstick: the f16 fused kernel on the f16 copy
    assert G.op_flash_attn_ext_path(qd, k16d, v16d, md) == G.FA_PATH_FUSED
    want = G.op_flash_attn_ext(qd, k16d, v16d, md, scale).cpu().numpy()
    assert np.isfinite(want).all()
    assert np.array_equal(bits(y), bits(want)), (kv, float(np.abs(y - want).max()))
    return y


# ------------------------------------------------------------------------------------------------ block types, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("kv", KV_TYPES)
def test_one_full_tile(G, torch, monkeypatch, kv):
    direct_vs_f16_copy(G, torch, monkeypatch, kv, quant_case(G, torch, kv, "one-tile", 64, 64, 2, 1, 16, 64, mask=False))


@pytest.mark.gpu
@pytest.mark.parametrize("kv", KV_TYPES)
def test_partial_tiles_tile_skip_llama_layout(G, torch, monkeypatch, kv):
    """the cache in the llama layout: rows of a head 8-byte (q8_0 at head size 128: 136 bytes) or 2-byte aligned"""
    direct_vs_f16_copy(G, torch, monkeypatch, kv, case_n70(G, torch, kv), layout=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kv", KV_TYPES)
def test_head_size_32_two_byte_aligned_blocks(G, torch, monkeypatch, kv):
    """three heads of ONE block each side by side: a head's row starts at h * 18 / 20 / 22 / 24 / 34 bytes"""
    direct_vs_f16_copy(G, torch, monkeypatch, kv, quant_case(G, torch, kv, "d32-h3", 32, 32, 3, 3, 16, 96), layout=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kv", ["q8_0", "q5_1"])
def test_largest_k_bucket_dk_ne_dv(G, torch, monkeypatch, kv):
    direct_vs_f16_copy(G, torch, monkeypatch, kv, quant_case(G, torch, kv, "dk256-dv64", 256, 64, 2, 2, 16, 128))


@pytest.mark.gpu
@pytest.mark.parametrize("kv", KV_TYPES)
def test_auto_prompt_in_the_new_window(G, torch, monkeypatch, kv):
    """n_kv = 8256 (129 tiles), N = 16, under `auto`: rule (d).  The call passes no workspace: with one, a quantized prompt keeps its f16 copy there
    (the measured decision of DESIGN.md 5.7f); without the flag this call is refused."""
    direct_vs_f16_copy(G, torch, monkeypatch, kv, quant_case(G, torch, kv, "n16-kv8256", 64, 64, 2, 1, 16, 8256), forced=False, split=False)


@pytest.mark.gpu
def test_auto_decode_beyond_the_row_kernels(G, torch, monkeypatch):
    """q8_0, N = 1, n_kv = 36880 under `auto`: the f16 call takes the fused kernel there by rule (c)"""
    direct_vs_f16_copy(G, torch, monkeypatch, "q8_0", quant_case(G, torch, "q8_0", "n1-kv36880", 64, 64, 2, 1, 1, 36880), forced=False)


# ------------------------------------------------------------------------------------------------ decode in the window the row kernel refuses
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 15])
@pytest.mark.parametrize("kv", KV_TYPES)
def test_decode_in_the_new_window(G, torch, monkeypatch, kv, N):
    monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    q, kb, vb, k16, v16, m, scale = quant_case(G, torch, kv, f"decode-n{N}", 64, 64, 2, 1, N, 8256)
    qd, kd, vd, md = dev(torch, q), dev(torch, kb), dev(torch, vb), dev(torch, m)
    assert G.op_flash_attn_ext_path(qd, kd, vd, md, kv=kv, kv_direct=True) == G.FA_PATH_FUSED_KV
    y = G.op_flash_attn_ext(qd, kd, vd, md, scale, kv=kv, kv_direct=True).cpu().numpy()
    ref, mag = fa_ref(q, k16, v16, m, scale)
    e = rel_err(y, ref, mag)
    measured(f"fa-kv-{kv}-decode-n{N}-kv8256", e)
    assert e <= FA_BOUND_MFMA, (kv, N, e)


@pytest.mark.gpu
def test_old_entry_point_still_refuses(G, torch, monkeypatch):
    monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    q, kb, vb, _, _, m, scale = quant_case(G, torch, "q8_0", "decode-n1", 64, 64, 2, 1, 1, 8256)
    qd, kd, vd, md = dev(torch, q), dev(torch, kb), dev(torch, vb), dev(torch, m)
    assert G.op_flash_attn_ext_path(qd, kd, vd, md, kv="q8_0") == G.ERR_UNSUPPORTED
    with pytest.raises(G.Mi355qError):
        G.op_flash_attn_ext(qd, kd, vd, md, scale, kv="q8_0")


# ------------------------------------------------------------------------------------------------ rows outside the window, masked rows
def bf16_case(torch, name, DK, DV, H, Hk, N, n_kv, mask=True, v_scale=1.0):
    """-> (q f32, k, v as torch.bfloat16 CPU tensors [1, Hk, n_kv, D], mask, scale)"""
    rng = np.random.default_rng(zlib.crc32(f"bf16-{name}".encode()))
    q = rng.standard_normal((1, H, N, DK)).astype(f32)
    k = torch.from_numpy(rng.standard_normal((1, Hk, n_kv, DK)).astype(f32)).to(torch.bfloat16)
    v = torch.from_numpy((rng.standard_normal((1, Hk, n_kv, DV)) * v_scale).astype(f32)).to(torch.bfloat16)
    m = fa_mask(rng, N, n_kv) if mask else None
    return q, k, v, m, float(f32(1.0 / np.sqrt(DK)))


@pytest.mark.gpu
@pytest.mark.parametrize("kv", KV_TYPES + ["bf16"])
def test_rows_behind_the_window_are_never_read(G, torch, monkeypatch, kv):
    """the cache buffer is 64 rows longer than n_kv = 200: those rows once 0xFF bytes (NaN scales, NaN bf16), once zeros -- the same bits"""
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    outs = []
    if kv == "bf16":
        q, k, v, m, scale = bf16_case(torch, "tail", 128, 128, 4, 2, 70, 200)
        kb, vb = k.view(torch.int16).numpy().view(np.uint8), v.view(torch.int16).numpy().view(np.uint8)
    else:
        q, kb, vb, _, _, m, scale = case_n70(G, torch, kv)
    for fill in (0xFF, 0x00):
        kd, vd = llama_layout(torch, kb, 64, fill), llama_layout(torch, vb, 64, fill)
        if kv == "bf16":
            kd, vd = kd.view(torch.bfloat16), vd.view(torch.bfloat16)
        qd, md = dev(torch, q), dev(torch, m)
        assert G.op_flash_attn_ext_path(qd, kd, vd, md, kv=kv if kv != "bf16" else "q8_0", kv_direct=True) == G.FA_PATH_FUSED_KV
        outs.append(G.op_flash_attn_ext(qd, kd, vd, md, scale, kv=kv if kv != "bf16" else "q8_0", kv_direct=True).cpu().numpy())
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("kv", KV_TYPES)
def test_masked_rows_do_not_matter(G, torch, monkeypatch, kv):
    """Every K / V position masked for ALL query rows once with the scale 256 (values up to 127 * 256: large, finite in f16), once as zero blocks"""
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    q, kb, vb, _, _, m, scale = quant_case(G, torch, kv, "masked", 128, 128, 8, 2, 150, 336)
    dead = np.isinf(m[:, :336]).all(axis=0)
    assert dead.any()
    bb = G.KV_BLOCK[kv][0]
    outs = []
    for big in (True, False):
        k2, v2 = kb.copy(), vb.copy()
        for c in (k2, v2):
            blk = c.reshape(c.shape[:-1] + (-1, bb))
            if big:
                blk[:, :, dead, :, 0:2] = np.array([256.0], "<f2").view(np.uint8)
            else:
                blk[:, :, dead] = 0
        qd, kd, vd, md = dev(torch, q), dev(torch, k2), dev(torch, v2), dev(torch, m)
        outs.append(G.op_flash_attn_ext(qd, kd, vd, md, scale, kv=kv, kv_direct=True).cpu().numpy())
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("kv", ["q8_0", "bf16"])
def test_fully_masked_query_row_gives_zeros(G, torch, monkeypatch, kv):
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    if kv == "bf16":
        q, k, v, m, scale = bf16_case(torch, "dead-row", 64, 64, 2, 2, 20, 100)
        kd, vd = k.cuda(), v.cuda()
    else:
        q, kb, vb, _, _, m, scale = quant_case(G, torch, kv, "dead-row", 64, 64, 2, 2, 20, 100)
        kd, vd = dev(torch, kb), dev(torch, vb)
    m = m.copy(); m[5, :] = -np.inf
    y = G.op_flash_attn_ext(dev(torch, q), kd, vd, dev(torch, m), scale, kv="q8_0", kv_direct=True).cpu().numpy()
    assert np.isfinite(y).all() and not y[:, 5].any() and y[:, 4].any()


# ------------------------------------------------------------------------------------------------ bf16
def fa_ref_bf16(torch, q, k, v, mask, scale, softcap=0.0):
    """float64 FLASH_ATTN_EXT with q rounded to bf16 and the bf16 K / V exactly; -> ref and sum_j p_j |v_j|, both [B, N, H, DV]"""
    qr = torch.from_numpy(q).to(torch.bfloat16).to(torch.float64).numpy()
    kk, vv = k.to(torch.float64).numpy(), v.to(torch.float64).numpy()
    B, H, N, _ = q.shape
    Hk, n_kv, DV = kk.shape[1], kk.shape[2], vv.shape[3]
    out = np.zeros((B, N, H, DV)); mag = np.zeros_like(out)
    for h in range(H):
        s = (qr[0, h] @ kk[0, h // (H // Hk)].T) * (scale / softcap if softcap else scale)
        if softcap:
            s = softcap * np.tanh(s)
        if mask is not None:
            s = s + mask[:N, :n_kv].astype(np.float64)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        out[0, :, h] = p @ vv[0, h // (H // Hk)]
        mag[0, :, h] = p @ np.abs(vv[0, h // (H // Hk)])
    return out, mag


# (name, DK, DV, H, Hk, N, n_kv, mask, softcap, forced, V magnitude, workspace)
BF16_CASES = [
    ("one-tile-nomask", 64, 64, 2, 1, 16, 64, False, 0.0, True, 1.0, True),
    ("n70-kv200", 128, 128, 4, 2, 70, 200, True, 0.0, True, 1.0, True),
    ("dk256-dv64", 256, 64, 2, 2, 16, 128, True, 0.0, True, 1.0, True),
    ("d80-16-tail", 80, 80, 4, 1, 16, 80, True, 0.0, True, 1.0, True),
    ("softcap-n33-kv1040", 128, 128, 4, 2, 33, 1040, True, 5.0, False, 1.0, True),
    ("auto-n1-kv8256", 64, 64, 2, 1, 1, 8256, True, 0.0, False, 1.0, True),
    ("auto-n16-kv8256", 64, 64, 2, 1, 16, 8256, True, 0.0, False, 1.0, False),    # (with a workspace its 1 MiB of scores keep the three-step path: rule (b))
    ("v-1e6", 128, 128, 4, 2, 70, 200, True, 0.0, True, 1e6, True),               # beyond f16's range
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_bf16(G, torch, monkeypatch, case):
    name, DK, DV, H, Hk, N, n_kv, mask, softcap, forced, v_scale, split = case
    if forced:
        monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    else:
        monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    q, k, v, m, scale = bf16_case(torch, name, DK, DV, H, Hk, N, n_kv, mask, v_scale)
    qd, kd, vd, md = dev(torch, q), k.cuda(), v.cuda(), dev(torch, m) if m is not None else None
    assert G.op_flash_attn_ext_path(qd, kd, vd, md, softcap, split=split, kv_direct=True) == G.FA_PATH_FUSED_KV, name
    y = G.op_flash_attn_ext(qd, kd, vd, md, scale, 0.0, softcap, split=split, kv_direct=True).cpu().numpy()
    ref, mag = fa_ref_bf16(torch, q, k, v, m, scale, softcap)
    e = rel_err(y, ref, mag)
    measured(f"fa-kv-bf16-{name}", e)
    assert e <= BF16_BOUND, (name, e)


# ------------------------------------------------------------------------------------------------ through the plugin
@pytest.mark.gpu
@pytest.mark.skipif(not PLUGIN.exists() or _harness() is None, reason="plugin or oracle/_ref not built")
def test_reference_harness_flash_attn_ext_kv_direct():
    """The reference's own test-backend-ops -o FLASH_ATTN_EXT through the plugin with MI355Q_FA_FUSED=1 (tests/test_gpu_fa_fused.py's invocation): the
    plugin's flag is on by default, so the quantized and bf16 cases with >= 16 rows take the direct form; every case passes.  A second run with
    MI355_FA_KV_DIRECT=0 is the plugin before the flag: it passes, and the same number of cases ran on the device."""
    counts = {}
    for direct in ("1", "0"):
        env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), MI355Q_FA_FUSED="1", MI355_FA_KV_DIRECT=direct)
        r = subprocess.run([str(_harness()), "test", "-b", "MI355_0", "-o", "FLASH_ATTN_EXT"], env=env, capture_output=True, text=True, timeout=900)
        tail = r.stdout[-3000:] + r.stderr[-2000:]
        assert r.returncode == 0, tail
        mt = re.search(r"(\d+)/(\d+) tests passed", r.stdout)
        assert mt and mt.group(1) == mt.group(2), tail
        assert "FAIL" not in r.stdout
        cases = [l for l in r.stdout.splitlines() if l.lstrip().startswith("FLASH_ATTN_EXT(")]
        counts[direct] = (len([l for l in cases if "OK" in l]), len(cases))
        print(f"FLASH_ATTN_EXT, fused forced, MI355_FA_KV_DIRECT={direct}: {counts[direct][0]} of {counts[direct][1]} cases ran on MI355_0 and passed")
    assert counts["1"][0] >= 1 and counts["1"] == counts["0"], counts
