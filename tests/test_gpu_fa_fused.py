"""k_flash_attn_mfma (csrc/fattn_mfma.hip): the fused matrix-core FLASH_ATTN_EXT for prompt-sized calls and long windows.

Every device case is compared with the float64 restatement of ggml-cpu/ops.cpp:6690-6905 (q rounded to f16 once, tanh for the soft-cap) in the
metric of tests/test_gpu_glue_branches.py, |y - ref| <= c * sum_j p_j |v_j| per output, under that file's bound for probabilities rounded to
f16 on the way to the matrix cores (FA_BOUND["mfma"] = 5e-4).  The cases under `auto` are one per clause of the dispatch rule; the forced
cases (MI355Q_FA_FUSED=1) are the smallest shapes that reach each edge of the kernel: a single tile, partial tiles in both directions, head
sizes that are no multiple of 32, DK != DV, every register bucket (64 / 128 / 256), GQA and batch broadcast with ALiBi, a mask wider than the
window, strided K / V views, several row tiles and a long walk.  (`pytest -s` prints what each case measured.)
"""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

f32 = np.float32
FA_BOUND_MFMA = 5e-4                       # tests/test_gpu_glue_branches.py FA_BOUND["mfma"] (measured there at 1.3e-4)
FIXTURE = GOLDEN / "fa_fused_prefill_gqa_d128_kv256.npz"


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


def measured(name, value):
    print(f"MEASURED {name} {value:.3e}")


def alibi_slopes(H, max_bias):
    n2 = 1
    while 2 * n2 <= H:
        n2 *= 2
    m0, m1 = 2.0 ** (-max_bias / n2), 2.0 ** (-(max_bias / 2.0) / n2)
    return [(m0 ** (h + 1) if h < n2 else m1 ** (2 * (h - n2) + 1)) if max_bias > 0 else 1.0 for h in range(H)]


def fa_ref(q, k, v, mask, scale, max_bias=0.0, softcap=0.0):
    """float64 FLASH_ATTN_EXT with q rounded to f16; -> ref and sum_j p_j |v_j|, both [B, N, H, DV]"""
    B, H, N, _ = q.shape
    Bk, Hk, n_kv, DV = k.shape[0], k.shape[1], k.shape[2], v.shape[3]
    qh = q.astype(np.float16).astype(np.float64)
    out = np.zeros((B, N, H, DV)); mag = np.zeros_like(out)
    slopes = alibi_slopes(H, max_bias)
    for b in range(B):
        for h in range(H):
            kk = k[b // (B // Bk), h // (H // Hk)].astype(np.float64); vv = v[b // (B // Bk), h // (H // Hk)].astype(np.float64)
            s = (qh[b, h] @ kk.T) * (scale / softcap if softcap else scale)
            if softcap:
                s = softcap * np.tanh(s)
            if mask is not None:
                s = s + slopes[h] * mask[:N, :n_kv].astype(np.float64)
            s = s - s.max(axis=1, keepdims=True)
            p = np.exp(s)
            p /= p.sum(axis=1, keepdims=True)
            out[b, :, h] = p @ vv
            mag[b, :, h] = p @ np.abs(vv)
    return out, mag


def rel_err(y, ref, mag):
    assert np.isfinite(y).all()
    return float((np.abs(np.asarray(y, np.float64) - ref) / mag).max())


def fa_mask(rng, N, n_kv, max_bias=0.0, cols=None):
    """causal (the batch is the last N positions of the window) with random holes; `cols` > n_kv: a mask wider than the window"""
    mask = np.zeros((N, cols or n_kv), np.float16)
    for t in range(N):
        mask[t, n_kv - N + t + 1:] = -np.inf
    if n_kv > N:
        mask[:, rng.choice(n_kv - N, max(1, n_kv // 20), replace=False)] = -np.inf
    if max_bias > 0:
        mask[:, :n_kv] += (rng.standard_normal((N, n_kv)) * 0.1).astype(np.float16)
    return mask


def inputs(name, DK, DV, H, Hk, N, n_kv, B=1, Bk=1, max_bias=0.0, mask=True, mask_cols=None):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    q = rng.standard_normal((B, H, N, DK)).astype(f32)
    k = rng.standard_normal((Bk, Hk, n_kv, DK)).astype(np.float16)
    v = rng.standard_normal((Bk, Hk, n_kv, DV)).astype(np.float16)
    m = fa_mask(rng, N, n_kv, max_bias, mask_cols) if mask else None
    return q, k, v, m, float(f32(1.0 / np.sqrt(DK)))


def run_and_check(G, torch, name, q, k, v, m, scale, max_bias=0.0, softcap=0.0, split=True, kd=None, vd=None):
    kd = dev(torch, k) if kd is None else kd
    vd = dev(torch, v) if vd is None else vd
    qd, md = dev(torch, q), dev(torch, m) if m is not None else None
    assert G.op_flash_attn_ext_path(qd, kd, vd, md, softcap, split=split) == G.FA_PATH_FUSED, name
    y = G.op_flash_attn_ext(qd, kd, vd, md, scale, max_bias, softcap, split=split).cpu().numpy()
    ref, mag = fa_ref(q, k, v, m, scale, max_bias, softcap)
    e = rel_err(y, ref, mag)
    measured(f"fa-fused-{name}", e)
    assert e <= FA_BOUND_MFMA, (name, e)
    return y


# ------------------------------------------------------------------------------------------------ under `auto`: one case per clause of the rule
# (name, DK, DV, H, Hk, N, n_kv, softcap, split)
AUTO_CASES = [
    ("softcap-n33-kv1040", 128, 128, 4, 2, 33, 1040, 5.0, True),
    ("noworkspace-n16-kv1025", 128, 128, 2, 2, 16, 1025, 0.0, False),
    ("long-n16-kv36880", 64, 64, 2, 1, 16, 36880, 0.0, True),
    ("long-decode-n1-kv36880", 64, 64, 2, 1, 1, 36880, 0.0, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", AUTO_CASES, ids=[c[0] for c in AUTO_CASES])
def test_auto_cases(G, torch, monkeypatch, case):
    name, DK, DV, H, Hk, N, n_kv, softcap, split = case
    monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    q, k, v, m, scale = inputs(name, DK, DV, H, Hk, N, n_kv)
    run_and_check(G, torch, name, q, k, v, m, scale, softcap=softcap, split=split)


# ------------------------------------------------------------------------------------------------ forced: the edges of the kernel
# (name, N, n_kv, DK, DV, H, Hk, B, Bk, max_bias, mask, extra mask columns)
FORCED_CASES = [
    ("one-tile-nomask", 16, 16, 64, 64, 2, 2, 1, 1, 0.0, False, 0),
    ("partial-both-d80", 17, 80, 80, 80, 2, 2, 1, 1, 0.0, True, 0),
    ("gqa8-n150-kv336", 150, 336, 128, 128, 8, 2, 1, 1, 0.0, True, 0),
    ("d256", 64, 128, 256, 256, 2, 2, 1, 1, 0.0, True, 0),
    ("dk192-dv128", 32, 96, 192, 128, 2, 2, 1, 1, 0.0, True, 0),
    ("alibi12-b2-bk1", 32, 512, 128, 128, 12, 4, 2, 1, 8.0, True, 0),
    ("wide-mask", 40, 96, 64, 64, 2, 2, 1, 1, 0.0, True, 64),
    ("long-walk-kv4112", 64, 4112, 128, 128, 4, 2, 1, 1, 0.0, True, 0),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", FORCED_CASES, ids=[c[0] for c in FORCED_CASES])
def test_forced_cases(G, torch, monkeypatch, case):
    name, N, n_kv, DK, DV, H, Hk, B, Bk, max_bias, mask, extra = case
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    q, k, v, m, scale = inputs(name, DK, DV, H, Hk, N, n_kv, B, Bk, max_bias, mask, n_kv + extra if extra else None)
    run_and_check(G, torch, name, q, k, v, m, scale, max_bias)


@pytest.mark.gpu
def test_forced_strided_head_views(G, torch, monkeypatch):
    """K / V as head views of one [n_kv, Hk, D] cache buffer each (a position's heads lie side by side: nb[1] = Hk * D * 2, nb[2] = D * 2)"""
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    name, N, n_kv, D, H, Hk = "strided-views", 48, 256, 128, 4, 2
    q, k, v, m, scale = inputs(name, D, D, H, Hk, N, n_kv)
    kbuf = dev(torch, np.ascontiguousarray(k[0].transpose(1, 0, 2)))          # [n_kv, Hk, D]
    vbuf = dev(torch, np.ascontiguousarray(v[0].transpose(1, 0, 2)))
    kd, vd = kbuf.permute(1, 0, 2).unsqueeze(0), vbuf.permute(1, 0, 2).unsqueeze(0)
    assert not kd.is_contiguous() and kd.stride(2) == Hk * D
    run_and_check(G, torch, name, q, k, v, m, scale, kd=kd, vd=vd)


# ------------------------------------------------------------------------------------------------ masked cache rows never reach the output
@pytest.mark.gpu
@pytest.mark.parametrize("forced", [True, False], ids=["forced-n150-kv336", "auto-softcap-n33-kv1040"])
def test_masked_rows_do_not_matter(G, torch, monkeypatch, forced):
    """Every K / V row that is masked for ALL query rows once zero and once +-65504 (the largest finite f16): the outputs are the same bits."""
    if forced:
        monkeypatch.setenv("MI355Q_FA_FUSED", "1")
        name, (DK, DV, H, Hk, N, n_kv), softcap = "masked-forced", (128, 128, 8, 2, 150, 336), 0.0
    else:
        monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
        name, (DK, DV, H, Hk, N, n_kv), softcap = "masked-auto", (128, 128, 4, 2, 33, 1040), 5.0
    q, k, v, m, scale = inputs(name, DK, DV, H, Hk, N, n_kv)
    dead = np.isinf(m[:, :n_kv]).all(axis=0)
    assert dead.any()
    outs = []
    for fill in (0.0, 65504.0):
        k2, v2 = k.copy(), v.copy()
        k2[:, :, dead] = np.float16(fill); v2[:, :, dead] = np.float16(-fill)
        k2[:, :, dead, ::2] *= np.float16(-1)
        qd, kd, vd, md = dev(torch, q), dev(torch, k2), dev(torch, v2), dev(torch, m)
        assert G.op_flash_attn_ext_path(qd, kd, vd, md, softcap) == G.FA_PATH_FUSED
        outs.append(G.op_flash_attn_ext(qd, kd, vd, md, scale, 0.0, softcap).cpu().numpy())
    assert np.isfinite(outs[0]).all()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


@pytest.mark.gpu
def test_fully_masked_query_row_is_harmless(G, torch, monkeypatch):
    """A query row with every position masked has no defined value; it must not disturb its neighbours (or fault)."""
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    q, k, v, m, scale = inputs("dead-row", 64, 64, 2, 2, 20, 100)
    m[5, :] = -np.inf
    y = G.op_flash_attn_ext(dev(torch, q), dev(torch, k), dev(torch, v), dev(torch, m), scale).cpu().numpy()
    ref, mag = fa_ref(np.delete(q, 5, axis=2), k, v, np.delete(m, 5, axis=0), scale)
    e = rel_err(np.delete(y, 5, axis=1), ref, mag)
    assert e <= FA_BOUND_MFMA, e


# ------------------------------------------------------------------------------------------------ the reference CPU backend's own output
def nmse(y, want):
    y = np.asarray(y, np.float64); want = np.asarray(want, np.float64)
    return float(((y - want) ** 2).sum() / (want ** 2).sum())


def test_fixture_loads_and_is_the_cpu():
    """tests/golden/make_fa_fused_golden.py: the fixture is the CPU's FLASH_ATTN_EXT (its bit-exact restatement reproduces it) and the float64
    restatement lies within the CPU's F16-accumulator distance of it: tests/test_gpu_glue_branches.py FA_BOUND["seq"] = 8e-3 in the metric
    |y - ref| <= c * sum_j p_j |v_j|, the bound of the kernel that reproduces the CPU's sequential F16 accumulation bit for bit."""
    from oracle import glue
    g = np.load(FIXTURE, allow_pickle=False)
    q = g["q"].astype(f32)
    assert q.shape == (1, 4, 48, 128) and g["k"].shape == (1, 2, 256, 128) and g["v"].shape == (1, 2, 256, 128) and g["y"].shape == (1, 48, 4, 128)
    assert FIXTURE.stat().st_size < 500_000
    want = glue.flash_attn_ext(q, g["k"], g["v"], g["mask"], float(g["scale"]))
    assert np.array_equal(want.view(np.uint32), g["y"].view(np.uint32))
    ref, mag = fa_ref(q, g["k"], g["v"], g["mask"], float(g["scale"]))
    e = rel_err(g["y"], ref, mag)
    measured("fa-fused-fixture-cpu-vs-f64", e)
    assert e <= 8e-3, e


@pytest.mark.gpu
def test_fused_is_as_close_to_the_cpu_as_three_step(G, torch, monkeypatch):
    """NMSE against the reference CPU backend's output on the same inputs: the three-step matrix-core path (MI355Q_FA_FUSED=0) is the yardstick.
    Both round P to f16 and accumulate in f32; they differ in summation order and the per-tile rescale, for which a factor of 2 is the slack."""
    g = np.load(FIXTURE, allow_pickle=False)
    qd, kd, vd, md = dev(torch, g["q"].astype(f32)), dev(torch, g["k"]), dev(torch, g["v"]), dev(torch, g["mask"])
    got = {}
    for mode, want_path in (("0", G.FA_PATH_MFMA3), ("1", G.FA_PATH_FUSED)):
        monkeypatch.setenv("MI355Q_FA_FUSED", mode)
        assert G.op_flash_attn_ext_path(qd, kd, vd, md) == want_path
        got[mode] = nmse(G.op_flash_attn_ext(qd, kd, vd, md, float(g["scale"])).cpu().numpy(), g["y"])
    measured("fa-fused-nmse-three-step", got["0"]); measured("fa-fused-nmse-fused", got["1"])
    assert got["1"] <= 2 * got["0"], got


# ------------------------------------------------------------------------------------------------ through the plugin
def _harness():
    import oracle
    v = oracle.best_ref_variant()
    p = ROOT / "oracle" / "_ref" / v / "test-backend-ops" if v else None
    return p if p is not None and p.exists() else None


PLUGIN = ROOT / "llama.cpp.dsp_amd" / "lib" / "libggml-mi355.so"


@pytest.mark.gpu
@pytest.mark.skipif(not PLUGIN.exists() or _harness() is None, reason="plugin or oracle/_ref not built")
def test_reference_harness_flash_attn_ext_forced_fused():
    """The reference's own test-backend-ops -o FLASH_ATTN_EXT through the plugin (tests/test_plugin.py's invocation) with every call the fused
    kernel can take sent to it: each case the plugin accepts passes the harness' NMSE check against the ggml CPU backend."""
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), MI355Q_FA_FUSED="1")
    r = subprocess.run([str(_harness()), "test", "-b", "MI355_0", "-o", "FLASH_ATTN_EXT"], env=env, capture_output=True, text=True, timeout=900)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    m = re.search(r"(\d+)/(\d+) tests passed", r.stdout)
    assert m and m.group(1) == m.group(2), tail
    assert "FAIL" not in r.stdout
    cases = [l for l in r.stdout.splitlines() if l.lstrip().startswith("FLASH_ATTN_EXT(")]
    ran = [l for l in cases if "OK" in l]
    print(f"FLASH_ATTN_EXT, fused forced: {len(ran)} of {len(cases)} cases ran on MI355_0 and passed")
    assert len(ran) >= 1, tail
