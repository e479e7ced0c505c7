"""mi355q_op_flash_attn_ext_path2 with MI355Q_FA_KV_DIRECT: which calls the fused kernel takes on a quantized or bf16 cache's own rows, asked from
descriptors alone (no device, fake addresses).  DESIGN.md 5.7f, rules (d) and (e).

Without the flag, and with it under MI355Q_FA_FUSED=0, every input of tests/test_fa_path_cpu.py answers as mi355q_op_flash_attn_ext_path does.
With it, a direct-eligible call answers FUSED_KV above 8192 positions (d) and, with >= 16 query rows, where it has neither the f16 copy nor the
three-step path (e); MI355Q_FA_FUSED=1 sends every direct-eligible call with >= 16 rows or a window above 8192 there.  A FUSED_KV answer does not
depend on the workspace.
"""
import pytest

import ggml_mi355 as G
from test_fa_path_cpu import BF16, F16, F32, FA_CASES, FA_EXT_CFGS
from test_fa_path_cpu import path as path_old


def path2(DK, DV, H, Hk, N, n_kv, B=1, Bk=1, softcap=0.0, split=True, kv_type=F16, mask_rows=None, mask_cols=None, k_addr=0x10000,
          workspace_bytes=None, mask=True, kv_direct=True):
    q = G.tensor_desc(F32, [DK, N, H, B], data=0x20000)
    k = G.tensor_desc(kv_type, [DK, n_kv, Hk, Bk], data=k_addr)
    v = G.tensor_desc(kv_type, [DV, n_kv, Hk, Bk], data=0x30000)
    m = G.tensor_desc(F16, [mask_cols or n_kv, mask_rows or N], data=0x40000) if mask else None
    return G.op_flash_attn_ext_path(q, k, v, m, softcap, split=split, workspace_bytes=workspace_bytes, kv_direct=kv_direct)


def path2_flags0(DK, DV, H, Hk, N, n_kv, B=1, Bk=1, softcap=0.0, split=True, kv_type=F16, mask_rows=None, k_addr=0x10000):
    """mi355q_op_flash_attn_ext_path2(..., flags = 0) itself (the mirror's kv_direct=False calls the old symbol)"""
    import ctypes as C
    q = G.tensor_desc(F32, [DK, N, H, B], data=0x20000)
    k = G.tensor_desc(kv_type, [DK, n_kv, Hk, Bk], data=k_addr)
    v = G.tensor_desc(kv_type, [DV, n_kv, Hk, Bk], data=0x30000)
    m = G.tensor_desc(F16, [n_kv, mask_rows or N], data=0x40000)
    out = G.tensor_desc(F32, [DV, H, N, B])
    ws = int(G.lib().mi355q_op_flash_attn_ext_workspace(DV, N, H, B, n_kv)) if split else 0
    return int(G.lib().mi355q_op_flash_attn_ext_path2(C.byref(q), C.byref(k), C.byref(v), C.byref(m), C.byref(out), softcap, 1 if ws > 0 else 0, ws, 0))


@pytest.fixture
def auto(monkeypatch):
    monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    monkeypatch.delenv("MI355Q_FA_EXACT", raising=False)


# test_fa_path_cpu.py test_other_caches_as_today, its literal calls
OTHER_CACHES = [
    ((128, 128, 4, 2, 1, 9000), dict(kv_type=BF16)), ((128, 128, 4, 2, 1, 8192), dict(kv_type=BF16)),
    ((128, 128, 4, 2, 32, 9008), dict(kv_type=BF16)), ((128, 128, 4, 2, 32, 9008), dict(kv_type=BF16, softcap=5.0)),
    ((128, 128, 4, 2, 1, 256), dict(kv_type=G.Q8_0)), ((128, 128, 4, 2, 1, 9000), dict(kv_type=G.Q8_0)),
    ((128, 128, 4, 2, 48, 256), dict(kv_type=G.Q8_0)), ((128, 128, 4, 2, 48, 256), dict(kv_type=G.Q8_0, softcap=5.0)),
]


def every_old_input():
    for name, DK, DV, H, Hk, N, B, Bk, n_kv, _, split in FA_CASES:
        yield (DK, DV, H, Hk, N, n_kv, B, Bk), dict(split=split)
    for (DK, DV, H, Hk, N, n_kv, _, softcap), _want in FA_EXT_CFGS:
        yield (DK, DV, H, Hk, N, n_kv), dict(softcap=softcap, mask_rows=32 * ((N + 31) // 32))
    yield from OTHER_CACHES


def test_flag_off_is_the_old_entry_point(auto):
    for a, kw in every_old_input():
        want = path_old(*a, **kw)
        assert path2_flags0(*a, **kw) == want, (a, kw)
        assert path2(*a, kv_direct=False, **kw) == want, (a, kw)


def test_flag_is_ignored_when_fused_is_off(monkeypatch):
    monkeypatch.setenv("MI355Q_FA_FUSED", "0")
    for a, kw in every_old_input():
        assert path2(*a, **kw) == path_old(*a, **kw), (a, kw)
    assert path2(128, 128, 4, 2, 1, 9000, kv_type=G.Q8_0) == G.ERR_UNSUPPORTED
    assert path2(128, 128, 4, 2, 48, 256, kv_type=G.Q8_0, softcap=5.0) == G.FA_PATH_KV_ROW


def test_flag_leaves_f16_caches_alone(auto):
    for name, DK, DV, H, Hk, N, B, Bk, n_kv, _, split in FA_CASES:
        assert path2(DK, DV, H, Hk, N, n_kv, B, Bk, split=split) == path_old(DK, DV, H, Hk, N, n_kv, B, Bk, split=split), name
    assert path2(64, 64, 2, 1, 1, 36880) == G.FA_PATH_FUSED


# (DK, DV, H, Hk, N, n_kv, cache, extra, expected)
AUTO_TABLE = [
    (128, 128, 4, 2, 1, 9000, G.Q8_0, {}, "FUSED_KV"),
    (128, 128, 4, 2, 1, 9000, BF16, {}, "FUSED_KV"),
    (128, 128, 4, 2, 1, 8192, G.Q8_0, {}, "KV_ROW"),
    (128, 128, 4, 2, 1, 8192, BF16, {}, "KV_ROW"),
    (128, 128, 4, 2, 32, 9008, BF16, dict(softcap=5.0), "FUSED_KV"),
    (128, 128, 4, 2, 32, 9008, BF16, {}, "MFMA3"),
    (128, 128, 4, 2, 48, 256, G.Q8_0, {}, "MFMA3"),
    (128, 128, 4, 2, 48, 256, G.Q8_0, dict(softcap=5.0), "FUSED_KV"),
    (128, 128, 4, 2, 48, 256, G.Q8_0, dict(split=False), "FUSED_KV"),
    (128, 128, 32, 8, 512, 16384, BF16, {}, "FUSED_KV"),                       # scores 512 * 16384 * 32 * 4 = 1 GiB > 256 MiB: rule (b)
]
WANT = {"FUSED_KV": G.FA_PATH_FUSED_KV, "KV_ROW": G.FA_PATH_KV_ROW, "MFMA3": G.FA_PATH_MFMA3}


@pytest.mark.parametrize("row", AUTO_TABLE, ids=[f"{r[6]}-n{r[4]}-kv{r[5]}-{'-'.join(r[7]) or 'plain'}" for r in AUTO_TABLE])
def test_auto_table(auto, row):
    DK, DV, H, Hk, N, n_kv, kvt, extra, want = row
    assert path2(DK, DV, H, Hk, N, n_kv, kv_type=kvt, **extra) == WANT[want]
    if want == "FUSED_KV":                                                     # consistency: the answer does not depend on the workspace
        assert path2(DK, DV, H, Hk, N, n_kv, kv_type=kvt, **dict(extra, split=False)) == G.FA_PATH_FUSED_KV


def test_every_block_type_and_bf16_tails(auto):
    for kvt in (G.Q8_0, G.Q4_0, G.Q4_1, G.Q5_0, G.Q5_1, G.IQ4_NL):
        assert path2(64, 64, 2, 1, 1, 8256, kv_type=kvt) == G.FA_PATH_FUSED_KV
        assert path2(64, 64, 2, 1, 15, 8256, kv_type=kvt) == G.FA_PATH_FUSED_KV
        assert path2(64, 64, 2, 1, 1, 36880, kv_type=kvt) == G.FA_PATH_FUSED_KV        # beyond the f16 row kernels' window too
        assert path2(64, 64, 2, 1, 15, 8192, kv_type=kvt) == G.FA_PATH_KV_ROW          # N < 16 at n_kv <= 8192 keeps the CPU-exact row kernel
    assert path2(80, 80, 4, 1, 16, 80, kv_type=BF16, split=False) == G.FA_PATH_FUSED_KV  # the 16-tail; no workspace
    assert path2(128, 128, 4, 2, 16, 1025, kv_type=BF16) == G.FA_PATH_FUSED_KV           # n_kv % 16 != 0: no three-step form
    assert path2(128, 128, 2, 2, 16, 1040, kv_type=BF16, mask_cols=1104) == G.FA_PATH_FUSED_KV   # a wide mask stride


def test_not_direct_eligible_answers_as_without_the_flag(auto):
    assert path2(128, 128, 4, 2, 1, 9000, kv_type=G.Q8_0, k_addr=0x10001) == G.ERR_UNSUPPORTED      # an odd address
    assert path2(48, 48, 4, 2, 1, 256, kv_type=G.Q8_0) == path_old(48, 48, 4, 2, 1, 256, kv_type=G.Q8_0)
    assert path2(48, 48, 4, 2, 48, 256, kv_type=G.Q8_0, softcap=5.0) == path_old(48, 48, 4, 2, 48, 256, kv_type=G.Q8_0, softcap=5.0)
    assert path2(72, 72, 4, 2, 1, 9000, kv_type=BF16) == G.ERR_UNSUPPORTED
    assert path2(128, 128, 4, 2, 1, 9000, kv_type=BF16, k_addr=0x10008) == G.ERR_UNSUPPORTED        # bf16 rows need 16 bytes


def test_long_quantized_prompt_with_a_workspace(auto):
    """Rule (d) for a quantized prompt above 8192 positions that HAS the workspace of the f16 copy: the copy followed by the f16 rule, decided by the
    measurement in profiles/fa_kv_direct.md ("Rule (d)": q8_0 at N = 512, n_kv = 16384: copy + fused 1093.4 us, direct 1315.6 us, spreads below
    2 %; 32768: 2098.8 against 2586.7 us).  Without the workspace the call is direct -- without the flag it is one workgroup per query row or refused."""
    assert path2(128, 128, 32, 8, 512, 16384, kv_type=G.Q8_0) == G.FA_PATH_FUSED
    assert path2(128, 128, 32, 8, 512, 16384, kv_type=G.Q8_0, split=False) == G.FA_PATH_FUSED_KV
    assert path2(128, 128, 32, 8, 512, 16384, kv_type=G.Q8_0, kv_direct=False) == G.FA_PATH_FUSED   # today: the f16 copy, then rule (b)


def test_forced(monkeypatch):
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    for kvt in (G.Q8_0, BF16):
        assert path2(128, 128, 4, 2, 48, 256, kv_type=kvt) == G.FA_PATH_FUSED_KV
        assert path2(128, 128, 4, 2, 48, 256, kv_type=kvt, split=False) == G.FA_PATH_FUSED_KV
        assert path2(128, 128, 4, 2, 1, 9000, kv_type=kvt) == G.FA_PATH_FUSED_KV
        assert path2(128, 128, 4, 2, 15, 256, kv_type=kvt) == G.FA_PATH_KV_ROW
    assert path2(128, 128, 4, 2, 48, 256, kv_type=G.Q8_0, kv_direct=False) == G.FA_PATH_FUSED       # as test_fa_path_cpu.py test_forced has them
    assert path2(128, 128, 4, 2, 48, 256, kv_type=BF16, kv_direct=False) == G.FA_PATH_MFMA3
    assert path2(128, 128, 4, 2, 32, 512, kv_type=BF16, kv_direct=False) == G.FA_PATH_MFMA3


def test_exports():
    assert G.FA_KV_DIRECT == 1 and G.FA_PATH_FUSED_KV == 6 and G.FA_PATH_NAMES[G.FA_PATH_FUSED_KV] == "fused_kv"
    assert {"mi355q_op_flash_attn_ext_path2", "mi355q_op_flash_attn_ext2"} <= set(G.ABI_SYMBOLS)
