"""mi355q_op_flash_attn_ext_path2 with MI355Q_FA_KV_MIXED: which kernels a FLASH_ATTN_EXT call over a mixed KV cache (K type != V type, each of f16, q8_0,
q4_0, q4_1, q5_0, q5_1, iq4_nl) takes, asked from descriptors alone (no device, fake addresses).  DESIGN.md 5.7g, the rule restated case by case:

  MI355Q_FA_FUSED=0   never the fused kernel; a window above 8192 positions then needs the f16 copy or is MI355Q_ERR_UNSUPPORTED
  >= 16 rows          with the copy route (no soft-cap, a workspace large enough, DK % 32 == DV % 32 == 0, an f16 side 16-byte aligned): the f16 rule's
                      answer about the copy; otherwise FUSED_KV where MI355Q_FA_KV_DIRECT is set, the pair and the buckets are built and the alignment
                      holds, else KV_ROW up to 8192 positions, else unsupported
  < 16 rows           KV_ROW up to 8192 positions, beyond it FUSED_KV under the same conditions, else unsupported
  MI355Q_FA_FUSED=1   forces FUSED_KV where it is available, with >= 16 rows or above 8192 positions
Without the flag a mixed pair is refused as before, and with it every same-type call answers what it answers without."""
import ctypes as C

import pytest

import ggml_mi355 as G
from test_fa_kv_path_cpu import AUTO_TABLE, WANT, every_old_input
from test_fa_kv_path_cpu import path2 as path2_same
from test_fa_path_cpu import BF16, F16, F32

SEVEN = [F16, G.Q8_0, G.Q4_0, G.Q4_1, G.Q5_0, G.Q5_1, G.IQ4_NL]
PAIRS = [(kt, vt) for kt in SEVEN for vt in SEVEN if kt != vt]
BUILT = [(kt, vt) for kt, vt in PAIRS if kt in (F16, G.Q8_0) or vt in (F16, G.Q8_0)]          # the fused kernel's mixed instantiations
NOT_BUILT = [p for p in PAIRS if p not in BUILT]


def mix(kt, vt, DK, DV, H, Hk, N, n_kv, softcap=0.0, split=True, k_addr=0x10000, v_addr=0x30000, q_addr=0x20000, workspace_bytes=None,
        kv_direct=True, kv_mixed=True):
    q = G.tensor_desc(F32, [DK, N, H, 1], data=q_addr)
    k = G.tensor_desc(kt, [DK, n_kv, Hk, 1], data=k_addr)
    v = G.tensor_desc(vt, [DV, n_kv, Hk, 1], data=v_addr)
    m = G.tensor_desc(F16, [n_kv, max(N, 64)], data=0x40000)
    return G.op_flash_attn_ext_path(q, k, v, m, softcap, split=split, workspace_bytes=workspace_bytes, kv_direct=kv_direct, kv_mixed=kv_mixed)


def f16_rule(DK, DV, H, Hk, N, n_kv):
    """what the f16 rule answers about the f16 copy of the same shapes (16-byte aligned, with the score scratch as its workspace)"""
    q = G.tensor_desc(F32, [DK, N, H, 1], data=0x20000)
    k = G.tensor_desc(F16, [DK, n_kv, Hk, 1]); v = G.tensor_desc(F16, [DV, n_kv, Hk, 1], data=0x30000)
    m = G.tensor_desc(F16, [n_kv, max(N, 64)], data=0x40000)
    return G.op_flash_attn_ext_path(q, k, v, m, workspace_bytes=(N * n_kv * H * 4 + 255) & ~255)


def last_error() -> str:
    return G.lib().mi355q_last_error().decode(errors="replace")


@pytest.fixture
def auto(monkeypatch):
    monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    monkeypatch.delenv("MI355Q_FA_EXACT", raising=False)


def test_counts():
    assert len(PAIRS) == 42 and len(BUILT) == 22 and len(NOT_BUILT) == 20
    assert G.FA_KV_MIXED == 2 and G.FA_KV_DIRECT == 1


# ------------------------------------------------------------------------------------------------ without the flag: as today
def test_mixed_pairs_without_the_flag_are_refused_as_before(auto):
    for kt, vt in PAIRS + [(BF16, F16), (G.Q8_0, BF16)]:
        for N, n_kv in ((1, 256), (48, 256), (1, 9000)):
            assert mix(kt, vt, 128, 128, 4, 2, N, n_kv, kv_mixed=False, kv_direct=False) == G.ERR_UNSUPPORTED     # the old entry point
            assert mix(kt, vt, 128, 128, 4, 2, N, n_kv, kv_mixed=False, kv_direct=True) == G.ERR_UNSUPPORTED      # ..._path2 with KV_DIRECT alone


def path2_with_bit(DK, DV, H, Hk, N, n_kv, B=1, Bk=1, softcap=0.0, split=True, kv_type=F16, mask_rows=None, mask_cols=None, k_addr=0x10000,
                   workspace_bytes=None, mask=True, kv_direct=True):
    """test_fa_kv_path_cpu.py path2, argument for argument and descriptor for descriptor, with MI355Q_FA_KV_MIXED set as well"""
    q = G.tensor_desc(F32, [DK, N, H, B], data=0x20000)
    k = G.tensor_desc(kv_type, [DK, n_kv, Hk, Bk], data=k_addr)
    v = G.tensor_desc(kv_type, [DV, n_kv, Hk, Bk], data=0x30000)
    m = G.tensor_desc(F16, [mask_cols or n_kv, mask_rows or N], data=0x40000) if mask else None
    return G.op_flash_attn_ext_path(q, k, v, m, softcap, split=split, workspace_bytes=workspace_bytes, kv_direct=kv_direct, kv_mixed=True)


# the literal calls of test_fa_kv_path_cpu.py's tests that its tables do not hold
BLOCK_TYPES = (G.Q8_0, G.Q4_0, G.Q4_1, G.Q5_0, G.Q5_1, G.IQ4_NL)
KV_PATH_LITERALS = (
    [((64, 64, 2, 1, N, n_kv), dict(kv_type=t)) for t in BLOCK_TYPES for N, n_kv in ((1, 8256), (15, 8256), (1, 36880), (15, 8192))] + [
        ((64, 64, 2, 1, 1, 36880), {}),
        ((80, 80, 4, 1, 16, 80), dict(kv_type=BF16, split=False)), ((128, 128, 4, 2, 16, 1025), dict(kv_type=BF16)),
        ((128, 128, 2, 2, 16, 1040), dict(kv_type=BF16, mask_cols=1104)),
        ((128, 128, 4, 2, 1, 9000), dict(kv_type=G.Q8_0, k_addr=0x10001)), ((48, 48, 4, 2, 1, 256), dict(kv_type=G.Q8_0)),
        ((48, 48, 4, 2, 48, 256), dict(kv_type=G.Q8_0, softcap=5.0)), ((72, 72, 4, 2, 1, 9000), dict(kv_type=BF16)),
        ((128, 128, 4, 2, 1, 9000), dict(kv_type=BF16, k_addr=0x10008)),
        ((128, 128, 32, 8, 512, 16384), dict(kv_type=G.Q8_0)), ((128, 128, 32, 8, 512, 16384), dict(kv_type=G.Q8_0, split=False)),
        ((128, 128, 4, 2, 48, 256), dict(kv_type=G.Q8_0)), ((128, 128, 4, 2, 48, 256), dict(kv_type=BF16)),
        ((128, 128, 4, 2, 48, 256), dict(kv_type=G.Q8_0, split=False)), ((128, 128, 4, 2, 48, 256), dict(kv_type=BF16, split=False)),
        ((128, 128, 4, 2, 15, 256), dict(kv_type=G.Q8_0)), ((128, 128, 4, 2, 15, 256), dict(kv_type=BF16)), ((128, 128, 4, 2, 32, 512), dict(kv_type=BF16)),
        ((128, 128, 4, 2, 48, 256), dict(kv_type=G.Q8_0, workspace_bytes=4096)), ((128, 128, 4, 2, 48, 256), dict(mask=False)),
    ])


def every_same_type_input():
    """every descriptor case of test_fa_path_cpu.py (FA_CASES, FA_EXT_CFGS, its other-cache calls: every_old_input) and of test_fa_kv_path_cpu.py
    (AUTO_TABLE, each row also without a workspace as test_auto_table asks it, and the literal calls of its other tests)"""
    yield from every_old_input()
    for DK, DV, H, Hk, N, n_kv, kvt, extra, _want in AUTO_TABLE:
        yield (DK, DV, H, Hk, N, n_kv), dict(extra, kv_type=kvt)
        yield (DK, DV, H, Hk, N, n_kv), dict(extra, kv_type=kvt, split=False)
    yield from KV_PATH_LITERALS


def test_same_type_calls_do_not_see_the_bit(monkeypatch):
    """every one of them answers identically with the bit set: with and without MI355Q_FA_KV_DIRECT, under MI355Q_FA_FUSED unset / 0 / 1"""
    n = 0
    for mode in (None, "0", "1"):
        if mode is None:
            monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
        else:
            monkeypatch.setenv("MI355Q_FA_FUSED", mode)
        for a, kw in every_same_type_input():
            for direct in (False, True):
                assert path2_with_bit(*a, kv_direct=direct, **kw) == path2_same(*a, kv_direct=direct, **kw), (mode, a, kw, direct)
                n += 1
    assert n == 3 * 2 * (len(list(every_old_input())) + 2 * len(AUTO_TABLE) + len(KV_PATH_LITERALS)) and n > 500


def test_auto_table_answers_with_the_bit(auto):
    """test_fa_kv_path_cpu.py's own expectations hold with the bit set (not only equality of the two answers)"""
    for DK, DV, H, Hk, N, n_kv, kvt, extra, want in AUTO_TABLE:
        assert path2_with_bit(DK, DV, H, Hk, N, n_kv, kv_type=kvt, **extra) == WANT[want], (kvt, N, n_kv, extra)


def test_python_defaults_do_not_change_a_call(auto):
    import inspect
    for fn in (G.op_flash_attn_ext, G.op_flash_attn_ext_path):
        p = inspect.signature(fn).parameters
        assert p["kv_v"].default is None and p["kv_mixed"].default is False and p["kv_direct"].default is False and p["kv"].default == "q8_0"
    q = G.tensor_desc(F32, [128, 1, 4, 1], data=0x20000); k = G.tensor_desc(G.Q8_0, [128, 256, 2, 1]); v = G.tensor_desc(G.Q8_0, [128, 256, 2, 1], data=0x30000)
    args = (C.byref(q), C.byref(k), C.byref(v), None, C.byref(G.tensor_desc(F32, [128, 4, 1, 1])), 0.0, 0, 0)
    assert G.op_flash_attn_ext_path(q, k, v, split=False) == int(G.lib().mi355q_op_flash_attn_ext_path(*args)) == G.FA_PATH_KV_ROW
    assert G.op_flash_attn_ext_path(q, k, v, split=False, kv_direct=True) == int(G.lib().mi355q_op_flash_attn_ext_path2(*args, 1))
    assert G.op_flash_attn_ext_path(q, k, v, split=False, kv_mixed=True) == int(G.lib().mi355q_op_flash_attn_ext_path2(*args, 2))
    assert G.op_flash_attn_ext_path(q, k, v, split=False, kv_direct=True, kv_mixed=True) == int(G.lib().mi355q_op_flash_attn_ext_path2(*args, 3))


# ------------------------------------------------------------------------------------------------ the rule, auto
@pytest.mark.parametrize("kt,vt", PAIRS, ids=[f"{k}-{v}" for k, v in PAIRS])
def test_decode_side(auto, kt, vt):
    built = (kt, vt) in BUILT
    for N in (1, 15):
        assert mix(kt, vt, 128, 128, 4, 2, N, 256) == G.FA_PATH_KV_ROW
        assert mix(kt, vt, 128, 128, 4, 2, N, 8192) == G.FA_PATH_KV_ROW                                           # the 8192 / 8193 edge
        assert mix(kt, vt, 128, 128, 4, 2, N, 8193) == (G.FA_PATH_FUSED_KV if built else G.ERR_UNSUPPORTED)
        assert mix(kt, vt, 128, 128, 4, 2, N, 8193, kv_direct=False) == G.ERR_UNSUPPORTED                         # FUSED_KV needs MI355Q_FA_KV_DIRECT too
        assert mix(kt, vt, 128, 128, 4, 2, N, 8192, split=False) == G.FA_PATH_KV_ROW                              # (no answer here depends on the workspace)
    assert mix(kt, vt, 64, 64, 2, 1, 1, 36880) == (G.FA_PATH_FUSED_KV if built else G.ERR_UNSUPPORTED)


@pytest.mark.parametrize("kt,vt", PAIRS, ids=[f"{k}-{v}" for k, v in PAIRS])
def test_prompt_side(auto, kt, vt):
    built = (kt, vt) in BUILT
    # the copy route: the f16 rule's answer about the copy
    assert mix(kt, vt, 128, 128, 4, 2, 48, 256) == f16_rule(128, 128, 4, 2, 48, 256) == G.FA_PATH_MFMA3
    assert mix(kt, vt, 128, 128, 32, 8, 512, 16384) == f16_rule(128, 128, 32, 8, 512, 16384) == G.FA_PATH_FUSED      # scores above 256 MiB: rule (b)
    assert mix(kt, vt, 128, 128, 4, 2, 16, 8193) == f16_rule(128, 128, 4, 2, 16, 8193)                               # above 8192, any pair: the copy
    # no copy (soft-cap, no workspace, too small a workspace): FUSED_KV where built, else the row kernel up to 8192, else refused
    for kw in (dict(softcap=5.0), dict(split=False), dict(workspace_bytes=4096)):
        assert mix(kt, vt, 128, 128, 4, 2, 48, 256, **kw) == (G.FA_PATH_FUSED_KV if built else G.FA_PATH_KV_ROW), kw
        assert mix(kt, vt, 128, 128, 4, 2, 48, 256, kv_direct=False, **kw) == G.FA_PATH_KV_ROW, kw
        assert mix(kt, vt, 128, 128, 4, 2, 16, 8192, **kw) == (G.FA_PATH_FUSED_KV if built else G.FA_PATH_KV_ROW), kw
        assert mix(kt, vt, 128, 128, 4, 2, 16, 8193, **kw) == (G.FA_PATH_FUSED_KV if built else G.ERR_UNSUPPORTED), kw   # an uninstantiated pair above 8192
    if not built:
        assert "8192" in last_error() and "f16 or q8_0 on one side" in last_error()                               # the message names the rule


def test_row_count_edge(auto):
    """N = 15 is the last decode-side row count: with a workspace it still is the row kernel, N = 16 takes the copy"""
    assert mix(G.Q8_0, G.Q4_0, 128, 128, 4, 2, 15, 256) == G.FA_PATH_KV_ROW
    assert mix(G.Q8_0, G.Q4_0, 128, 128, 4, 2, 16, 256) == f16_rule(128, 128, 4, 2, 16, 256)
    assert mix(G.Q8_0, G.Q4_0, 128, 128, 4, 2, 16, 256, softcap=5.0) == G.FA_PATH_FUSED_KV


def test_mixed_buckets(auto):
    """the fused kernel is built for DK and DV in ONE bucket (<= 64, <= 128, <= 256)"""
    for DK, DV, same in ((64, 64, True), (32, 64, True), (96, 128, True), (160, 256, True), (64, 128, False), (128, 64, False), (128, 256, False), (256, 64, False)):
        want_long = G.FA_PATH_FUSED_KV if same else G.ERR_UNSUPPORTED
        assert mix(G.Q8_0, G.Q4_0, DK, DV, 4, 2, 1, 8256) == want_long, (DK, DV)
        assert mix(G.Q8_0, G.Q4_0, DK, DV, 4, 2, 48, 256, softcap=5.0) == (G.FA_PATH_FUSED_KV if same else G.FA_PATH_KV_ROW), (DK, DV)
        assert mix(G.Q8_0, G.Q4_0, DK, DV, 4, 2, 1, 256) == G.FA_PATH_KV_ROW
        assert mix(G.Q8_0, G.Q4_0, DK, DV, 4, 2, 48, 256) == G.FA_PATH_MFMA3                                        # the copy route does not care


def test_alignment(auto):
    # a block side at an odd address: refused outright (blocks are read as halves of words)
    assert mix(G.Q8_0, G.Q4_0, 128, 128, 4, 2, 1, 256, k_addr=0x10001) == G.ERR_UNSUPPORTED
    assert mix(G.Q8_0, G.Q4_0, 128, 128, 4, 2, 1, 256, v_addr=0x30001) == G.ERR_UNSUPPORTED
    assert mix(G.Q8_0, G.Q4_0, 128, 128, 4, 2, 48, 256, v_addr=0x30001) == G.ERR_UNSUPPORTED
    # an even address is enough for a block side on every route
    assert mix(G.Q8_0, G.Q4_0, 128, 128, 4, 2, 1, 8256, k_addr=0x10002, v_addr=0x30006) == G.FA_PATH_FUSED_KV
    # an f16 side that is not 16-byte aligned: no fused kernel and no copy route (it would be read as it lies) -- the row kernel, up to 8192
    assert mix(F16, G.Q8_0, 128, 128, 4, 2, 1, 8256, k_addr=0x10008) == G.ERR_UNSUPPORTED
    assert mix(F16, G.Q8_0, 128, 128, 4, 2, 1, 8256) == G.FA_PATH_FUSED_KV
    assert mix(G.Q8_0, F16, 128, 128, 4, 2, 48, 256, v_addr=0x30008) == G.FA_PATH_KV_ROW
    assert mix(G.Q8_0, F16, 128, 128, 4, 2, 48, 256) == G.FA_PATH_MFMA3
    # q not 16-byte aligned: no fused kernel; the copy route asks the f16 rule, which then has no matrix-core path
    assert mix(G.Q8_0, G.Q4_0, 128, 128, 4, 2, 1, 8256, q_addr=0x20004) == G.ERR_UNSUPPORTED
    assert mix(G.Q8_0, G.Q4_0, 128, 128, 4, 2, 48, 256, softcap=5.0, q_addr=0x20004) == G.FA_PATH_KV_ROW


def test_head_sizes(auto):
    assert mix(G.Q8_0, G.Q4_0, 48, 64, 4, 2, 1, 256) == G.ERR_UNSUPPORTED                  # DK of whole 32-blocks, whatever K's type
    assert mix(F16, G.Q8_0, 48, 64, 4, 2, 1, 256) == G.ERR_UNSUPPORTED
    assert mix(F16, G.Q8_0, 64, 48, 4, 2, 1, 256) == G.ERR_UNSUPPORTED                     # DV of whole 32-blocks under a block V
    assert mix(G.Q8_0, F16, 64, 48, 4, 2, 1, 256) == G.FA_PATH_KV_ROW                      # an f16 V: any DV on the row kernel
    assert mix(G.Q8_0, F16, 64, 48, 4, 2, 48, 256) == G.FA_PATH_FUSED_KV                   # ... no copy (DV % 32), but the fused kernel takes an f16 V of whole 16s
    assert mix(G.Q8_0, F16, 64, 40, 4, 2, 48, 256) == G.FA_PATH_KV_ROW
    assert mix(G.Q8_0, G.Q4_0, 288, 288, 4, 2, 1, 256) == G.ERR_UNSUPPORTED                # the head-size cap of 256


def test_bf16_side_is_refused_with_its_own_message(auto):
    for kt, vt in ((BF16, F16), (F16, BF16), (BF16, G.Q8_0), (G.Q4_0, BF16)):
        for N, n_kv in ((1, 256), (48, 256), (1, 9000)):
            assert mix(kt, vt, 128, 128, 4, 2, N, n_kv) == G.ERR_UNSUPPORTED
            assert "bf16" in last_error()
    assert mix(F16, 0, 128, 128, 4, 2, 1, 256) == G.ERR_UNSUPPORTED                        # an f32 side is no cache type


def test_fused_off(monkeypatch):
    monkeypatch.setenv("MI355Q_FA_FUSED", "0")
    for kt, vt in ((G.Q8_0, G.Q4_0), (F16, G.Q8_0), (G.Q4_0, G.Q4_1)):
        assert mix(kt, vt, 128, 128, 4, 2, 1, 8192) == G.FA_PATH_KV_ROW
        assert mix(kt, vt, 128, 128, 4, 2, 1, 8193) == G.ERR_UNSUPPORTED                    # windows above 8192 are unsupported ...
        assert mix(kt, vt, 128, 128, 4, 2, 15, 36880) == G.ERR_UNSUPPORTED
        assert mix(kt, vt, 128, 128, 4, 2, 48, 8208, softcap=5.0) == G.ERR_UNSUPPORTED
        assert mix(kt, vt, 128, 128, 4, 2, 48, 8208, split=False) == G.ERR_UNSUPPORTED
        assert mix(kt, vt, 128, 128, 4, 2, 48, 256, softcap=5.0) == G.FA_PATH_KV_ROW        # never the fused kernel
        assert mix(kt, vt, 128, 128, 4, 2, 48, 256) == G.FA_PATH_MFMA3                      # the copy route is not the fused kernel
        assert mix(kt, vt, 128, 128, 4, 2, 48, 8208) == G.FA_PATH_MFMA3                     # ... unless the prompt has its f16 copy: the f16 rule under 0
        assert mix(kt, vt, 128, 128, 4, 2, 48, 36880) == G.ERR_UNSUPPORTED                  # (which refuses above 36864 without the fused kernel)


def test_forced(monkeypatch):
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    for kt, vt in BUILT:
        assert mix(kt, vt, 128, 128, 4, 2, 48, 256) == G.FA_PATH_FUSED_KV                   # before the copy route, as for same-type caches
        assert mix(kt, vt, 128, 128, 4, 2, 48, 256, split=False) == G.FA_PATH_FUSED_KV
        assert mix(kt, vt, 128, 128, 4, 2, 1, 9000) == G.FA_PATH_FUSED_KV
        assert mix(kt, vt, 128, 128, 4, 2, 15, 256) == G.FA_PATH_KV_ROW                     # < 16 rows inside 8192: the CPU's bits, forced or not
        assert mix(kt, vt, 128, 128, 4, 2, 48, 256, kv_direct=False) == G.FA_PATH_FUSED     # not available: the copy, where the f16 rule is forced too
    for kt, vt in NOT_BUILT:
        assert mix(kt, vt, 128, 128, 4, 2, 48, 256) == G.FA_PATH_FUSED
        assert mix(kt, vt, 128, 128, 4, 2, 48, 256, split=False) == G.FA_PATH_KV_ROW
        assert mix(kt, vt, 128, 128, 4, 2, 1, 9000) == G.ERR_UNSUPPORTED


def test_shape_errors_are_the_ops(auto):
    q = G.tensor_desc(F32, [128, 16, 4, 1]); k = G.tensor_desc(G.Q8_0, [128, 64, 3, 1]); v = G.tensor_desc(G.Q4_0, [128, 64, 3, 1])
    assert G.op_flash_attn_ext_path(q, k, v, kv_mixed=True) == G.ERR_SHAPE                  # 4 heads over 3
    k = G.tensor_desc(G.Q8_0, [128, 64, 2, 1]); v = G.tensor_desc(G.Q4_0, [128, 63, 2, 1])
    assert G.op_flash_attn_ext_path(q, k, v, kv_mixed=True) == G.ERR_SHAPE                  # K and V windows differ
    v = G.tensor_desc(G.Q4_0, [128, 64, 2, 1], nb=[20, 80, 80 * 64, 80 * 128])
    assert G.op_flash_attn_ext_path(q, k, v, kv_mixed=True) == G.ERR_UNSUPPORTED            # nb[0] is not V's block size
