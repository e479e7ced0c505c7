"""mi355q_op_flash_attn_ext_path: which kernels a FLASH_ATTN_EXT call takes, asked from descriptors alone (no device, fake addresses).

The rule stands once in the library and mi355q_op_flash_attn_ext follows it.  With MI355Q_FA_FUSED unset no input of the
existing device tests may move to the fused kernel; one input per clause of the rule must.  MI355Q_FA_FUSED=0 never answers FUSED and keeps
the refusal above 36864 positions; =1 sends every call the kernel can take with >= 16 query rows to it.
"""
import pytest

import ggml_mi355 as G

F32, F16, BF16 = 0, 1, 30

# tests/test_gpu_glue_branches.py FA_CASES: (branch, DK, DV, H, Hk, N, B, Bk, n_kv, max_bias, split)
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
BRANCH_PATH = {"seq": G.FA_PATH_ROW_SEQ, "split": G.FA_PATH_ROW_SPLIT, "single": G.FA_PATH_ROW_F32, "mfma": G.FA_PATH_MFMA3}

# tests/test_gpu_glue.py test_flash_attn_ext: (DK, DV, H, Hk, N, n_kv, max_bias, softcap) -> today's path; the mask has 32 * ceil(N / 32) rows
FA_EXT_CFGS = [
    ((128, 128, 8, 2, 1, 512, 0.0, 0.0), G.FA_PATH_ROW_SEQ), ((64, 64, 4, 4, 7, 96, 0.0, 0.0), G.FA_PATH_ROW_SEQ),
    ((128, 128, 8, 8, 3, 300, 8.0, 0.0), G.FA_PATH_ROW_SEQ), ((80, 80, 4, 1, 2, 64, 0.0, 10.0), G.FA_PATH_ROW_F32),
    ((256, 256, 2, 2, 1, 1000, 0.0, 0.0), G.FA_PATH_ROW_SEQ), ((128, 128, 32, 8, 1, 4096, 0.0, 0.0), G.FA_PATH_ROW_SPLIT),
    ((128, 128, 8, 2, 150, 336, 0.0, 0.0), G.FA_PATH_MFMA3), ((64, 64, 4, 2, 40, 96, 4.0, 0.0), G.FA_PATH_MFMA3),
    ((96, 96, 4, 4, 33, 80, 0.0, 5.0), G.FA_PATH_ROW_SEQ),
]


def path(DK, DV, H, Hk, N, n_kv, B=1, Bk=1, softcap=0.0, split=True, kv_type=F16, mask_rows=None, mask_cols=None, k_addr=0x10000, workspace_bytes=None,
         mask=True):
    q = G.tensor_desc(F32, [DK, N, H, B], data=0x20000)
    k = G.tensor_desc(kv_type, [DK, n_kv, Hk, Bk], data=k_addr)
    v = G.tensor_desc(kv_type, [DV, n_kv, Hk, Bk], data=0x30000)
    m = G.tensor_desc(F16, [mask_cols or n_kv, mask_rows or N], data=0x40000) if mask else None
    return G.op_flash_attn_ext_path(q, k, v, m, softcap, split=split, workspace_bytes=workspace_bytes)


@pytest.fixture
def auto(monkeypatch):
    monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    monkeypatch.delenv("MI355Q_FA_EXACT", raising=False)


@pytest.mark.parametrize("case", FA_CASES, ids=[c[0] for c in FA_CASES])
def test_branch_cases_keep_their_path(auto, case):
    name, DK, DV, H, Hk, N, B, Bk, n_kv, _, split = case
    assert path(DK, DV, H, Hk, N, n_kv, B, Bk, split=split) == BRANCH_PATH[name.split("-")[0].rstrip("0123456789")], name


@pytest.mark.parametrize("cfg,want", FA_EXT_CFGS, ids=str)
def test_flash_attn_ext_configurations_keep_their_path(auto, cfg, want):
    DK, DV, H, Hk, N, n_kv, _, softcap = cfg
    assert path(DK, DV, H, Hk, N, n_kv, softcap=softcap, mask_rows=32 * ((N + 31) // 32)) == want


def test_auto_rule_clause_a(auto):
    assert path(128, 128, 4, 2, 33, 1040, softcap=5.0) == G.FA_PATH_FUSED                  # soft-cap
    assert path(128, 128, 4, 2, 33, 1040) == G.FA_PATH_MFMA3                               # (without it: three-step)
    assert path(128, 128, 2, 2, 16, 1025, split=False) == G.FA_PATH_FUSED                  # no workspace
    assert path(128, 128, 2, 2, 16, 1040, workspace_bytes=16 * 1040 * 2 * 4 - 1) == G.FA_PATH_FUSED       # a workspace too small for the scores
    assert path(128, 128, 2, 2, 16, 1040, mask_cols=1104) == G.FA_PATH_FUSED               # a mask wider than the window
    assert path(128, 128, 2, 2, 15, 1025, split=False) == G.FA_PATH_ROW_F32                # fewer than 16 rows: a row kernel
    assert path(80, 80, 4, 1, 16, 80, softcap=5.0) == G.FA_PATH_FUSED                      # DK % 32 != 0: no CPU-exact row kernel to keep
    assert path(96, 96, 4, 1, 16, 80, softcap=5.0) == G.FA_PATH_ROW_SEQ                    # (DK % 32 == 0 and a short window: the CPU's bits stay)
    assert path(128, 128, 2, 2, 16, 1025, split=False, k_addr=0x10008) == G.FA_PATH_ROW_F32      # a misaligned K: the row kernel
    assert path(72, 72, 2, 2, 16, 1025, split=False) == G.FA_PATH_ROW_F32                  # head size no multiple of 16


def test_auto_rule_clause_b(auto):
    # N * n_kv * H * B * 4 = 256 MiB exactly at N = 512, n_kv = 4096, H = 32: the three-step path; one query row more: fused
    assert 512 * 4096 * 32 * 4 == 256 << 20
    assert path(128, 128, 32, 8, 512, 4096) == G.FA_PATH_MFMA3
    assert path(128, 128, 32, 8, 513, 4096) == G.FA_PATH_FUSED
    assert path(128, 128, 32, 8, 512, 8192) == G.FA_PATH_FUSED


def test_auto_rule_clause_c(auto):
    assert path(64, 64, 2, 1, 1, 36880) == G.FA_PATH_FUSED
    assert path(64, 64, 2, 1, 16, 36880) == G.FA_PATH_FUSED
    assert path(64, 64, 2, 1, 1, 36864) == G.FA_PATH_ROW_SPLIT                              # (the last window of the row kernels)
    assert path(72, 72, 2, 1, 1, 36880) == G.ERR_UNSUPPORTED
    assert b"multiples of 16" in G.lib().mi355q_last_error()
    assert path(64, 64, 2, 1, 1, 36880, k_addr=0x10008) == G.ERR_UNSUPPORTED


def test_other_caches_as_today(auto):
    assert path(128, 128, 4, 2, 1, 9000, kv_type=BF16) == G.ERR_UNSUPPORTED                # a bf16 cache: n_kv <= 8192 on the row kernel
    assert path(128, 128, 4, 2, 1, 8192, kv_type=BF16) == G.FA_PATH_KV_ROW
    assert path(128, 128, 4, 2, 32, 9008, kv_type=BF16) == G.FA_PATH_MFMA3                 # (its three-step form has no such limit)
    assert path(128, 128, 4, 2, 32, 9008, kv_type=BF16, softcap=5.0) == G.ERR_UNSUPPORTED  # no bf16 fused form
    assert path(128, 128, 4, 2, 1, 256, kv_type=G.Q8_0) == G.FA_PATH_KV_ROW
    assert path(128, 128, 4, 2, 1, 9000, kv_type=G.Q8_0) == G.ERR_UNSUPPORTED
    assert path(128, 128, 4, 2, 48, 256, kv_type=G.Q8_0) == G.FA_PATH_MFMA3                # decoded to f16 scratch, then the rule again
    assert path(128, 128, 4, 2, 48, 256, kv_type=G.Q8_0, softcap=5.0) == G.FA_PATH_KV_ROW


def test_off_is_the_parent(monkeypatch):
    monkeypatch.setenv("MI355Q_FA_FUSED", "0")
    for case in FA_CASES:
        name, DK, DV, H, Hk, N, B, Bk, n_kv, _, split = case
        assert path(DK, DV, H, Hk, N, n_kv, B, Bk, split=split) == BRANCH_PATH[name.split("-")[0].rstrip("0123456789")], name
    assert path(128, 128, 4, 2, 33, 1040, softcap=5.0) == G.FA_PATH_ROW_SPLIT
    assert path(128, 128, 2, 2, 16, 1025, split=False) == G.FA_PATH_ROW_F32
    assert path(80, 80, 4, 1, 16, 80, softcap=5.0) == G.FA_PATH_ROW_F32
    assert path(128, 128, 32, 8, 513, 4096) == G.FA_PATH_MFMA3
    assert path(64, 64, 2, 1, 1, 36880) == G.ERR_UNSUPPORTED
    assert path(64, 64, 2, 1, 16, 36880) == G.ERR_UNSUPPORTED


def test_forced(monkeypatch):
    monkeypatch.setenv("MI355Q_FA_FUSED", "1")
    for case in FA_CASES:
        name, DK, DV, H, Hk, N, B, Bk, n_kv, _, split = case
        got = path(DK, DV, H, Hk, N, n_kv, B, Bk, split=split)
        assert got == (G.FA_PATH_FUSED if N >= 16 else BRANCH_PATH[name.split("-")[0].rstrip("0123456789")]), name
    for cfg, want in FA_EXT_CFGS:
        DK, DV, H, Hk, N, n_kv, _, softcap = cfg
        assert path(DK, DV, H, Hk, N, n_kv, softcap=softcap, mask_rows=32 * ((N + 31) // 32)) == (G.FA_PATH_FUSED if N >= 16 else want), cfg
    assert path(16, 16, 1, 1, 16, 1, mask=False) == G.FA_PATH_FUSED
    assert path(64, 64, 2, 1, 1, 36880) == G.FA_PATH_FUSED
    assert path(72, 72, 2, 2, 16, 64) == G.FA_PATH_ROW_F32                                  # not a multiple of 16: never fused
    assert path(128, 128, 2, 2, 16, 1025, k_addr=0x10008) == G.FA_PATH_ROW_SPLIT
    assert path(128, 128, 4, 2, 32, 512, kv_type=BF16) == G.FA_PATH_MFMA3
    assert path(128, 128, 4, 2, 48, 256, kv_type=G.Q8_0) == G.FA_PATH_FUSED                # the f16 copy follows the same rule
    monkeypatch.setenv("MI355Q_FA_FUSED", "auto")
    assert path(128, 128, 4, 2, 48, 256, kv_type=G.Q8_0) == G.FA_PATH_MFMA3


def test_shape_errors_are_the_ops(auto):
    q = G.tensor_desc(F32, [128, 16, 4, 1]); k = G.tensor_desc(F16, [128, 64, 3, 1]); v = G.tensor_desc(F16, [128, 64, 3, 1])
    assert G.op_flash_attn_ext_path(q, k, v) == G.ERR_SHAPE                                  # 4 heads over 3
    k = G.tensor_desc(F32, [128, 64, 2, 1])
    assert G.op_flash_attn_ext_path(q, k, v) == G.ERR_UNSUPPORTED
