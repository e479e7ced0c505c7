"""tests/fa_exact.py without a device: the selector cases of tests/test_gpu_fa_exact.py stay within their own design.

  * the project's CPU restatements of FLASH_ATTN_EXT (oracle.glue.flash_attn_ext for an f16 cache -- the F16 accumulator and all --,
    oracle.glue.flash_attn_ext_q8_0 for q8_0 / q4_0, tests/kvq_ref.py for q4_1 / q5_0 / q5_1 / iq4_nl) return the expectation BIT FOR BIT on every
    case: the expectation is what the reference CPU backend computes, not a property of one kernel.  (A bf16 cache has no restatement here; its
    cases are held by exact_expectation's own assertions.)
  * exact_expectation refuses data outside the design: a runner-up only 64 below the maximum, a tie set of 3, a tie sum beyond f16's integers.
  * mi355q_op_flash_attn_ext_path2 answers the path each device case means to test, from descriptors alone (tests/test_fa_path_cpu.py's way).
"""
import numpy as np
import pytest

import fa_exact
import ggml_mi355 as G
import kvq_ref
from oracle import glue

F32, F16, BF16 = 0, 1, 30
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# cases that share their data (the three-step cases are the fused ones on another path) are restated once
def _distinct():
    seen, out = set(), []
    for cid, (_, kw) in fa_exact.CASES.items():
        key = repr(sorted(dict(kw, cache=kw.get("cache", "f16")).items(), key=lambda x: x[0]))
        if key not in seen and kw.get("cache", "f16") != "bf16":
            seen.add(key); out.append(cid)
    return out


@pytest.mark.parametrize("cid", _distinct())
def test_cpu_restatement_returns_the_expectation(cid):
    c = fa_exact.case(cid)
    k, v = (np.broadcast_to(a, (c.B,) + a.shape[1:]) for a in (c.k, c.v))          # (the restatements take one cache per batch)
    if c.cache == "f16":
        y = glue.flash_attn_ext(c.q, k, v, c.mask, c.scale, c.max_bias, c.softcap)
    elif c.cache in ("q8_0", "q4_0"):
        y = glue.flash_attn_ext_q8_0(c.q, k, v, c.mask, c.scale, c.max_bias, c.softcap, kv=c.cache)
    else:
        y = kvq_ref.flash_attn_ext(c.cache, c.q, k, v, c.mask, c.scale, c.max_bias, c.softcap)
    assert np.array_equal(bits(y), bits(c.expect)), (cid, int((bits(y) != bits(c.expect)).sum()))


def test_every_case_builds_and_is_distinctive():
    """every case of the device file builds (selector_case asserts the design on its own data); the expectation is no constant, and every V row
    outside the tie sets holds poison: no element of it is smaller than 16 (units of the cache's values)"""
    for cid in fa_exact.CASES:
        c = fa_exact.case(cid)
        assert c.expect.shape == (c.B, c.N, c.H, c.DV) and np.isfinite(c.expect).all()
        assert len(np.unique(c.expect)) > 8, cid
        v = fa_exact.cache_values(c.cache, c.v)
        inside = np.zeros((c.Hk, c.n_kv), bool)
        for (b, h, t), A in c.sets.items():
            inside[h // (c.H // c.Hk), A] = True
        if (~inside).any():
            assert np.abs(v[0][~inside]).min() >= 16 * c.unit, cid


def _tiny(mask_decoy=-128.0, n_match=1, v_big=False):
    """one head, one row, 8 positions of 32 elements: `n_match` positions share the maximum, position 7 is a decoy"""
    w = fa_exact.code_words(32, 32, 0)
    q = (127.0 * w[1])[None, None, None]
    k = np.zeros((1, 1, 8, 32)); v = np.arange(8 * 32, dtype=np.float64).reshape(1, 1, 8, 32) % 13
    for j in range(n_match):
        k[0, 0, j] = w[1]
    k[0, 0, 7] = w[1]
    if v_big:
        v[0, 0, 0, 0] = 4096.0
    mask = np.zeros((1, 8), np.float16); mask[0, 7] = mask_decoy
    return q, k, v, mask, 2.0 ** -4


def test_exact_expectation_accepts_the_design_and_rejects_what_lies_outside():
    q, k, v, m, s = _tiny()
    assert np.array_equal(fa_exact.exact_expectation(q, k, v, m, s)[0, 0, 0], v[0, 0, 0].astype(f32))
    q, k, v, m, s = _tiny(n_match=2)
    assert np.array_equal(fa_exact.exact_expectation(q, k, v, m, s)[0, 0, 0], ((v[0, 0, 0] + v[0, 0, 1]) / 2).astype(f32))
    with pytest.raises(AssertionError, match="64.0 below"):
        fa_exact.exact_expectation(*_tiny(mask_decoy=-64.0))                    # a gap of 64: exp(-64) = 1.6e-28 is a normal f32
    with pytest.raises(AssertionError, match="tie set of 3"):
        fa_exact.exact_expectation(*_tiny(n_match=3))
    with pytest.raises(AssertionError, match="beyond 2048"):
        fa_exact.exact_expectation(*_tiny(v_big=True))
    q, k, v, m, s = _tiny()
    with pytest.raises(AssertionError, match="power of two"):
        fa_exact.exact_expectation(q, k, v, m, 0.1)
    m2 = m.copy(); m2[:] = -np.inf
    with pytest.raises(AssertionError, match="fully masked"):
        fa_exact.exact_expectation(q, k, v, m2, s)
    m3 = m.copy(); m3[0, 3] = 0.5
    with pytest.raises(AssertionError, match="integers"):
        fa_exact.exact_expectation(q, k, v, m3, s)


def test_gap_against_expf():
    """the one number the design rests on: expf underflows to +0 below about -103.98 (log of the smallest subnormal, 2^-149, is -103.28; halfway
    to zero -103.97); GAP = 128 is below it with room, 64 is not"""
    assert fa_exact.GAP == 128.0
    assert float(kvq_ref._libm.expf(-128.0)) == 0.0 and float(kvq_ref._libm.expf(-104.0)) == 0.0
    assert float(kvq_ref._libm.expf(-103.0)) > 0.0 and float(kvq_ref._libm.expf(-64.0)) > 1e-28
    assert float(kvq_ref._libm.expf(0.0)) == 1.0
    assert f32(np.exp(np.float64(-128.0))) == 0.0


# ---------------------------------------------------------------------------------------------------------------- the path of every device case
TYPE_CODE = {"f16": F16, "bf16": BF16, "q8_0": G.Q8_0, "q4_0": G.Q4_0, "q4_1": G.Q4_1, "q5_0": G.Q5_0, "q5_1": G.Q5_1, "iq4_nl": G.IQ4_NL}
PATHS = {"fused": G.FA_PATH_FUSED, "fused_kv": G.FA_PATH_FUSED_KV, "mfma3": G.FA_PATH_MFMA3, "row_seq": G.FA_PATH_ROW_SEQ,
         "row_split": G.FA_PATH_ROW_SPLIT, "row_f32": G.FA_PATH_ROW_F32, "kv_row": G.FA_PATH_KV_ROW}


def descriptors(c):
    """the operands of the device test as descriptors with fake addresses: contiguous, or ("heads") head views of one [n_kv, Hk, row] buffer"""
    t = TYPE_CODE[c.cache]
    def kv_desc(D, data):
        if c.cache in fa_exact.BLOCK_TYPES:
            e, row = fa_exact.BLOCK_BYTES[c.cache], D // 32 * fa_exact.BLOCK_BYTES[c.cache]
        else:
            e, row = 2, 2 * D
        nb = [e, c.Hk * row, row, c.n_kv * c.Hk * row] if c.run.layout == "heads" else [e, row, c.n_kv * row, c.Hk * c.n_kv * row]
        return G.tensor_desc(t, [D, c.n_kv, c.Hk, c.Bk], nb=nb, data=data)
    q = G.tensor_desc(F32, [c.DK, c.N, c.H, c.B], data=0x200000)
    m = G.tensor_desc(F16, [c.mask.shape[1], c.mask.shape[0]], data=0x400000) if c.mask is not None else None
    return q, kv_desc(c.DK, 0x100000), kv_desc(c.DV, 0x300000), m


def set_env(monkeypatch, c):
    monkeypatch.delenv("MI355Q_FA_EXACT", raising=False)
    if c.run.fused is None:
        monkeypatch.delenv("MI355Q_FA_FUSED", raising=False)
    else:
        monkeypatch.setenv("MI355Q_FA_FUSED", c.run.fused)


@pytest.mark.parametrize("cid", list(fa_exact.CASES))
def test_every_device_case_takes_its_path(monkeypatch, cid):
    c = fa_exact.case(cid)
    set_env(monkeypatch, c)
    q, k, v, m = descriptors(c)
    got = G.op_flash_attn_ext_path(q, k, v, m, c.softcap, split=c.run.split, kv_direct=c.run.kv_direct)
    assert got == PATHS[c.run.path], (cid, G.FA_PATH_NAMES.get(got, got))


def test_the_case_list_covers_what_it_must():
    ids = set(fa_exact.CASES)
    for kv in fa_exact.BLOCK_TYPES:
        assert {f"fused-{kv}-swa", f"fused-{kv}-walk-d32", f"fused-{kv}-walk-d32-llama", f"kvrow-{kv}-swa", f"kvrow-{kv}-late_after_decoy",
                f"kvrow-{kv}-ties_across"} <= ids
    assert {p for p in PATHS} == {run["path"] for run, _ in fa_exact.CASES.values()}
    # the llama layout of the 18-, 22- and 34-byte blocks is only 2-byte aligned (three heads side by side), the others' 4-byte: both load forms run
    for kv in fa_exact.BLOCK_TYPES:
        assert (3 * fa_exact.BLOCK_BYTES[kv]) % 4 == (2 if kv in ("q8_0", "q4_0", "q5_0", "iq4_nl") else 0)
    # the walk selects every position of a tile (of both tiles) in every walk case
    for cid in ("fused-f16-walk", "fused-f16-walk-dk192-dv80", "fused-bf16-big-walk", "fused-q5_1-walk-d32", "fused-iq4_nl-walk-d32-llama"):
        c = fa_exact.case(cid)
        sel = {int(A[0]) for A in c.sets.values()}
        assert {j % 64 for j in sel} == set(range(64)) and {j // 64 for j in sel} == {0, 1}, cid
    # the sliding window: workgroup 0 starts at tile 1, whose every position is masked for row 63 and not for row 0
    c = fa_exact.case("fused-f16-swa")
    assert c.dead[:64, :64].all() and c.dead[63, 64:128].all() and not c.dead[0, 64:128].all() and not c.dead[64:, 192:].all()
    # the late maximum: the first live tile holds a position exactly GAP below the maximum of the last tile
    c = fa_exact.case("fused-f16-late_after_decoy")
    assert all(int(A[0]) >= 192 for A in c.sets.values()) and (c.mask[:, :64] == -128).any()
    # tie sets that span tiles / pieces
    for cid, cut in (("fused-f16-ties_across-2", 64), ("fused-f16-ties_across-4", 64), ("fused-f16-ties_across-64", 64), ("split3-f16-ties_across-2", 100),
                     ("split3-f16-ties_across-4", 100)):
        c = fa_exact.case(cid)
        assert all((A < cut).sum() * 2 == A.size for A in c.sets.values()), cid
    # bf16 beyond f16's range
    c = fa_exact.case("fused-bf16-big-swa")
    assert np.abs(fa_exact.cache_values("bf16", c.v)).min() > 65504 or np.abs(c.expect[c.expect != 0]).min() >= 2.0 ** 18
    assert np.abs(fa_exact.cache_values("bf16", c.k)).min() >= 2.0 ** 18
