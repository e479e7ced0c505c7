"""tests/kvmix_ref.py, the numpy restatement of the CPU's FLASH_ATTN_EXT over a mixed KV cache (K type != V type), against the reference: the fixtures
tests/golden/kvmix_*.npz (made by make_kvmix_golden.py from the x86-64-v3 build through the reference's C API).  Exact, not a tolerance: this is what gives
the device tests (test_gpu_fa_mix.py) their meaning.  With kt == vt the restatement IS the same-type ones (oracle.glue, tests/kvq_ref.py), bit for bit on
their own golden inputs -- it adds no arithmetic of its own, only the pairing.  No GPU needed."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import kvmix_ref  # noqa: E402
import kvq_ref  # noqa: E402
from oracle import glue  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
PAIRS = [(kt, vt) for kt in kvmix_ref.TYPES for vt in kvmix_ref.TYPES if kt != vt]
RING_TAGS = ["decode_gqa_d128_kv256", "batch3_dk64_dv96_kv40_alibi", "softcap_d96_kv64", "decode_nomask_d64_kv1"]
FUSED_PREFILL = GOLDEN / "fa_fused_prefill_gqa_d128_kv256.npz"


def load(name):
    return np.load(GOLDEN / name, allow_pickle=False)


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def test_fixture_set():
    assert len(PAIRS) == 42
    assert sorted(k for k, _ in kvmix_ref.RING) == sorted(v for _, v in kvmix_ref.RING) == sorted(kvmix_ref.TYPES)      # every type once on each side
    files = sorted(GOLDEN.glob("kvmix_*.npz"))
    assert len(files) == 1 + 7 * 4
    assert all(f.stat().st_size < 0.6 * FUSED_PREFILL.stat().st_size for f in files)                                   # well under that fixture's size
    z = load("kvmix_all_pairs_d64_kv96.npz")
    assert z["q"].shape == (1, 2, 2, 64) and z["k_q8_0"].shape == (1, 1, 96, 68) and z["v_f16"].shape == (1, 1, 96, 128)
    m = z["mask"]
    assert np.isinf(m[:2, 41]).all() and not np.isinf(m[:2, 40]).any() and not np.isinf(m[:2, 42]).any()               # a fully masked position in the middle
    assert np.isinf(m[0, 90:]).all() and not np.isinf(m[1, 90]) and np.isinf(m[1, 91:]).all()                          # causal-style


@pytest.mark.parametrize("kt,vt", PAIRS, ids=[f"{k}-{v}" for k, v in PAIRS])
def test_all_pairs_fixture_bit_exact(kt, vt):
    z = load("kvmix_all_pairs_d64_kv96.npz")
    got = kvmix_ref.flash_attn_ext(kt, vt, z["q"], z[f"k_{kt}"], z[f"v_{vt}"], z["mask"], float(z["scale"]))
    want = z[f"y_{kt}_{vt}"]
    assert np.array_equal(bits(got), bits(want)), float(np.abs(got - want).max())


@pytest.mark.parametrize("tag", RING_TAGS)
@pytest.mark.parametrize("kt,vt", kvmix_ref.RING, ids=[f"{k}-{v}" for k, v in kvmix_ref.RING])
def test_ring_fixture_bit_exact(kt, vt, tag):
    z = load(f"kvmix_{kt}_{vt}_{tag}.npz")
    mask = z["mask"] if "mask" in z.files else None
    got = kvmix_ref.flash_attn_ext(kt, vt, z["q"], z["k"], z["v"], mask, float(z["scale"]), float(z["max_bias"]), float(z["softcap"]))
    assert np.array_equal(bits(got), bits(z["y"])), float(np.abs(got - z["y"]).max())


def test_all_pairs_outputs_differ_by_side():
    """the fixture can tell the sides apart: changing only K's type, or only V's, changes the output"""
    z = load("kvmix_all_pairs_d64_kv96.npz")
    assert not np.array_equal(z["y_q8_0_q4_0"], z["y_q4_0_q8_0"])
    assert not np.array_equal(z["y_f16_q8_0"], z["y_f16_q4_0"]) and not np.array_equal(z["y_f16_q8_0"], z["y_q4_0_q8_0"])


# ---- kt == vt: the same-type restatements on their own golden inputs
@pytest.mark.parametrize("name", ["flash_attn_decode_d64_kv96", "flash_attn_decode_gqa_d128_kv256", "flash_attn_batch3_d64_kv40", "flash_attn_alibi_d128_kv64",
                                  "flash_attn_softcap_d96_kv64"])
def test_same_type_f16_is_glue(name):
    g = load(f"{name}.npz")
    args = (g["mask"], float(g["scale"]), float(g["max_bias"]), float(g["softcap"]))
    got = kvmix_ref.flash_attn_ext("f16", "f16", g["q"], g["k"], g["v"], *args)
    assert np.array_equal(bits(got), bits(glue.flash_attn_ext(g["q"], g["k"], g["v"], *args)))
    assert np.array_equal(bits(got), bits(g["y"]))


@pytest.mark.parametrize("name", ["flash_attn_q8_0_batch3_d64_kv96", "flash_attn_q8_0_decode_gqa_d128_kv256"])
def test_same_type_q8_0_is_glue(name):
    g = load(f"{name}.npz")
    args = (g["mask"], float(g["scale"]), float(g["max_bias"]), float(g["softcap"]))
    got = kvmix_ref.flash_attn_ext("q8_0", "q8_0", g["q"], g["k_blocks"], g["v_blocks"], *args)
    assert np.array_equal(bits(got), bits(glue.flash_attn_ext_q8_0(g["q"], g["k_blocks"], g["v_blocks"], *args)))
    assert np.array_equal(bits(got), bits(g["y"]))


def test_same_type_q4_0_is_glue():
    """glue's Q4_0 form has no fixture of its own: the all-pairs fixture's Q4_0 rows on both sides"""
    z = load("kvmix_all_pairs_d64_kv96.npz")
    args = (z["mask"], float(z["scale"]))
    got = kvmix_ref.flash_attn_ext("q4_0", "q4_0", z["q"], z["k_q4_0"], z["v_q4_0"], *args)
    assert np.array_equal(bits(got), bits(glue.flash_attn_ext_q8_0(z["q"], z["k_q4_0"], z["v_q4_0"], *args, kv="q4_0")))


@pytest.mark.parametrize("tag", ["decode_gqa_d128_kv256", "batch3_d96_kv40", "decode_nomask_d64_kv1", "softcap_d96_kv64"])
@pytest.mark.parametrize("kv", list(kvq_ref.TYPES))
def test_same_type_block_types_are_kvq_ref(kv, tag):
    z = load(f"kvq_{kv}_fa_{tag}.npz")
    mask = z["mask"] if "mask" in z.files else None
    args = (mask, float(z["scale"]), float(z["max_bias"]), float(z["softcap"]))
    got = kvmix_ref.flash_attn_ext(kv, kv, z["q"], z["k"], z["v"], *args)
    assert np.array_equal(bits(got), bits(kvq_ref.flash_attn_ext(kv, z["q"], z["k"], z["v"], *args)))
    assert np.array_equal(bits(got), bits(z["y"]))
