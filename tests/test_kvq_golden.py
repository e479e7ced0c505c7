"""The numpy restatement of the CPU backend's arithmetic on a Q4_1 / Q5_0 / Q5_1 / IQ4_NL KV cache (tests/kvq_ref.py) against the reference:
the fixtures tests/golden/kvq_*.npz (made by make_kvq_golden.py from the x86-64-v3 build) and, where oracle/_ref is built, the live reference.
Exact, not a tolerance: this is what gives the device tests (test_gpu_kvq.py, test_gpu_plan_kvq.py) their meaning.  No GPU needed.

Which build: the AVX2 one.  The stores and the dequantization are the same bytes in the scalar build (ggml-quants.c is ISO C, nothing is
contracted in either; checked live below); the dot products differ between the builds by their summation order, as for Q8_0 / Q4_0."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import kvq_ref  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
KVS = list(kvq_ref.TYPES)
PLAIN = ["decode_gqa_d128_kv256", "decode_gqa_d256_kv128", "decode_nomask_d64_kv1", "batch3_d96_kv40"]


def load(name):
    return np.load(GOLDEN / name, allow_pickle=False)


def fa_fixture(kv, tag):
    z = load(f"kvq_{kv}_fa_{tag}.npz")
    mask = z["mask"] if "mask" in z.files else None
    return z, kvq_ref.flash_attn_ext(kv, z["q"], z["k"], z["v"], mask, float(z["scale"]), float(z["max_bias"]), float(z["softcap"]))


@pytest.mark.parametrize("kv", KVS)
def test_store_bytes_fixture(kv):
    z = load(f"kvq_{kv}_store.npz")
    got = kvq_ref.quantize_rows(kv, z["x"])
    assert got.shape == z["blocks"].shape and got.shape[1] == 4 * kvq_ref.block_bytes(kv)
    bad = np.argwhere(got != z["blocks"])
    assert bad.size == 0, (kv, bad[:8])


@pytest.mark.parametrize("tag", PLAIN)
@pytest.mark.parametrize("kv", KVS)
def test_flash_attn_fixture_bit_exact(kv, tag):
    z, got = fa_fixture(kv, tag)
    assert np.array_equal(got.view(np.uint32), z["y"].view(np.uint32)), (kv, tag, float(np.abs(got - z["y"]).max()))


@pytest.mark.parametrize("tag", ["alibi_d128_kv64", "softcap_d96_kv64"])
@pytest.mark.parametrize("kv", KVS)
def test_flash_attn_fixture_alibi_softcap(kv, tag):
    """powf / tanhf go through numpy and the C library here: the bound the Q8_0 cache is held to (tests/test_gpu_glue.py)"""
    z, got = fa_fixture(kv, tag)
    assert float(np.abs(got - z["y"]).max()) <= 1e-5 * float(np.abs(z["y"]).max()), (kv, tag)


@pytest.mark.parametrize("kv", KVS)
def test_prefill_fixture_rows(kv):
    """the 48-row prefill fixture, a few rows of it (the walk is a python loop): first, one in the middle, last"""
    z = load(f"kvq_{kv}_fa_prefill_gqa_d128_kv256.npz")
    for n in (0, 23, 47):
        got = kvq_ref.flash_attn_ext(kv, z["q"][:, :, n:n + 1], z["k"], z["v"], z["mask"][n:n + 1], float(z["scale"]))
        assert np.array_equal(got[:, 0].view(np.uint32), z["y"][:, n].view(np.uint32)), (kv, n)


@pytest.mark.parametrize("kv", KVS)
def test_decode_loop_fixture(kv):
    z = load(f"kvq_{kv}_loop.npz")
    steps = z["q"].shape[0]
    for s in range(steps):
        mask = np.zeros((64, s + 1), np.float16)
        got = kvq_ref.flash_attn_ext(kv, z["q"][s], z["k"][:, :, :s + 1], z["v"][:, :, :s + 1], mask, 0.125)
        assert np.array_equal(got.view(np.uint32), z["y"][s].view(np.uint32)), (kv, s)
    if kv != "iq4_nl":                   # the fixture's cache is ggml_quantize_chunk's: the row quantizer for these, a seven-try search for IQ4_NL
        assert np.array_equal(kvq_ref.quantize_rows(kv, z["kf"]), z["k"]) and np.array_equal(kvq_ref.quantize_rows(kv, z["vf"]), z["v"])


@pytest.mark.parametrize("kv", KVS)
def test_longest_window_fixture(kv):
    """the 8192-position case from its seed: the restatement's store bytes have the fixture's digests, its walk the reference's output bits"""
    z = load(f"kvq_{kv}_long_kv8192.npz")
    rng = np.random.default_rng(int(z["seed"]))
    q = rng.standard_normal((1, 2, 1, 64)).astype(np.float32)
    kf = rng.standard_normal((1, 1, 8192, 64)).astype(np.float32); vf = rng.standard_normal((1, 1, 8192, 64)).astype(np.float32)
    kb, vb = kvq_ref.quantize_rows(kv, kf), kvq_ref.quantize_rows(kv, vf)
    assert int(kb.astype(np.uint64).sum()) == int(z["k_sum"]) and int(vb.astype(np.uint64).sum()) == int(z["v_sum"])
    if kv == "iq4_nl":
        assert "y" not in z.files          # (the reference's window there is ggml_quantize_chunk's, not a store's: make_kvq_golden.py)
        return
    mask = np.zeros((64, 8192), np.float16); mask[0, 8000:] = -np.inf
    got = kvq_ref.flash_attn_ext(kv, q, kb, vb, mask, 0.125)
    assert np.array_equal(got.view(np.uint32), z["y"].view(np.uint32)), float(np.abs(got - z["y"]).max())


def test_fixture_sizes_and_generator_cases():
    files = sorted(GOLDEN.glob("kvq_*.npz"))
    assert len(files) == 4 * (1 + 7 + 1 + 1)
    assert all(f.stat().st_size < 1 << 20 for f in files)
    src = (GOLDEN / "make_kvq_golden.py").read_text()
    for tag in PLAIN + ["alibi_d128_kv64", "softcap_d96_kv64", "prefill_gqa_d128_kv256"]:
        assert re.search(rf'"{tag}"', src)


# ---- live, where the reference is built.  In a child process per build: the avx2 and scalar builds share library names, and a process that has
# loaded one resolves the other's libggml to it.
_LIVE = r"""
import importlib.util, sys
from pathlib import Path
import numpy as np
ROOT = Path(sys.argv[1]); variant = sys.argv[2]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import oracle, kvq_ref
spec = importlib.util.spec_from_file_location("make_kvq_golden", ROOT / "tests" / "golden" / "make_kvq_golden.py")
gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
ref = oracle.Reference(variant)
for kv, (t, bb, _) in kvq_ref.TYPES.items():
    # stores and dequantization: random rows of several magnitudes (ggml-quants.c: nothing contracted, the same bytes in both builds)
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((256, 256)) * rng.choice([1e-4, 1.0, 50.0], (256, 1))).astype(np.float32)
    mine = kvq_ref.quantize_rows(kv, x)
    for fn in ("ref_from_float_ref", "ref_from_float_cpu"):
        want = gen.from_float(ref, fn, t, bb, x)
        assert np.array_equal(mine, want), (kv, variant, fn, int((mine != want).sum()))
    deq = np.empty(x.shape, np.float32)
    for i in range(x.shape[0]):
        ref.lib.ref_dequantize_row(t, oracle._ptr(want[i]), oracle._ptr(deq[i]), x.shape[1])
    assert np.array_equal(kvq_ref.dequantize(kv, want).view(np.uint32), deq.view(np.uint32)), (kv, variant)
    if variant != "avx2":
        continue
    # the fixtures come out of the reference again, and FLASH_ATTN_EXT on fresh shapes (odd block counts included) has the restatement's bits
    z = np.load(ROOT / "tests" / "golden" / f"kvq_{kv}_store.npz", allow_pickle=False)
    got = gen.from_float(ref, "ref_from_float_ref", t, bb, z["x"])
    small = np.abs(z["x"].reshape(z["x"].shape[0], -1, 32)).max(axis=-1) < np.float32(1e-15)
    keep = np.repeat(~small if kv == "iq4_nl" else np.ones_like(small), bb, axis=1)        # (an all-small IQ4_NL block: only d = 0 is defined)
    assert np.array_equal(got[keep], z["blocks"][keep]), kv
    rng = np.random.default_rng(5 + t)
    for (H, Hk, N, D, n_kv) in ((4, 2, 2, 96, 33), (2, 1, 1, 32, 70), (4, 4, 1, 160, 50)):
        q = (rng.standard_normal((1, H, N, D)) * 2).astype(np.float32)
        kf = rng.standard_normal((1, Hk, n_kv, D)).astype(np.float32); vf = rng.standard_normal((1, Hk, n_kv, D)).astype(np.float32)
        mask = gen.causal_mask(N, n_kv, n_kv - 3)
        y, kb, vb = gen.fa(ref, t, bb, q, kf, vf, mask, 0.1)
        got = kvq_ref.flash_attn_ext(kv, q, kb, vb, mask, 0.1)
        assert np.array_equal(got.view(np.uint32), y.view(np.uint32)), (kv, D, float(np.abs(got - y).max()))
print("live ok")
"""


@pytest.mark.parametrize("variant", ["avx2", "scalar"])
def test_restatement_against_live_reference(variant):
    import subprocess
    if not (ROOT / "oracle" / "_ref" / variant / "librefshim.so").exists():
        pytest.skip(f"oracle/_ref/{variant} is not built")
    r = subprocess.run([sys.executable, "-c", _LIVE, str(ROOT), variant], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "live ok" in r.stdout, (r.stdout + r.stderr)[-2000:]
