"""The bf16 KV-cache fixtures (tests/golden/bf16_kv_*.npz) on the CPU: the numpy statement of ggml_compute_fp32_to_bf16 the GPU tests use gives the
fixture's bits, and where oracle/_ref is built the reference regenerates them byte for byte (make_bf16_kv_golden.py)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle

GOLDEN = Path(__file__).parent / "golden"


def test_fixture_bits_follow_the_rounding_rule():
    g = np.load(GOLDEN / "bf16_kv_convert.npz", allow_pickle=False)
    u = g["x"].view(np.uint32).astype(np.uint64)
    rne = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    want = np.where((u & 0x7FFFFFFF) > 0x7F800000, ((u >> 16) | 0x40).astype(np.uint16), rne)
    assert np.array_equal(want, g["bits"])
    v = (g["bits"].astype(np.uint32) << 16).view(np.float32)
    assert np.isnan(v).sum() == np.isnan(g["x"]).sum()                     # a NaN stays a NaN, nothing else becomes one


_REGEN = """
import importlib.util, sys
from pathlib import Path
import numpy as np
GOLDEN = Path(sys.argv[1])
sys.path.insert(0, str(GOLDEN.parents[1]))
import oracle
spec = importlib.util.spec_from_file_location("make_bf16_kv_golden", GOLDEN / "make_bf16_kv_golden.py")
gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
ref = oracle.Reference("avx2")
g = np.load(GOLDEN / "bf16_kv_convert.npz", allow_pickle=False)
assert np.array_equal(gen.to_bf16(ref, g["x"]), g["bits"])
mm = np.load(GOLDEN / "bf16_kv_mul_mat.npz", allow_pickle=False)
for K in (128, 100, 8):
    y = gen.mul_mat(ref, mm[f"w_k{K}"], mm[f"x_k{K}"][:3])
    assert np.array_equal(y.view(np.uint32), mm[f"y_k{K}_n3"].view(np.uint32)), K
fa = np.load(GOLDEN / "bf16_kv_fa_decode_gqa_d128_kv256.npz", allow_pickle=False)
kf = (fa["k"].astype(np.uint32) << 16).view(np.float32); vf = (fa["v"].astype(np.uint32) << 16).view(np.float32)    # (bf16 values round-trip)
y, kb, vb = gen.fa(ref, fa["q"], kf, vf, fa["mask"], float(fa["scale"]))
assert np.array_equal(kb, fa["k"]) and np.array_equal(vb, fa["v"]) and np.array_equal(y.view(np.uint32), fa["y"].view(np.uint32))
print("regenerated")
"""


@pytest.mark.skipif(not oracle.ref_available("avx2"), reason="oracle/_ref/avx2 not built")
def test_reference_regenerates_the_fixtures():
    # in a child process: the avx2 and scalar builds share library names, and a process that has loaded one resolves the other's libggml to it
    r = subprocess.run([sys.executable, "-c", _REGEN, str(GOLDEN)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "regenerated" in r.stdout, (r.stdout + r.stderr)[-2000:]
