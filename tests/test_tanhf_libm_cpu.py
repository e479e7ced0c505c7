"""csrc/tanhf_libm.h, the host C library's tanhf restated for the soft-cap of the CPU-exact mixed-cache attention kernel (k_flash_attn_ext_mix), bit for
bit against RECORDED values: tests/golden/tanhf_libm.npz holds arguments around every branch edge, a logarithmic grid, random bit patterns, both signs, and
the values the C library gave that the reference's soft-cap fixtures were made with (tests/golden/make_tanhf_golden.py).  So the check does not move with the
host's C library.  The header is plain C++: tools/check_tanhf_libm.cc is compiled with the host compiler and runs the text the kernel compiles; on the device
the soft-cap cases of tests/test_gpu_fa_mix.py hold it.  Needs a host C++ compiler -- a tool, not hardware: without one the test skips and says so."""
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def test_tanhf_libm_equals_the_c_library(tmp_path):
    z = np.load(ROOT / "tests" / "golden" / "tanhf_libm.npz", allow_pickle=False)
    x, y = z["x"], z["y"]
    assert x.dtype == y.dtype == np.float32 and len(x) == len(y) > 50000
    ax = np.abs(x[np.isfinite(x)])
    assert ax.min() == 0 and (ax < 2.0 ** -55).any() and ((ax > 0.3) & (ax < 0.6)).sum() > 1000 and (ax >= 22).any()      # every branch has arguments
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine (a missing tool, not missing hardware): csrc/tanhf_libm.h was not checked")
    pairs = tmp_path / "pairs.bin"
    np.stack([x, y], axis=1).astype("<f4").tofile(pairs)
    exe = tmp_path / "check_tanhf_libm"
    r = subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-pthread", f"-I{ROOT / 'llama.cpp.dsp_amd' / 'csrc'}",
                        str(ROOT / "tools" / "check_tanhf_libm.cc"), "-o", str(exe), "-lm"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([str(exe), "--file", str(pairs)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and f"checked {len(x)} values, 0 differ" in r.stdout, r.stdout[-2000:]
