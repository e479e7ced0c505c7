#!/usr/bin/env python3
"""Generate tests/golden/tanhf_libm.npz: arguments x and the values y = tanhf(x) of the host C library the reference CPU backend was run with for the
soft-cap fixtures (the GNU C library 2.35: the fdlibm single-precision form over expm1f).  csrc/tanhf_libm.h restates that function; the recorded values
pin it whatever C library a later host has.  The arguments: every branch edge of tanhf and of the expm1f it calls (a window of bit patterns around each),
magnitudes from 2^-60 to 2^6 on a logarithmic grid, random bit patterns, both signs, zeros, infinities and a NaN.  Arrays only."""
import ctypes
import ctypes.util
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent / "tanhf_libm.npz"


def main():
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.tanhf.restype = ctypes.c_float; m.tanhf.argtypes = [ctypes.c_float]
    rng = np.random.default_rng(2235)
    # |x| at tanhf's own edges, and where 2 |x| meets expm1f's edges (0.5 ln2, 1.5 ln2, 27 ln2, 2^-25) and its k = 1, 2, 23, 56 steps
    edges = [0x24000000, 0x3f800000, 0x41b00000, 0x3eb17218 - 0x00800000, 0x3F851592 - 0x00800000, 0x4195b844 - 0x00800000, 0x33000000 - 0x00800000]
    edges += [int(np.float32(k * 0.34657359).view(np.uint32)) for k in (1, 2, 3, 5, 22, 23, 24, 55, 56, 57, 63)]
    bits = [np.arange(e - 600, e + 600, dtype=np.int64) for e in edges]
    bits.append(np.float32(2.0 ** np.linspace(-60, 6, 12000)).view(np.uint32).astype(np.int64))
    bits.append(rng.integers(0x30000000, 0x42000000, 14000))
    bits.append(rng.integers(0, 0x7f800000, 2000))
    b = np.unique(np.concatenate(bits)).astype(np.uint32)
    b = np.concatenate([b, b | np.uint32(0x80000000), np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000], np.uint32)])
    x = b.view(np.float32)
    y = np.array([m.tanhf(float(v)) for v in x], np.float32)
    np.savez_compressed(OUT, x=x, y=y)
    print(OUT.name, OUT.stat().st_size, len(x))


if __name__ == "__main__":
    main()
