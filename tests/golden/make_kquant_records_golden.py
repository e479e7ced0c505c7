"""Records what mi355q_mul_mat gives for the cases of tests/kquant_cases.py, as tests/golden/kquant_records_outputs.npz.

The file was written with the library as it stood BEFORE the planar Q4_K / Q5_K scale field became four 24-bit records, so
tests/test_gpu_kquant_records.py holds the new layout to the old outputs bit for bit.  Usage (on a GPU):
    [MI355Q_LIB=path/to/libmi355q.so] python tests/golden/make_kquant_records_golden.py OUT.npz"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT, ROOT / "llama.cpp.dsp_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import numpy as np
import torch

import ggml_mi355 as g
from kquant_cases import KS, NS, TYPES, M, case_inputs, golden_key

out = {}
for t in TYPES:
    for k in KS:
        for n in NS:
            w, x = case_inputs(t, k, n)
            y = g.mul_mat(g.QWeight.from_host(t, w, M, k), torch.from_numpy(x).cuda()).cpu().numpy()
            out[golden_key(t, k, n)] = y
np.savez_compressed(sys.argv[1], **out)
print("wrote", len(out), "arrays to", sys.argv[1])
