#!/usr/bin/env python3
"""Time IQ3_S / IQ3_XXS MUL_MAT with HIP events: N = 1 at the three Llama-3-8B matrix shapes, N = 512 at 4096 x 4096, and Q4_K at the same
shapes as the bandwidth yardstick of the box.  --moe times MUL_MAT_ID instead: 8 experts of 4096 x 4096, 2 used by each of 512 tokens (1024
pairs, a prompt-sized batch), where planar IQ3 rows run one streamed column per pair and canonical rows are grouped onto the matrix cores.

    python tools/measure_iq3.py [--pkg DIR] [--reps R] [--rounds K] [--json OUT] [--moe]

--pkg points at a llama.cpp.dsp_amd directory (default: this checkout's), so the same script times another build of the library -- the commit
before the planar IQ3 layout keeps these rows canonical and answers on the generic tiers.  Every figure is the median over `rounds` rounds of
`reps` back-to-back launches; the weights of one matrix (7 .. 33 MB) fit the 256 MB Infinity Cache, so each round walks `ring` distinct copies
of the matrix and the rate is an HBM rate, not a cache rate.  Prints one line per (type, shape): microseconds per launch, weight bytes per
second, and the spread (max - min) / median over the rounds.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

SHAPES = [(1, 4096, 4096), (1, 14336, 4096), (1, 4096, 14336), (512, 4096, 4096)]     # (N, M, K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=str(Path(__file__).resolve().parents[1] / "llama.cpp.dsp_amd"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default="")
    ap.add_argument("--moe", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, a.pkg)
    import torch
    import ggml_mi355 as g

    rng = np.random.default_rng(0)
    types = [(g.IQ3_S, 110, 256), (g.IQ3_XXS, 98, 256), (g.Q4_K, 144, 256)]
    out = []
    if a.moe:
        ne, nu, n_tok, M, K = 8, 2, 512, 4096, 4096
        ids = torch.from_numpy(np.stack([rng.permutation(ne)[:nu] for _ in range(n_tok)]).astype(np.int32)).cuda()
        b = torch.from_numpy(rng.uniform(-1, 1, (n_tok, 1, K)).astype(np.float32)).cuda()
        for t, bsize, blck in types:
            w = rng.integers(0, 256, (ne * M, K // blck, bsize), dtype=np.uint8)
            d = rng.uniform(1e-3, 2e-2, (ne * M, K // blck)).astype(np.float16).view(np.uint8).reshape(ne * M, -1, 2)
            w[:, :, 0:2] = d
            if t == g.Q4_K:
                w[:, :, 2:4] = d
            qw = g.QWeight.from_host(t, w.reshape(ne * M, -1), M, K, n_expert=ne)
            for _ in range(2):
                g.mul_mat_id(qw, b, ids)
            torch.cuda.synchronize()
            us = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.reps):
                    g.mul_mat_id(qw, b, ids)
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
            med = statistics.median(us)
            rec = {"type": g.TYPE_NAMES[t], "op": "mul_mat_id", "pairs": n_tok * nu, "n_expert": ne, "M": M, "K": K, "planar": bool(g.is_planar(t, K)),
                   "us": round(med, 2), "spread": round((max(us) - min(us)) / med, 4)}
            out.append(rec)
            print(f"{rec['type']:8s} mul_mat_id pairs={n_tok * nu} experts={ne} M={M} K={K} planar={int(rec['planar'])}  {med:10.2f} us  spread {100 * rec['spread']:.1f} %", flush=True)
    for t, bsize, blck in ([] if a.moe else types):
        for N, M, K in SHAPES:
            rb = K // blck * bsize
            copies = max(2, min(16, (1 << 30) // (M * rb)))                      # ~1 GB of distinct weights: 4 x the Infinity Cache
            w = rng.integers(0, 256, (M, K // blck, bsize), dtype=np.uint8)
            d = rng.uniform(1e-3, 2e-2, (M, K // blck)).astype(np.float16).view(np.uint8).reshape(M, -1, 2)
            w[:, :, 0:2] = d                                                    # every one of these blocks leads with its f16 scale d ...
            if t == g.Q4_K:
                w[:, :, 2:4] = d                                                # ... and Q4_K's dmin follows it
            ws = [g.QWeight.from_host(t, w.reshape(M, -1), M, K) for _ in range(copies)]
            x = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32)).cuda()
            y = torch.empty((N, M), dtype=torch.float32, device="cuda")
            for q in ws[:2]:
                g.mul_mat(q, x, out=y)                                           # warm-up: code objects, workspace
            torch.cuda.synchronize()
            us = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.reps):
                    g.mul_mat(ws[i % copies], x, out=y)
                e1.record()
                torch.cuda.synchronize()
                us.append(e0.elapsed_time(e1) * 1e3 / a.reps)
            med = statistics.median(us)
            rec = {"type": g.TYPE_NAMES[t], "N": N, "M": M, "K": K, "planar": bool(g.is_planar(t, K)), "us": round(med, 2),
                   "GBps": round(M * rb / med / 1e3, 1), "spread": round((max(us) - min(us)) / med, 4)}
            out.append(rec)
            print(f"{rec['type']:8s} N={N:<4d} M={M:<6d} K={K:<6d} planar={int(rec['planar'])}  {med:10.2f} us  {rec['GBps']:8.1f} GB/s  spread {100 * rec['spread']:.1f} %", flush=True)
            del ws
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
