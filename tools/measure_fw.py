#!/usr/bin/env python3
"""Float-weight GEMV: mi355q_op_mul_mat_f (the route every f16 / bf16 weight matrix took before) against mi355q_mul_mat_fw, in alternating runs in
one process on one device.  Per (type, M x K, N): ROUNDS rounds, each timing REPS back-to-back launches of one route and then of the other
with events (the weights are larger than the Infinity Cache or are evicted by the other route's operands only by chance: the table says which
shapes fit); the median over rounds and the spread (min .. max) are reported as microseconds per launch and TB/s of weight bytes.

    python tools/measure_fw.py [--out profiles/fw_stream.md] [--rounds 7] [--reps 20]"""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "llama.cpp.dsp_amd"))

import torch

import ggml_mi355 as G

SHAPES = ((4096, 4096), (14336, 4096), (4096, 14336), (128256, 4096))
NS = (1, 4, 8)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None); ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--forms", action="store_true", help="also time every MI355Q_FW_ROWS_* form at N = 1")
    args = ap.parse_args()
    lines = ["| type | M x K | N | op_mul_mat_f us (min .. max) | mul_mat_fw us (min .. max) | TB/s old | TB/s new | new / old |", "|---|---|---|---|---|---|---|---|"]
    for dt, name in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        for M, K in SHAPES:
            w = (torch.randn(M, K, device="cuda") * 0.05).to(dt)
            for N in NS:
                x = torch.randn(N, K, device="cuda"); y0 = torch.empty(N, M, device="cuda"); y1 = torch.empty(N, M, device="cuda")
                if G.mul_mat_fw_path(30 if dt == torch.bfloat16 else 1, w.data_ptr(), 2 * K, x.data_ptr(), 4 * K, y1.data_ptr(), 4 * M, M, N, K) != G.FW_PATH_STREAM:
                    lines.append(f"| {name} | {M} x {K} | {N} | -- | refused: stays with op_mul_mat_f | | | |")
                    continue
                routes = {"old": lambda: G.op_mul_mat_f(w, x, out=y0), "new": lambda: G.mul_mat_fw(w, x, out=y1)}
                if args.forms and N == 1:
                    for fl, r in G.FW_ROWS_PER_WAVE.items():
                        routes[f"rows{r}"] = (lambda fl=fl: G.mul_mat_fw(w, x, out=y1, flags=fl))
                for f in routes.values():
                    f()
                torch.cuda.synchronize()
                t = {k: [] for k in routes}
                for _ in range(args.rounds):
                    for k, f in routes.items():
                        t[k].append(timed(f, args.reps))
                med = {k: statistics.median(v) for k, v in t.items()}
                tb = {k: 2.0 * M * K / med[k] * 1e-6 for k in med}
                lines.append(f"| {name} | {M} x {K} | {N} | {med['old']:.1f} ({min(t['old']):.1f} .. {max(t['old']):.1f}) | {med['new']:.1f} ({min(t['new']):.1f} .. {max(t['new']):.1f}) | "
                             f"{tb['old']:.2f} | {tb['new']:.2f} | {med['new'] / med['old']:.2f} |")
                extra = "  ".join(f"{k} {med[k]:.1f}" for k in routes if k.startswith("rows"))
                print(lines[-1] + ("   forms: " + extra if extra else ""), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
