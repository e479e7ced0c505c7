#!/usr/bin/env python3
"""Time FLASH_ATTN_EXT for a prompt batch with HIP events: the fused matrix-core kernel (MI355Q_FA_FUSED=1, k_flash_attn_mfma) against the
path the call takes without it (MI355Q_FA_FUSED=0: the three-step matrix-core path with its score scratch, or the per-row kernel under a
soft-cap), alternating the two call by call in one process.

    python tools/measure_fa.py [--reps R] [--warmup W] [--md OUT.md] [--json OUT.json]

One layer of Llama-3-8B attention: 32 heads over 8 KV heads, head size 128, 512 query rows, causal f16 mask (the batch is the last 512 positions
of the window), windows of 512, 4096, 8192 and 32768 positions; a soft-cap case at 4096 (per-row kernel against fused); a no-mask case at 8192
next to the causal one.  Every figure is the median of `reps` (>= 20) single calls, each between two device events and ended by a synchronise,
after `warmup` calls of each form; spread = (max - min) / median over the timed calls.  The last column is the largest difference of the two
forms' outputs relative to the largest output: both round P to f16, so it is of the order of 1e-4.
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "llama.cpp.dsp_amd"))

H, HK, D, N = 32, 8, 128, 512
# (tag, n_kv, mask: "causal" or "none", soft-cap)
CASES = [("causal", 512, "causal", 0.0), ("causal", 4096, "causal", 0.0), ("causal", 8192, "causal", 0.0), ("causal", 32768, "causal", 0.0),
         ("softcap", 4096, "causal", 30.0), ("nomask", 8192, "none", 0.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--md", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed calls per form"
    import torch
    import ggml_mi355 as g
    assert torch.cuda.is_available(), "this measurement needs the GPU: there is no fallback"

    rng = np.random.default_rng(0)
    out = []
    for tag, n_kv, mask_kind, softcap in CASES:
        q = torch.from_numpy(rng.standard_normal((1, H, N, D)).astype(np.float32)).cuda()
        k = torch.from_numpy(rng.standard_normal((1, HK, n_kv, D)).astype(np.float16)).cuda()
        v = torch.from_numpy(rng.standard_normal((1, HK, n_kv, D)).astype(np.float16)).cuda()
        m = None
        if mask_kind == "causal":
            mh = np.zeros((N, n_kv), np.float16)
            for t in range(N):
                mh[t, n_kv - N + t + 1:] = -np.inf
            m = torch.from_numpy(mh).cuda()
        scale = float(np.float32(1.0 / np.sqrt(D)))
        paths, ys, us = {}, {}, {"0": [], "1": []}

        def call(mode):
            os.environ["MI355Q_FA_FUSED"] = mode
            return g.op_flash_attn_ext(q, k, v, m, scale, 0.0, softcap)

        for mode in ("0", "1"):
            os.environ["MI355Q_FA_FUSED"] = mode
            paths[mode] = g.FA_PATH_NAMES[g.op_flash_attn_ext_path(q, k, v, m, softcap)]
            for _ in range(a.warmup):
                ys[mode] = call(mode)
        torch.cuda.synchronize()
        assert paths["1"] == "fused" and paths["0"] != "fused", paths
        top = float(ys["0"].abs().max())
        diff = float((ys["0"] - ys["1"]).abs().max()) / top
        for _ in range(a.reps):
            for mode in ("0", "1"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call(mode)
                e1.record()
                torch.cuda.synchronize()
                us[mode].append(e0.elapsed_time(e1) * 1e3)
        rec = {"case": tag, "n_kv": n_kv, "mask": mask_kind, "softcap": softcap, "scratch_MiB": N * n_kv * H * 4 / 2 ** 20, "other_path": paths["0"], "max_rel_diff": diff}
        for mode, name in (("0", "other"), ("1", "fused")):
            med = statistics.median(us[mode])
            rec[name + "_us"] = round(med, 1); rec[name + "_spread"] = round((max(us[mode]) - min(us[mode])) / med, 3)
        out.append(rec)
        print(f"{tag:8s} n_kv={n_kv:<6d} {paths['0']:9s} {rec['other_us']:10.1f} us (spread {100 * rec['other_spread']:.1f} %)   fused {rec['fused_us']:10.1f} us "
              f"(spread {100 * rec['fused_spread']:.1f} %)   ratio {rec['other_us'] / rec['fused_us']:.2f}x   diff {diff:.1e}", flush=True)
        del q, k, v, m, ys
    os.environ.pop("MI355Q_FA_FUSED", None)
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1))
    if a.md:
        lines = ["| case | n_kv | score scratch | other path | other, us (spread) | fused, us (spread) | other / fused | max diff / max output |", "|---|---|---|---|---|---|---|---|"]
        for r in out:
            lines.append(f"| {r['case']} | {r['n_kv']} | {r['scratch_MiB']:.0f} MiB | {r['other_path']} | {r['other_us']} ({100 * r['other_spread']:.1f} %) | "
                         f"{r['fused_us']} ({100 * r['fused_spread']:.1f} %) | {r['other_us'] / r['fused_us']:.2f} | {r['max_rel_diff']:.1e} |")
        Path(a.md).parent.mkdir(parents=True, exist_ok=True)
        Path(a.md).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
