#!/usr/bin/env python3
"""Time FLASH_ATTN_EXT over a mixed KV cache (-ctk A -ctv B; MI355Q_FA_KV_MIXED) with HIP events against the same-type forms, which this
feature left as they were, alternating the forms call by call in one process.

    python tools/measure_fa_mix.py [--reps R] [--warmup W] [--md OUT.md] [--json OUT.json]

One layer of Llama-3-8B attention: 32 heads over 8 KV heads, head size 128; the pairs (q8_0, q4_0) and (f16, q8_0).
  row kernel    one query row at 2048 and 8192 positions, no workspace: the mixed row kernel against the same-type row kernel on q8_0 and on q4_0 and the
                f16 call (the CPU-exact seq kernel is for <= 1024 positions: here the f32 row kernel)
  fused direct  one query row and 512 query rows (causal) at 16384 positions, no workspace, MI355Q_FA_KV_DIRECT: the mixed instantiations against the
                same-type direct form on q8_0 and on q4_0
Every figure is the median of `reps` (>= 20) single calls, each between two device events and ended by a synchronise, after `warmup` calls of each form;
spread = (max - min) / median over the timed calls.  These are call times (launches included), not kernel times.
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "llama.cpp.dsp_amd"))

H, HK, D = 32, 8, 128
MIXED = [("q8_0", "q4_0"), ("f16", "q8_0")]
SAME = ["q8_0", "q4_0", "f16"]
# (group, query rows, positions)
CASES = [("row", 1, 2048), ("row", 1, 8192), ("fused", 1, 16384), ("fused", 512, 16384)]


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
    os.environ.pop("MI355Q_FA_FUSED", None)

    rng = np.random.default_rng(0)
    scale = float(np.float32(1.0 / np.sqrt(D)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def side(t, x):
        if t == "f16":
            return x.to(torch.float16)
        out = torch.zeros(x.shape[:-1] + (D // 32 * g.KV_BLOCK[t][0],), dtype=torch.uint8, device="cuda")
        g.op_cpy(x, out, kv=t)
        return out

    recs = []
    for group, N, n_kv in CASES:
        kf = torch.from_numpy(rng.standard_normal((1, HK, n_kv, D)).astype(np.float32)).cuda()
        vf = torch.from_numpy(rng.standard_normal((1, HK, n_kv, D)).astype(np.float32)).cuda()
        q = torch.from_numpy(rng.standard_normal((1, H, N, D)).astype(np.float32)).cuda()
        mh = np.zeros((N, n_kv), np.float16)
        for t in range(N):
            mh[t, n_kv - N + t + 1:] = -np.inf
        m = torch.from_numpy(mh).cuda()
        forms = {}
        for kt, vt in MIXED + [(t, t) for t in SAME]:
            if group == "fused" and kt == vt == "f16":
                continue                                                      # (the f16 fused kernel is the yardstick of the bits, not of this time)
            k, v = side(kt, kf), side(vt, vf)
            kwargs = dict(kv=kt if kt != "f16" else "q8_0", split=False)
            if kt != vt:
                kwargs.update(kv_v=vt if vt != "f16" else "q8_0", kv_mixed=True)
            if group == "fused":
                kwargs["kv_direct"] = True
            path = g.op_flash_attn_ext_path(q, k, v, m, **kwargs)
            assert path >= 0, (kt, vt, path)
            if kt != vt or kt != "f16":
                assert path == (g.FA_PATH_KV_ROW if group == "row" else g.FA_PATH_FUSED_KV), (kt, vt, g.FA_PATH_NAMES[path])
            forms[f"{kt}/{vt}"] = (g.FA_PATH_NAMES[path], (lambda k=k, v=v, kwargs=kwargs: g.op_flash_attn_ext(q, k, v, m, scale, **kwargs)))
        for _, fn in forms.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        us = {name: [] for name in forms}
        for _ in range(a.reps):
            for name, (_, fn) in forms.items():
                us[name].append(timed(fn))
        for name, (path, _) in forms.items():
            med = statistics.median(us[name])
            rec = {"group": group, "N": N, "n_kv": n_kv, "k/v": name, "path": path, "us": round(med, 1), "spread": round((max(us[name]) - min(us[name])) / med, 3)}
            recs.append(rec)
            print(f"{group:5s} N={N:<4d} n_kv={n_kv:<6d} {name:12s} {path:9s} {rec['us']:10.1f} us ({100 * rec['spread']:.1f} %)", flush=True)
        del kf, vf, q, m, forms
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(recs, indent=1))
    if a.md:
        lines = ["| form | query rows | n_kv | K / V | path | us (spread) |", "|---|---|---|---|---|---|"]
        for r in recs:
            lines.append(f"| {r['group']} | {r['N']} | {r['n_kv']} | {r['k/v']} | {r['path']} | {r['us']} ({100 * r['spread']:.1f} %) |")
        Path(a.md).parent.mkdir(parents=True, exist_ok=True)
        Path(a.md).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
