#!/usr/bin/env python3
"""Time FLASH_ATTN_EXT over a quantized (q8_0, q4_0) or bf16 KV cache with HIP events: the route a call takes today (mi355q_op_flash_attn_ext, no
flag: the f16 copy of a quantized cache followed by the three-step or the fused f16 kernel, the three-step bf16 path) against the fused kernel on
the cache's own rows (mi355q_op_flash_attn_ext2 with MI355Q_FA_KV_DIRECT; MI355Q_FA_FUSED=1 where `auto` would not send the call there),
alternating the two call by call in one process.

    python tools/measure_fa_kv.py [--reps R] [--warmup W] [--md OUT.md] [--json OUT.json]

One layer of Llama-3-8B attention: 32 heads over 8 KV heads, head size 128.  Prompt: 512 query rows, causal f16 mask (the batch is the last 512
positions of the window), windows of 4096, 8192, 16384 and 32768 positions.  Decode: one query row, direct at 16384 and 32768 positions (there is
no other route above 8192), with the row kernel's time at 8192 beside it for scale.  Every figure is the median of `reps` (>= 20) single calls,
each between two device events and ended by a synchronise, after `warmup` calls of each form; spread = (max - min) / median over the timed calls.
These are call times (launches and, for today's route, the copy kernels included), not kernel times.
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
KVS = ["q8_0", "q4_0", "bf16"]
WINDOWS = [4096, 8192, 16384, 32768]


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
    scale = float(np.float32(1.0 / np.sqrt(D)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    def stats(us):
        med = statistics.median(us)
        return round(med, 1), round((max(us) - min(us)) / med, 3)

    def fused_env(mode):
        if mode is None:
            os.environ.pop("MI355Q_FA_FUSED", None)
        else:
            os.environ["MI355Q_FA_FUSED"] = mode

    prompt, decode = [], []
    for n_kv in WINDOWS:
        kf = torch.from_numpy(rng.standard_normal((1, HK, n_kv, D)).astype(np.float32)).cuda()
        vf = torch.from_numpy(rng.standard_normal((1, HK, n_kv, D)).astype(np.float32)).cuda()
        q = torch.from_numpy(rng.standard_normal((1, H, N, D)).astype(np.float32)).cuda()
        q1 = q[:, :, :1].contiguous()
        mh = np.zeros((N, n_kv), np.float16)
        for t in range(N):
            mh[t, n_kv - N + t + 1:] = -np.inf
        m = torch.from_numpy(mh).cuda()
        m1 = torch.zeros((1, n_kv), dtype=torch.float16, device="cuda")
        for kv in KVS:
            if kv == "bf16":
                k, v, kvarg = kf.to(torch.bfloat16), vf.to(torch.bfloat16), "q8_0"
            else:
                bb = g.KV_BLOCK[kv][0]
                k = torch.zeros((1, HK, n_kv, D // 32 * bb), dtype=torch.uint8, device="cuda"); v = torch.zeros_like(k)
                g.op_cpy(kf, k, kv=kv); g.op_cpy(vf, v, kv=kv)
                kvarg = kv
            # ---- the prompt: today's route under `auto` against direct
            fused_env(None)
            auto_direct = g.op_flash_attn_ext_path(q, k, v, m, kv=kvarg, kv_direct=True) == g.FA_PATH_FUSED_KV
            forms = {"today": (None, False), "direct": (None if auto_direct else "1", True)}
            paths, ys, us = {}, {}, {"today": [], "direct": []}

            def call(form):
                mode, direct = forms[form]
                fused_env(mode)
                return g.op_flash_attn_ext(q, k, v, m, scale, kv=kvarg, kv_direct=direct)

            for form, (mode, direct) in forms.items():
                fused_env(mode)
                paths[form] = g.FA_PATH_NAMES[g.op_flash_attn_ext_path(q, k, v, m, kv=kvarg, kv_direct=direct)]
                if form == "today" and kv != "bf16":               # what the f16 copy takes (the copy itself is not a path of its own)
                    k16 = g.tensor_desc(1, [D, n_kv, HK, 1]); v16 = g.tensor_desc(1, [D, n_kv, HK, 1], data=0x20000000)
                    paths[form] = "copy+" + g.FA_PATH_NAMES[g.op_flash_attn_ext_path(q, k16, v16, m)]
                for _ in range(a.warmup):
                    ys[form] = call(form)
            torch.cuda.synchronize()
            assert paths["direct"] == "fused_kv", paths
            diff = float((ys["today"] - ys["direct"]).abs().max()) / float(ys["today"].abs().max())
            for _ in range(a.reps):
                for form in forms:
                    us[form].append(timed(lambda: call(form)))
            rec = {"kv": kv, "n_kv": n_kv, "today_path": paths["today"], "direct_mode": "auto" if auto_direct else "forced", "max_rel_diff": diff}
            for form in forms:
                rec[form + "_us"], rec[form + "_spread"] = stats(us[form])
            prompt.append(rec)
            print(f"N=512 {kv:5s} n_kv={n_kv:<6d} today {rec['today_path']:11s} {rec['today_us']:10.1f} us ({100 * rec['today_spread']:.1f} %)   direct ({rec['direct_mode']}) "
                  f"{rec['direct_us']:10.1f} us ({100 * rec['direct_spread']:.1f} %)   today / direct {rec['today_us'] / rec['direct_us']:.2f}   diff {diff:.1e}", flush=True)
            del ys
            # ---- decode: one row
            fused_env(None)
            if n_kv == 8192:
                assert g.op_flash_attn_ext_path(q1, k, v, m1, kv=kvarg, kv_direct=True) == g.FA_PATH_KV_ROW
                fn = lambda: g.op_flash_attn_ext(q1, k, v, m1, scale, kv=kvarg)
                name = "kv_row"
            elif n_kv > 8192:
                assert g.op_flash_attn_ext_path(q1, k, v, m1, kv=kvarg, kv_direct=True) == g.FA_PATH_FUSED_KV
                fn = lambda: g.op_flash_attn_ext(q1, k, v, m1, scale, kv=kvarg, kv_direct=True)
                name = "fused_kv"
            else:
                continue
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            med, spread = stats([timed(fn) for _ in range(a.reps)])
            decode.append({"kv": kv, "n_kv": n_kv, "path": name, "us": med, "spread": spread})
            print(f"N=1   {kv:5s} n_kv={n_kv:<6d} {name:9s} {med:10.1f} us ({100 * spread:.1f} %)", flush=True)
        del kf, vf, q, m
    fused_env(None)
    out = {"prompt": prompt, "decode": decode}
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(out, indent=1))
    if a.md:
        lines = ["| cache | n_kv | today's route | today, us (spread) | direct | direct, us (spread) | today / direct | max diff / max output |", "|---|---|---|---|---|---|---|---|"]
        for r in prompt:
            lines.append(f"| {r['kv']} | {r['n_kv']} | {r['today_path']} | {r['today_us']} ({100 * r['today_spread']:.1f} %) | {r['direct_mode']} | "
                         f"{r['direct_us']} ({100 * r['direct_spread']:.1f} %) | {r['today_us'] / r['direct_us']:.2f} | {r['max_rel_diff']:.1e} |")
        lines += ["", "| cache | n_kv | one query row: path | us (spread) |", "|---|---|---|---|"]
        for r in decode:
            lines.append(f"| {r['kv']} | {r['n_kv']} | {r['path']} | {r['us']} ({100 * r['spread']:.1f} %) |")
        Path(a.md).parent.mkdir(parents=True, exist_ok=True)
        Path(a.md).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
