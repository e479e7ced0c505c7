#!/usr/bin/env python3
"""Time the decode plan's attention stage over mixed K / V cache types (MI355Q_STAGE_KVV_*, plan_attn_mix) at the C-ABI, beside the
same-type stages, alternating the forms run by run in one process.

    python tools/measure_plan_kvmix.py [--reps R] [--warmup W] [--layers L] [--windows 128,1024,4096] [--md OUT.md] [--json OUT.json]

Llama-3-8B's shapes (32 heads over 8 KV heads of 128, n_embd 4096, Q4_K_M weights made of random valid blocks as bench.py makes them), the flash
layout (V rows per position), windows of 128, 1024 and 4096 positions with the token at the window's last position; caches (q8_0, q4_0), (f16, q8_0),
(q8_0, f16) beside q8_0, q4_0 and f16.  Per window and cache, three plans:
  qkv     the q | k | v GEMV stage alone (the same for every cache: the yardstick of the next line)
  stage   that stage and the attention stage: `stage - qkv` is what the attention stage adds to a launch
  step    the whole decode step of `--layers` layers and the output matrix as one launch (norms, rope, cache stores, attention, SiLU, residuals)
A plan that mi355q_plan_create refuses (a window past the pair's LDS limit) is reported as refused with the library's message: the plugin runs such a
graph node by node.  Every figure is the median of `reps` (>= 20) single runs, each between two device events and ended by a synchronise, after `warmup`
runs of each form; spread = (max - min) / median.  The forms of one window alternate run by run.  These are launch-to-end times of one plan run with the
token's inputs already on the device, not llama-bench rates.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "llama.cpp.dsp_amd"), str(ROOT)]

CACHES = [("q8_0", "q4_0"), ("f16", "q8_0"), ("q8_0", "f16"), ("q8_0", "q8_0"), ("q4_0", "q4_0"), ("f16", "f16")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--windows", default="128,1024,4096")
    ap.add_argument("--md", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 timed runs per form"
    windows = [int(w) for w in a.windows.split(",")]
    import torch
    import ggml_mi355 as g
    from ggml_mi355 import workloads as wl
    import bench
    assert torch.cuda.is_available(), "this measurement needs the GPU: there is no fallback"
    dev = torch.device("cuda")
    cfg = dict(wl.LLAMA3_8B, n_layer=a.layers)
    E, F, nh, nkv, hd = cfg["n_embd"], cfg["n_ff"], cfg["n_head"], cfg["n_head_kv"], cfg["head_dim"]
    kvd, L = nkv * hd, a.layers
    by = {s.name: bench.device_random_weight(torch, g, s, dev) for s in wl.llama_matmuls(cfg, "Q4_K_M")}
    torch.manual_seed(0)
    f32 = lambda n: torch.zeros((1, n), dtype=torch.float32, device=dev)
    x_in = torch.randn((1, E), dtype=torch.float32, device=dev)
    q, k, v, att, o, gate, up, d, hcur, ffn_inp = f32(E), f32(kvd), f32(kvd), f32(E), f32(E), f32(F), f32(F), f32(E), f32(E), f32(E)
    logits = f32(by["output"].M)
    norm_w = [(1.0 + 0.1 * torch.randn(E, device=dev)).float() for _ in range(2 * L + 1)]
    bb = lambda t: 64 if t == "f16" else g.KV_BLOCK[t][0]                     # bytes per 32 elements of a row

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    recs = []
    for n_kv in windows:
        pos = n_kv - 1
        pos_d = torch.tensor([pos], dtype=torch.int32, device=dev)
        mask = torch.zeros(n_kv, dtype=torch.float32, device=dev)
        src = torch.randn((n_kv, kvd), dtype=torch.float32, device=dev)

        def cache(t):
            """n_kv positions of one layer's K or V in the side's type, as bytes [n_kv, n_head_kv * rb]"""
            if t == "f16":
                return src.to(torch.float16).view(torch.uint8).clone()
            out = torch.zeros((n_kv, kvd // 32 * bb(t)), dtype=torch.uint8, device=dev)
            g.op_cpy(src, out, kv=t)
            return out

        forms, keep = {}, []
        for kt, vt in CACHES:
            krb, vrb = hd // 32 * bb(kt), hd // 32 * bb(vt)
            krow, vrow = nkv * krb, nkv * vrb
            kcs, vcs = [cache(kt) for _ in range(L)], [cache(vt) for _ in range(L)]
            dst = torch.tensor([[kc.data_ptr() + pos * krow, vc.data_ptr() + pos * vrow] for kc, vc in zip(kcs, vcs)], dtype=torch.int64, device=dev)
            keep.append((kcs, vcs, dst))

            def attn(li, kt=kt, vt=vt, kcs=kcs, vcs=vcs, dst=dst, krb=krb, vrb=vrb, krow=krow, vrow=vrow):
                ad = dict(q=q, k=k, v=v, pos=pos_d, rope=dict(n_dims=hd, mode=0, n_ctx_orig=8192, freq_base=500000.0), k_cache=kcs[li], v_cache=vcs[li],
                          k_nb_pos=krow, k_nb_head=krb, v_nb_pos=vrow, v_nb_dim=2 if vt == "f16" else bb(vt), v_nb_head=vrb, k_dst=dst[li, 0:1], v_dst=dst[li, 1:2],
                          v_dst_nb=2 if vt == "f16" else 0, mask=mask, n_head=nh, n_head_kv=nkv, head_dim=hd, n_kv=n_kv, scale=1.0 / hd ** 0.5, out=att, kv=kt)
                if vt != kt:
                    ad["kv_v"] = vt
                return dict(attn=ad, no_plain=True)

            W = lambda il, n: by[f"blk.{il}.{n}"]
            qkv0 = dict(ws=[W(0, "attn_q"), W(0, "attn_k"), W(0, "attn_v")], ys=[q, k, v], x=x_in, x_kind=g.X_NORM, norm_w=norm_w[0], eps=1e-5, no_plain=True)
            step, x0, x1 = [], x_in, None
            for li in range(L):
                step.append(dict(ws=[W(li, "attn_q"), W(li, "attn_k"), W(li, "attn_v")], ys=[q, k, v], x=x0, x1=x1, x_kind=g.X_NORM, norm_w=norm_w[2 * li], eps=1e-5,
                                 sum_out=hcur if x1 is not None else None, no_plain=True))
                h_res = hcur if x1 is not None else x0
                step.append(attn(li))
                step.append(dict(ws=[W(li, "attn_output")], ys=[o], x=att, no_plain=True))
                step.append(dict(ws=[W(li, "ffn_gate"), W(li, "ffn_up")], ys=[gate, up], x=h_res, x1=o, x_kind=g.X_NORM, norm_w=norm_w[2 * li + 1], eps=1e-5,
                                 sum_out=ffn_inp, y_kind=g.Y_UNARY_MUL, y_unary=g.UNARY_SILU, no_plain=True))
                step.append(dict(ws=[W(li, "ffn_down")], ys=[d], x=gate, no_plain=True))
                x0, x1 = ffn_inp, d
            step.append(dict(ws=[by["output"]], ys=[logits], x=x0, x1=x1, x_kind=g.X_NORM, norm_w=norm_w[2 * L], eps=1e-5))
            name = f"{kt}/{vt}"
            for what, stages in (("qkv", [qkv0]), ("stage", [qkv0, attn(0)]), ("step", step)):
                if what == "qkv" and forms.get(("qkv", "any")):
                    continue
                try:
                    plan = g.Plan(stages)
                except g.Mi355qError as e:
                    msg = str(e).split("plan_create: ", 1)[-1]
                    recs.append({"n_kv": n_kv, "k/v": name, "what": what, "refused": msg})
                    print(f"n_kv={n_kv:<5d} {name:10s} {what:5s} refused: {msg}", flush=True)
                    continue
                forms[(what, "any" if what == "qkv" else name)] = plan
        for plan in forms.values():
            for _ in range(a.warmup):
                plan.run()
        torch.cuda.synchronize()
        assert all(p.status() == 0 for p in forms.values())
        us = {key: [] for key in forms}
        for _ in range(a.reps):
            for key, plan in forms.items():
                us[key].append(timed(plan.run))
        assert all(p.status() == 0 for p in forms.values())
        qkv_med = statistics.median(us[("qkv", "any")])
        for (what, name), ts in us.items():
            med = statistics.median(ts)
            rec = {"n_kv": n_kv, "k/v": name, "what": what, "us": round(med, 1), "spread": round((max(ts) - min(ts)) / med, 3)}
            if what == "stage":
                rec["attn_us"] = round(med - qkv_med, 1)
            recs.append(rec)
            print(f"n_kv={n_kv:<5d} {name:10s} {what:5s} {rec['us']:10.1f} us ({100 * rec['spread']:.1f} %)" + (f"  attention adds {rec['attn_us']:.1f} us" if what == "stage" else ""), flush=True)
        for plan in forms.values():
            plan.close()
        del forms, keep
    if a.json:
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(recs, indent=1))
    if a.md:
        lines = [f"| n_kv | K / V | plan | us (spread) | attention adds, us |", "|---|---|---|---|---|"]
        for r in recs:
            if "refused" in r:
                lines.append(f"| {r['n_kv']} | {r['k/v']} | {r['what']} | refused: {r['refused']} | |")
            else:
                lines.append(f"| {r['n_kv']} | {r['k/v']} | {r['what']} | {r['us']} ({100 * r['spread']:.1f} %) | {r.get('attn_us', '')} |")
        Path(a.md).parent.mkdir(parents=True, exist_ok=True)
        Path(a.md).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
