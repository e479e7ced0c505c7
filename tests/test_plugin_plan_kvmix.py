"""The decode plan over a mixed KV cache (-ctk A -ctv B) through the plugin (libggml-mi355.so), with the reference's llama-bench built under oracle/_ref.

llama-bench -ngl 99 -fa 1 -p 64 -n 16 -r 1 on the small synthetic model, built exactly as tests/test_plugin_kvmix.py builds it.  The plan matcher takes K and V
views of different types only with MI355_PLAN_KV_MIXED=1 (off by default: DESIGN.md 5.6): then -ctk q8_0 -ctv q4_0 and -ctk f16 -ctv q8_0 report as many
graph_compute calls as the f16 run, and as many of them planned (one persistent launch per token) as the f16 run, which is above 0.  With the variable set
to 0 they run node by node as without it: planned == 0 and the same call count.  One process per run, each under its own time limit."""
import json
import os
import re
import subprocess
from pathlib import Path

import pytest

from conftest import ROOT

PLUGIN = ROOT / "llama.cpp.dsp_amd" / "lib" / "libggml-mi355.so"
REF = ROOT / "oracle" / "_ref" / "avx2"
PAIRS = [("q8_0", "q4_0"), ("f16", "q8_0")]

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not PLUGIN.exists() or not (REF / "llama-bench").exists(), reason="plugin or oracle/_ref not built")]


@pytest.fixture(scope="module")
def small_gguf(tmp_path_factory):
    synth = REF / "gguf_synth"
    if not synth.exists():
        pytest.skip("oracle/_ref/avx2 gguf_synth not built")
    out = tmp_path_factory.mktemp("plan_kvmix") / "small_q4_k_m.gguf"
    r = subprocess.run([str(synth), "--preset", "small", "--ftype", "q4_k_m", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return out


def _bench(gguf: Path, ctk: str, ctv: str, plan_mixed=None):
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), MI355_GRAPH_STATS="1")
    env.pop("MI355_PLAN_KV_MIXED", None); env.pop("MI355_FA_KV_MIXED", None)
    if plan_mixed is not None:
        env["MI355_PLAN_KV_MIXED"] = plan_mixed
    cmd = [str(REF / "llama-bench"), "-m", str(gguf), "-p", "64", "-n", "16", "-r", "1", "-ngl", "99", "-t", "4", "-fa", "1", "-ctk", ctk, "-ctv", ctv, "-o", "json"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    rows = json.loads(r.stdout[r.stdout.index("["):])
    calls = sum(sum(map(int, m)) for m in re.findall(r"MI355 graph_compute calls: (\d+) eager, (\d+) captured, (\d+) replayed", r.stderr))
    plans = re.findall(r"MI355 decode plans: (\d+) graph_compute calls ran as one persistent launch, (\d+) plans built", r.stderr)
    assert plans, r.stderr[-2000:]
    planned = sum(int(a) for a, _ in plans)
    return rows, calls + planned, planned


@pytest.fixture(scope="module")
def f16_run(small_gguf):
    return _bench(small_gguf, "f16", "f16")


@pytest.mark.parametrize("ctk,ctv", PAIRS, ids=[f"{k}-{v}" for k, v in PAIRS])
def test_mixed_cache_is_planned_with_the_switch(small_gguf, f16_run, ctk, ctv):
    rows, calls, planned = _bench(small_gguf, ctk, ctv, plan_mixed="1")
    _, calls_f16, planned_f16 = f16_run
    print(f"MI355_PLAN_KV_MIXED=1 -fa 1 -ctk {ctk} -ctv {ctv}: {calls} graph_compute calls reached MI355, {planned} planned "
          f"({[round(r['avg_ts'], 1) for r in rows]} tok/s); f16 cache: {calls_f16} calls, {planned_f16} of them planned")
    assert planned_f16 > 0
    assert calls == calls_f16, (calls, calls_f16)
    assert planned == planned_f16, (planned, planned_f16)


def test_switch_at_zero_keeps_the_node_path(small_gguf, f16_run):
    _, calls, planned = _bench(small_gguf, "q8_0", "q4_0", plan_mixed="0")
    _, calls_f16, _ = f16_run
    print(f"MI355_PLAN_KV_MIXED=0 -fa 1 -ctk q8_0 -ctv q4_0: {calls} graph_compute calls reached MI355, {planned} planned; f16 cache: {calls_f16}")
    assert planned == 0
    assert calls == calls_f16, (calls, calls_f16)
