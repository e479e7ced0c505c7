"""A mixed KV cache (-ctk A -ctv B) through the plugin (libggml-mi355.so), with the reference's llama-bench built under oracle/_ref.

llama-bench -ngl 99 -fa 1 -p 64 -n 16 -r 1 on the small synthetic model: with -ctk q8_0 -ctv q4_0 and -ctk f16 -ctv q8_0 as many graph_compute calls
reach the MI355 backend as with an f16 cache -- no FLASH_ATTN_EXT node is declined, so no graph is split (a declined node in every layer adds calls).
The decode plan declines such a cache (a mixed plan stage is not built), so these graphs run node by node: the count is calls + planned of the f16 run.
With MI355_FA_KV_MIXED=0 the plugin refuses the nodes as it did before, and the count differs."""
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
    out = tmp_path_factory.mktemp("kvmix") / "small_q4_k_m.gguf"
    r = subprocess.run([str(synth), "--preset", "small", "--ftype", "q4_k_m", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return out


def _bench(gguf: Path, ctk: str, ctv: str, mixed=None):
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), MI355_GRAPH_STATS="1")
    env.pop("MI355_FA_KV_MIXED", None)
    if mixed is not None:
        env["MI355_FA_KV_MIXED"] = mixed
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
def test_llama_bench_mixed_cache_stays_resident(small_gguf, f16_run, ctk, ctv):
    rows, calls, planned = _bench(small_gguf, ctk, ctv)
    _, calls_f16, planned_f16 = f16_run
    print(f"-fa 1 -ctk {ctk} -ctv {ctv}: {calls} graph_compute calls reached MI355, {planned} planned ({[round(r['avg_ts'], 1) for r in rows]} tok/s); "
          f"f16 cache: {calls_f16} calls, {planned_f16} of them planned")
    assert calls == calls_f16, (calls, calls_f16)              # no node declined: the graphs are not split
    assert planned == 0                                        # the plan matcher declines a cache whose V type differs from K's


def test_switch_restores_the_refusal(small_gguf, f16_run):
    _, calls, _ = _bench(small_gguf, "q8_0", "q4_0", mixed="0")
    _, calls_f16, _ = f16_run
    print(f"-fa 1 -ctk q8_0 -ctv q4_0 with MI355_FA_KV_MIXED=0: {calls} graph_compute calls reached MI355; f16 cache: {calls_f16}")
    assert calls != calls_f16, (calls, calls_f16)              # every layer's graph is split around the declined node
