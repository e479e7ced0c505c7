"""A Q8_0 / Q4_0 KV cache with flash attention through the plugin (libggml-mi355.so): the decode plan takes it.

llama-bench -ngl 99 -fa 1 -ctk {q8_0,q4_0} -ctv same on a small synthetic model: every decode token runs as one persistent launch, as many as with an
f16 cache; the MI355 backend sees as many graph_compute calls as with an f16 cache; and under MI355_PLAN_DEBUG the attention stages report the cache
type and the strides of the model's cache (k_nb_pos = n_embd_kv / 32 * BB, k_nb_head = head_dim / 32 * BB, v_nb_dim = BB; BB = 34 or 18).
The numbers of the stage are pinned in tests/test_gpu_plan_quant_kv.py (bit for bit against the reference's FLASH_ATTN_EXT at one split)."""
import json
import os
import re
import subprocess
from pathlib import Path

import pytest

from conftest import ROOT

PLUGIN = ROOT / "llama.cpp.dsp_amd" / "lib" / "libggml-mi355.so"
REF = ROOT / "oracle" / "_ref" / "avx2"
BB = {"q8_0": 34, "q4_0": 18}

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not PLUGIN.exists() or not (REF / "llama-bench").exists(), reason="plugin or oracle/_ref not built")]


@pytest.fixture(scope="module")
def small_gguf(tmp_path_factory):
    synth = REF / "gguf_synth"
    if not synth.exists():
        pytest.skip("oracle/_ref/avx2 gguf_synth not built")
    out = tmp_path_factory.mktemp("quantkv") / "small_q4_k_m.gguf"
    r = subprocess.run([str(synth), "--preset", "small", "--ftype", "q4_k_m", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return out


def _bench(gguf: Path, ctk: str, debug: bool = False):
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), MI355_GRAPH_STATS="1")
    if debug:
        env["MI355_PLAN_DEBUG"] = "1"
    cmd = [str(REF / "llama-bench"), "-m", str(gguf), "-p", "64", "-n", "16", "-r", "1", "-ngl", "99", "-t", "4", "-fa", "1", "-ctk", ctk, "-ctv", ctk, "-o", "json"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    rows = json.loads(r.stdout[r.stdout.index("["):])
    calls = sum(sum(map(int, m)) for m in re.findall(r"MI355 graph_compute calls: (\d+) eager, (\d+) captured, (\d+) replayed", r.stderr))
    plans = re.findall(r"MI355 decode plans: (\d+) graph_compute calls ran as one persistent launch, (\d+) plans built", r.stderr)
    assert plans, r.stderr[-2000:]
    planned, built = sum(int(a) for a, _ in plans), sum(int(b) for _, b in plans)
    return rows, calls + planned, planned, built, r.stderr


@pytest.fixture(scope="module")
def f16_run(small_gguf):
    return _bench(small_gguf, "f16")


@pytest.mark.parametrize("ctk", ["q8_0", "q4_0"])
def test_llama_bench_quantized_cache_is_planned(small_gguf, f16_run, ctk):
    rows, calls, planned, built, _ = _bench(small_gguf, ctk)
    _, calls_f16, planned_f16, built_f16, _ = f16_run
    print(f"-fa 1 -ctk {ctk}: {calls} MI355 graph_compute calls, {planned} planned, {built} plans built ({[round(r['avg_ts'], 1) for r in rows]} tok/s); "
          f"f16 cache: {calls_f16} calls, {planned_f16} planned, {built_f16} built")
    assert planned_f16 > 0
    assert built >= 1
    assert planned == planned_f16, (planned, planned_f16)      # every decode token the f16 cache plans is planned here too
    assert calls == calls_f16, (calls, calls_f16)


@pytest.mark.parametrize("ctk", ["q8_0", "q4_0"])
def test_plan_debug_reports_the_cache_type_and_strides(small_gguf, ctk):
    _, _, planned, _, err = _bench(small_gguf, ctk, debug=True)
    lines = [l for l in err.splitlines() if l.startswith("MI355 plan attn:")]
    assert planned > 0 and lines, err[-3000:]
    bb = BB[ctk]
    for l in lines:
        m = re.search(r"n_head_kv (\d+) hd (\d+) .*\| kv (\w+) \| k_cache \S+ nb_pos (\d+) nb_head (\d+) \| v_cache \S+ nb_pos (\d+) nb_dim (\d+) nb_head (\d+)", l)
        assert m, l
        n_head_kv, hd, kv, k_pos, k_head, v_pos, v_dim, v_head = m.groups()
        n_head_kv, hd = int(n_head_kv), int(hd)
        assert kv == ctk, l
        assert int(k_pos) == n_head_kv * hd // 32 * bb and int(k_head) == hd // 32 * bb, l
        assert int(v_pos) == n_head_kv * hd // 32 * bb and int(v_head) == hd // 32 * bb and int(v_dim) == bb, l
