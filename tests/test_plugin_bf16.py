"""A bf16 KV cache through the plugin (libggml-mi355.so): the reference's own harnesses, unmodified, drive it.

  * test-backend-ops: every FLASH_ATTN_EXT case with type_KV=bf16, every MUL_MAT case with type_a=bf16 (f32 src1, plain layout) and every CPY
    case among f32 / f16 / bf16 runs on MI355_0 and passes the harness' NMSE check against the ggml CPU backend (none "not supported").
  * llama-bench -ngl 99 -ctk bf16 -ctv bf16, with -fa 1 and -fa 0, on a small synthetic model: the graph is not split around the attention
    (the MI355 backend sees as many graph_compute calls as with an f16 cache) and no decode plan is built (the plan has no bf16 attention stage)."""
import json
import os
import re
import subprocess
from pathlib import Path

import pytest

import oracle
from conftest import ROOT

PLUGIN = ROOT / "llama.cpp.dsp_amd" / "lib" / "libggml-mi355.so"
REF = ROOT / "oracle" / "_ref" / "avx2"

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not PLUGIN.exists() or not (REF / "test-backend-ops").exists(), reason="plugin or oracle/_ref not built")]


def _backend_ops(op):
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN))
    r = subprocess.run([str(REF / "test-backend-ops"), "test", "-b", "MI355_0", "-o", op], env=env, capture_output=True, text=True, timeout=1200)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    assert "FAIL" not in r.stdout, tail
    return [l for l in r.stdout.splitlines() if l.lstrip().startswith(op + "(")]


def test_flash_attn_ext_bf16_cases_run():
    cases = [l for l in _backend_ops("FLASH_ATTN_EXT") if "type_KV=bf16" in l]
    print(f"FLASH_ATTN_EXT type_KV=bf16: {len(cases)} cases")
    assert len(cases) >= 100 and all("OK" in l for l in cases), [l for l in cases if "OK" not in l][:5]


def test_mul_mat_bf16_cases_run():
    cases = [l for l in _backend_ops("MUL_MAT") if "type_a=bf16,type_b=f32" in l]
    plain = [l for l in cases if "per=[0,1,2,3]" in l and "v=0" in l]
    print(f"MUL_MAT type_a=bf16,type_b=f32: {len(cases)} cases, {sum('OK' in l for l in cases)} ran")
    assert plain and all("OK" in l for l in plain), [l for l in plain if "OK" not in l][:5]


def test_cpy_bf16_cases_run():
    types = ("f32", "f16", "bf16")
    cases = [l for l in _backend_ops("CPY") if "bf16" in l]
    mine = [l for l in cases if re.search(r"type_src=(\w+)", l) and re.search(r"type_src=(\w+)", l).group(1) in types
            and re.search(r"type_dst=(\w+)", l) and re.search(r"type_dst=(\w+)", l).group(1) in types]
    print(f"CPY among f32/f16/bf16 with a bf16 side: {len(mine)} cases")
    assert mine and all("OK" in l for l in mine), [l for l in mine if "OK" not in l][:5]


# ---------------------------------------------------------------- llama-bench

@pytest.fixture(scope="module")
def small_gguf(tmp_path_factory):
    synth = REF / "gguf_synth"
    if not (synth.exists() and (REF / "llama-bench").exists()):
        pytest.skip("oracle/_ref/avx2 llama-bench / gguf_synth not built")
    out = tmp_path_factory.mktemp("bf16kv") / "small_q4_k_m.gguf"
    r = subprocess.run([str(synth), "--preset", "small", "--ftype", "q4_k_m", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return out


def _bench(gguf: Path, ctk: str, fa: str):
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), MI355_GRAPH_STATS="1")
    cmd = [str(REF / "llama-bench"), "-m", str(gguf), "-p", "64", "-n", "16", "-r", "1", "-ngl", "99", "-t", "4", "-fa", fa, "-ctk", ctk, "-ctv", ctk, "-o", "json"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    rows = json.loads(r.stdout[r.stdout.index("["):])
    calls = sum(sum(map(int, m)) for m in re.findall(r"MI355 graph_compute calls: (\d+) eager, (\d+) captured, (\d+) replayed", r.stderr))
    plans = re.findall(r"MI355 decode plans: (\d+) graph_compute calls ran as one persistent launch, (\d+) plans built", r.stderr)
    assert plans, r.stderr[-2000:]
    planned, built = sum(int(a) for a, _ in plans), sum(int(b) for _, b in plans)
    return rows, calls + planned, built


@pytest.mark.parametrize("fa", ["1", "0"])
def test_llama_bench_bf16_cache_stays_resident(small_gguf, fa):
    rows, calls, built = _bench(small_gguf, "bf16", fa)
    _, calls_f16, _ = _bench(small_gguf, "f16", fa)
    print(f"-fa {fa}: bf16 cache {calls} MI355 graph_compute calls ({[round(r['avg_ts'], 1) for r in rows]} tok/s), f16 cache {calls_f16}; {built} plans built")
    assert calls == calls_f16, (calls, calls_f16)          # (a split graph would add MI355 graph_compute calls around every layer's attention)
    assert built == 0
