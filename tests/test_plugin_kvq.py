"""A Q4_1 / Q5_0 / Q5_1 / IQ4_NL KV cache through the plugin (libggml-mi355.so), with the reference's own tools built under oracle/_ref.

  * test-backend-ops -o CPY: every `f32 -> q4_1 / q5_0 / q5_1 / iq4_nl` case runs on MI355_0 and passes the harness' check against the ggml CPU
    backend, none "not supported"; -o MUL_MAT keeps every type_a=iq4_nl case (an IQ4_NL tensor outside a weight buffer now keeps canonical rows and
    is packed before a plain MUL_MAT, as Q8_0 / Q4_0 are).  The harness has no FLASH_ATTN_EXT cases for these types: tests/test_gpu_kvq.py and
    tests/test_kvq_golden.py carry that weight.
  * llama-bench -ngl 99 -fa 1 -ctk T -ctv T on a small synthetic model: every decode token the f16 cache runs as one persistent launch runs as one
    here too, with as many MI355 graph_compute calls; MI355_PLAN_DEBUG names the type and strides consistent with its block size.
  * llama-bench -fa 0 -ctk T (quantized K read by a plain MUL_MAT over a view of the cache, f16 V): stays resident -- as many graph_compute calls
    reach the MI355 backend as with an f16 cache (a node the backend declined would split every layer's graph and add calls); it is not planned.
    q8_0 / q4_0 are held to the same (before the cache-view form of the MUL_MAT they were split: 95 calls against 19 on this model)."""
import json
import os
import re
import subprocess
from pathlib import Path

import pytest

from conftest import ROOT

PLUGIN = ROOT / "llama.cpp.dsp_amd" / "lib" / "libggml-mi355.so"
REF = ROOT / "oracle" / "_ref" / "avx2"
BB = {"q4_1": 20, "q5_0": 22, "q5_1": 24, "iq4_nl": 18}
KVS = list(BB)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not PLUGIN.exists() or not (REF / "llama-bench").exists() or not (REF / "test-backend-ops").exists(),
                                 reason="plugin or oracle/_ref not built")]


def _backend_ops(op):
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN))
    r = subprocess.run([str(REF / "test-backend-ops"), "test", "-b", "MI355_0", "-o", op], env=env, capture_output=True, text=True, timeout=1200)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    assert "FAIL" not in r.stdout, tail
    return [l for l in r.stdout.splitlines() if l.lstrip().startswith(op + "(")]


def test_cpy_f32_to_the_cache_types_runs():
    cases = _backend_ops("CPY")
    for kv in KVS:
        mine = [l for l in cases if f"type_src=f32,type_dst={kv}," in l]
        print(f"CPY f32 -> {kv}: {len(mine)} cases, {sum('OK' in l for l in mine)} ran and passed")
        assert mine, kv
        assert all("OK" in l and "not supported" not in l for l in mine), [l for l in mine if "OK" not in l][:5]


def test_mul_mat_iq4_nl_cases_still_run():
    """No iq4_nl case is lost.  A proxy, not a comparison with a recorded run of the parent: every iq4_nl case runs and passes whose q4_0 twin (the
    same case with type_a=q4_0: the type that has always kept canonical rows outside a weight buffer and is packed the same way) runs, and the plain
    f32 cases all do.  Measured with this harness: 11 iq4_nl cases, 11 ran and passed, none "not supported"."""
    all_cases = _backend_ops("MUL_MAT")
    cases = [l for l in all_cases if "type_a=iq4_nl," in l]
    ran = [l for l in cases if "OK" in l]
    key = lambda l, t: re.sub(r"\x1b\[[0-9;]*m", "", l).split("):")[0].replace(f"type_a={t},", "type_a=T,")
    twins_ok = {key(l, "q4_0") for l in all_cases if "type_a=q4_0," in l and "OK" in l}
    print(f"MUL_MAT type_a=iq4_nl: {len(cases)} cases, {len(ran)} ran and passed, {sum('not supported' in l for l in cases)} not supported")
    plain = [l for l in cases if "type_b=f32" in l and "per=[0,1,2,3]" in l and "v=0" in l]
    assert plain and all("OK" in l for l in plain), [l for l in plain if "OK" not in l][:5]
    lost = [l for l in cases if "OK" not in l and key(l, "iq4_nl") in twins_ok]
    assert not lost, lost[:5]


@pytest.fixture(scope="module")
def small_gguf(tmp_path_factory):
    synth = REF / "gguf_synth"
    if not synth.exists():
        pytest.skip("oracle/_ref/avx2 gguf_synth not built")
    out = tmp_path_factory.mktemp("kvq") / "small_q4_k_m.gguf"
    r = subprocess.run([str(synth), "--preset", "small", "--ftype", "q4_k_m", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return out


def _bench(gguf: Path, ctk: str, ctv: str, fa: str = "1", debug: bool = False):
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), MI355_GRAPH_STATS="1")
    if debug:
        env["MI355_PLAN_DEBUG"] = "1"
    cmd = [str(REF / "llama-bench"), "-m", str(gguf), "-p", "64", "-n", "16", "-r", "1", "-ngl", "99", "-t", "4", "-fa", fa, "-ctk", ctk, "-ctv", ctv, "-o", "json"]
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
    return _bench(small_gguf, "f16", "f16")


@pytest.mark.parametrize("ctk", KVS)
def test_llama_bench_cache_is_planned(small_gguf, f16_run, ctk):
    rows, calls, planned, built, _ = _bench(small_gguf, ctk, ctk)
    _, calls_f16, planned_f16, built_f16, _ = f16_run
    print(f"-fa 1 -ctk {ctk}: {calls} MI355 graph_compute calls, {planned} planned, {built} plans built ({[round(r['avg_ts'], 1) for r in rows]} tok/s); "
          f"f16 cache: {calls_f16} calls, {planned_f16} planned, {built_f16} built")
    assert planned_f16 > 0
    assert built >= 1
    assert planned == planned_f16, (planned, planned_f16)      # every decode token the f16 cache plans is planned here too
    assert calls == calls_f16, (calls, calls_f16)


@pytest.mark.parametrize("ctk", KVS)
def test_plan_debug_reports_the_cache_type_and_strides(small_gguf, ctk):
    _, _, planned, _, err = _bench(small_gguf, ctk, ctk, debug=True)
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


@pytest.fixture(scope="module")
def f16_noflash_run(small_gguf):
    return _bench(small_gguf, "f16", "f16", fa="0")


@pytest.mark.parametrize("ctk", KVS + ["q8_0", "q4_0"])
def test_llama_bench_no_flash_quantized_k_stays_resident(small_gguf, f16_noflash_run, ctk):
    rows, calls, planned, _, _ = _bench(small_gguf, ctk, "f16", fa="0")
    _, calls_f16, planned_f16, _, _ = f16_noflash_run
    print(f"-fa 0 -ctk {ctk}: {calls} graph_compute calls reached MI355, {planned} planned ({[round(r['avg_ts'], 1) for r in rows]} tok/s); f16: {calls_f16} calls, {planned_f16} planned")
    assert calls == calls_f16, (calls, calls_f16)              # no node declined: the graphs are not split
