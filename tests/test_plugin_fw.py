"""f16 / bf16 weight matrices through the plugin (libggml-mi355.so): the reference's own test-backend-ops, unmodified, drives MUL_MAT on MI355_0.
Every type_a=f16 / bf16, type_b=f32 case that ran on the old route still reports OK, none FAIL, the streaming GEMV takes nodes (the
MI355_GRAPH_STATS line counts them), and MI355_FW_STREAM=0 keeps every node on the old route with the same verdicts."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

PLUGIN = ROOT / "llama.cpp.dsp_amd" / "lib" / "libggml-mi355.so"
REF = ROOT / "oracle" / "_ref" / "avx2"

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not PLUGIN.exists() or not (REF / "test-backend-ops").exists(), reason="plugin or oracle/_ref not built")]


def _mul_mat(stream):
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN), MI355_GRAPH_STATS="1")
    env.pop("MI355_FW_STREAM", None)
    if not stream:
        env["MI355_FW_STREAM"] = "0"
    r = subprocess.run([str(REF / "test-backend-ops"), "test", "-b", "MI355_0", "-o", "MUL_MAT"], env=env, capture_output=True, text=True, timeout=1200)
    tail = r.stdout[-3000:] + r.stderr[-2000:]
    assert r.returncode == 0, tail
    assert "FAIL" not in r.stdout, tail
    counts = re.findall(r"MI355 float-weight GEMV: (\d+) MUL_MAT nodes streamed", r.stderr)
    assert counts, r.stderr[-2000:]
    cases = {}
    for l in r.stdout.splitlines():
        if l.lstrip().startswith("MUL_MAT(") and ("type_a=f16,type_b=f32" in l or "type_a=bf16,type_b=f32" in l):
            cases[l.split("):")[0]] = "OK" in l
    return cases, sum(int(c) for c in counts)


@pytest.fixture(scope="module")
def runs():
    return _mul_mat(True), _mul_mat(False)


def test_streamed_nodes_are_counted_and_pass(runs):
    (new, n_new), (old, n_old) = runs
    print(f"MUL_MAT float-weight cases: {len(new)}; ran OK {sum(new.values())} streamed route / {sum(old.values())} old route; nodes streamed {n_new} / {n_old}")
    assert n_new > 0
    assert old and sum(old.values()) > 0
    assert set(new) == set(old)
    lost = [c for c in old if old[c] and not new[c]]
    assert not lost, lost[:5]


def test_fw_stream_0_keeps_the_old_route(runs):
    _, (old, n_old) = runs
    assert n_old == 0
