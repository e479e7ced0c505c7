"""Run named cases of a test module on the decode plan's ring engine (csrc/plan_ring.hip).

The engine is chosen once per process (MI355Q_PLAN_ENGINE, read at the first mi355q_plan_create), so the cases run in ONE fresh interpreter
started with MI355Q_PLAN_ENGINE=ring.  The child imports `module` from tests/, calls module.run_ring_case(G, torch, name) per name and prints
a PASS / FAIL line each; the caller's tests assert their own line.  Before the first case the child proves which engine it got: a plan over
an IQ3_S matrix is created -- the ring engine refuses that type by name, the register engine takes it -- and an "ENGINE ring" / "ENGINE regs"
line is printed.  Nothing is launched for that.

The run ends -- the remaining names are reported as FAIL, not run -- after a plan that reports a non-zero status (a timed-out poll) and after
any exception that is not a test's own verdict (AssertionError, pytest's Failed): a HIP error surfaces as a RuntimeError, and no further GPU
work is started behind one."""
import os
import subprocess
import sys

from conftest import PKG, ROOT

CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import importlib
import numpy as np, torch
import pytest
import ggml_mi355 as G
import oracle
from qdata import random_blocks
M = importlib.import_module(sys.argv[4])

def engine():
    w = G.QWeight.from_host(oracle.IQ3_S, random_blocks(oracle.IQ3_S, 32, 2048, np.random.default_rng(0)), 32, 2048)
    x = torch.zeros((1, 2048), dtype=torch.float32, device="cuda"); y = torch.zeros((1, 32), dtype=torch.float32, device="cuda")
    try:
        G.Plan([dict(ws=[w], ys=[y], x=x)]).close()
        return "regs"
    except G.Mi355qError as e:
        return "ring" if "the ring engine does not stream IQ3_S" in str(e) else "unknown: " + str(e)[:200]
print("ENGINE", engine(), flush=True)

# a plan that reports a non-zero status (a timed-out poll) ends the run: no further GPU work after it
aborted = []
_status = G.Plan.status
def _watched_status(self):
    st = _status(self)
    if st != 0:
        aborted.append("an earlier plan reported status %d" % st)
    return st
G.Plan.status = _watched_status

names = sys.argv[5].split(",")
for i, name in enumerate(names):
    try:
        r = M.run_ring_case(G, torch, name)
        print("PASS", name, "" if r is None else f"{r:.3e}", flush=True)
    except (AssertionError, pytest.fail.Exception) as e:
        print("FAIL", name, type(e).__name__, str(e)[:400].replace(chr(10), " "), flush=True)
    except BaseException as e:
        print("FAIL", name, type(e).__name__, str(e)[:400].replace(chr(10), " "), flush=True)
        aborted.append("an earlier case raised " + type(e).__name__)
    if aborted:
        for rest in names[i + 1:]:
            print("FAIL", rest, "not run:", aborted[0], flush=True)
        break
"""


def run_ring_cases(module: str, names, timeout: int = 900):
    """-> (return code, {name: its PASS / FAIL line}, the end of stderr, the engine the child found)."""
    env = dict(os.environ, MI355Q_PLAN_ENGINE="ring")
    r = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), str(PKG), str(ROOT / "tests"), module, ",".join(names)], env=env,
                       capture_output=True, text=True, timeout=timeout)
    lines, engine = {}, None
    for ln in r.stdout.splitlines():
        parts = ln.split(" ", 2)
        if len(parts) >= 2 and parts[0] in ("PASS", "FAIL"):
            lines[parts[1]] = ln
        elif parts[0] == "ENGINE":
            engine = ln[len("ENGINE "):]
    print(r.stdout[-4000:])
    return r.returncode, lines, r.stderr[-3000:], engine
