"""tq_plan_query "tables_digest": FNV-1a-64 over what the device reads of a compiled plan (gather
tables, descriptor blobs, the ops' launch fields).  It must not depend on the process (no padding
or pointer reaches it), and it must see a planner change that the describe text and the other
query keys can miss -- here TQ_S2_REORDER, which re-lists C2's chains (test_reorder_cpu.py: fewer
passes on C2).  Compile-only; the knob is read once per process, so every compile is a child."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from tneq_qc_amd.circuits import config_task
from tneq_qc_amd.expression import HipContractExpression
t = config_task("C2")
p = HipContractExpression(t.eq, *t.shapes, optimize=t.path, slices=t.sliced).plan(torch.complex64)
print(p.query("tables_digest"), p.query("whole_tables_digest"))
"""


def _digests(*reorder):
    """one child process per TQ_S2_REORDER value, side by side"""
    procs = [subprocess.Popen([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, TQ_S2_REORDER=v),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for v in reorder]
    out = []
    for p in procs:
        so, se = p.communicate(timeout=300)
        assert p.returncode == 0, se[-2000:]
        out.append([int(v) for v in so.strip().splitlines()[-1].split()])
    return out


def test_tables_digest_is_stable_and_sees_the_relisting():
    a, b, off = _digests("1", "1", "0")
    assert a[0] > 0 and a == b           # two processes, one value
    assert a[1] == -1                    # C2 has no sliced modes: no whole program
    assert off[0] > 0 and off[0] != a[0]
