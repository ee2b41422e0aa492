"""The sweep-chain layout planner on its own (csrc/tq_sweep2_layout.cpp, linked with nothing else of
the library): `make host-check` builds probes/s2_layout_host.cpp with ASan + UBSan on the host code
and runs it on the CPU, once with the default knobs and once with lane blocks (TQ_S2_LANEBLK=1).  The
program lays out synthetic brick-wall chains for element sizes 4 / 8 / 16 and checks every accepted
descriptor: enumeration and pass limits, pass gate indices, the swizzled tile map a bijection, group
tables inside the tile, the blob size.  It fails when a kind of layout it was written for (plain block
pass, epilogue, re-listed order, one chunk) does not occur, and on any sanitizer report."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantum_circuits_symmetry_breaking_based_on_tneq-qc_amd", "csrc")


def test_layout_planner_alone_under_sanitizers():
    r = subprocess.run(["make", "-j2", "-C", CSRC, "host-check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("layouts tried")]
    assert len(lines) == 2, r.stdout[-2000:]
    assert any("lane block 0" in l for l in lines) and any("lane block 0" not in l for l in lines), lines
