"""The environment knobs of the native layer (csrc/tq_env.h): every TQ_* variable is read through
the tq_env.h functions, and INTEGRATION.md §8 documents exactly the set that the sources read."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "quantum_circuits_symmetry_breaking_based_on_tneq-qc_amd" / "csrc"
READER = re.compile(r'\benv_(?:on|opt_in|set|int|int64|double)\(\s*"(TQ_[A-Z0-9_]+)"')


def _sources():
    return sorted(p for p in CSRC.iterdir() if p.suffix in (".h", ".hip", ".cpp"))


def _section8():
    text = (ROOT / "INTEGRATION.md").read_text()
    start = text.index("## 8. Tuning knobs")
    nxt = text.find("\n## ", start + 1)
    return text[start:nxt if nxt >= 0 else len(text)]


def test_documented_knobs_are_the_knobs_read():
    read = {}
    for p in _sources():
        for name in READER.findall(p.read_text()):
            read.setdefault(name, []).append(p.name)
    assert len(read) >= 40, sorted(read)
    twice = {k: v for k, v in read.items() if len(v) != 1}
    assert not twice, f"knobs read in more than one place: {twice}"
    names = set(read) | {"TQ_TRACE_FILE"}
    documented = set()
    for line in _section8().splitlines():
        if line.startswith("| `TQ_"):
            documented |= set(re.findall(r"`(TQ_[A-Z0-9_]+)`", line.split("|")[1]))
    assert names - documented == set(), "read in csrc/ but missing from INTEGRATION.md §8"
    assert documented - names == set(), "in INTEGRATION.md §8 but read nowhere in csrc/"


def test_no_raw_getenv_outside_tq_env():
    hits = []
    for p in _sources():
        if p.name == "tq_env.h":
            continue
        for n, line in enumerate(p.read_text().splitlines(), 1):
            if 'getenv("TQ_' in line and "TQ_TRACE_FILE" not in line:
                hits.append(f"{p.name}:{n}")
    assert not hits, hits
    # the one exception reads its variable in one helper
    capi = (CSRC / "tq_capi.cpp").read_text()
    assert capi.count('getenv("TQ_TRACE_FILE")') == 1
