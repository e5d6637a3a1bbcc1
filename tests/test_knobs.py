"""CPU: the library reads its environment knobs through one accessor, and INTEGRATION.md lists exactly the knobs of
the library's table (csrc/kmcf_knobs.hpp)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "accelerated-kinetic-monte-carlo-simulations-of-atomistically-resolved-resistive-memory-arrays_amd", "csrc")


def _table():
    src = open(os.path.join(CSRC, "kmcf_knobs.hpp")).read()
    body = src[src.index("kmcf_knobs[] = {"):]
    body = body[:body.index("};")]
    return re.findall(r'\{KNOB_(\w+),\s*"(KMCF_\w+)"', body)


def test_getenv_only_in_the_accessor():
    hits = []
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".hpp", ".h", ".cpp")):
            continue
        for line in open(os.path.join(CSRC, f)):
            if "getenv" in line:
                hits.append((f, line.strip()))
    assert hits == [("kmcf_knobs.hpp", "inline const char *kmcf_knob(kmcf_knob_id k) { return getenv(kmcf_knobs[k].name); }")], hits


def test_table_entries_are_consistent():
    entries = _table()
    assert len(entries) >= 30
    assert all(name == "KMCF_" + knob for knob, name in entries), entries
    assert len({name for _, name in entries}) == len(entries)


def test_integration_lists_the_table():
    table = {name for _, name in _table()}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    listed = re.findall(r"^\| `(KMCF_\w+)` \|", doc, flags=re.M)
    assert len(listed) == len(set(listed)), listed
    assert set(listed) == table, (sorted(set(listed) - table), sorted(table - set(listed)))
    assert "KMCF_LIB_PATH" not in table and "`KMCF_LIB_PATH`" in doc
