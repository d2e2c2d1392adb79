"""CPU-only: every environment switch the backend reads has a row in DESIGN.md's "Environment switches" table and is set
by at least one test (the switch-table counterpart of tests/test_layout_table.py).  The names are parsed out of the
sources, so a switch added later without a row or without a test fails here.  No compute calls, no library load."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approximatenn_amd", "csrc")
READ = re.compile(r'(?:getenv|env_int|env_size)\(\s*"(ANN_HIP_[A-Z0-9_]+)"')

# switches that no test sets, each with its reason; anything else the sources read must occur in a tests/test_*.py
UNTESTED = {
    "ANN_HIP_DEVICE": "selects the HIP device ordinal: the test box has one GPU, and gpu_init reads it once per process",
    "ANN_HIP_HOST_TIMING": "prints query_gpu's host timeline to stderr and changes no result; read once per process",
    "ANN_HIP_HOST_THREADS": "sizes the host thread pool when it is first used: read once per process, no result depends on it",
    "ANN_HIP_LIBDIR": "chooses the directory the loader takes the library from (A/B builds); read by _lib.py, not by the library",
}


def _text(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _load_env_body():
    src = _text(os.path.join(CSRC, "ann_host.hip"))
    start = src.index("static void load_env() {")
    return src[start:src.index("\n}\n", start)]


def switches_read():
    """{name: where it is read}: load_env()'s names, the ones ann_host.hip reads outside it, the two headers' and the
    loader's."""
    names = {n: "load_env" for n in READ.findall(_load_env_body())}
    for f in ("ann_host.hip", "ann_multi_host.h", "ann_hostpool.h"):
        for n in READ.findall(_text(os.path.join(CSRC, f))):
            names.setdefault(n, f)
    for n in re.findall(r'os\.environ\.get\(\s*"(ANN_HIP_[A-Z0-9_]+)"', _text(os.path.join(ROOT, "approximatenn_amd", "_lib.py"))):
        names.setdefault(n, "_lib.py")
    return names


def _table_names():
    """The variables of DESIGN.md's switch table: every `NAME...` in the first column of its rows."""
    doc = _text(os.path.join(ROOT, "DESIGN.md"))
    start = doc.index("### Environment switches")
    names = set()
    for line in doc[start:].splitlines()[1:]:
        if line.startswith("#"):
            break
        if line.startswith("| `"):
            names |= set(re.findall(r"`(ANN_[A-Z0-9_]+)", line.split("|")[1]))
    return names


def _names_in_tests():
    found = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "test_*.py")):
        if os.path.basename(path) != os.path.basename(__file__):
            found |= set(re.findall(r"ANN_HIP_[A-Z0-9_]+", _text(path)))
    return found


def test_the_parser_finds_the_switches():
    names = switches_read()
    assert len([n for n, w in names.items() if w == "load_env"]) >= 20, sorted(names)
    for n in ("ANN_HIP_S1_SLOTS", "ANN_HIP_DEVICE", "ANN_HIP_HOST_TIMING", "ANN_HIP_IO_PIECES", "ANN_HIP_HOST_THREADS",
              "ANN_HIP_VIRTUAL_SHARDS", "ANN_HIP_DEVICES", "ANN_HIP_FORCE_RCCL", "ANN_HIP_LIBDIR"):
        assert n in names, n


def test_every_switch_has_a_row_in_the_design_table():
    missing = sorted(set(switches_read()) - _table_names())
    assert not missing, "switches without a row in DESIGN.md's \"Environment switches\" table: %s" % missing


def test_the_design_table_names_no_switch_that_is_gone():
    gone = sorted(n for n in _table_names() if n.startswith("ANN_HIP_") and n not in switches_read())
    assert not gone, "DESIGN.md lists ANN_HIP_ switches that nothing reads: %s" % gone


def test_every_switch_is_set_by_a_test_or_exempt_with_a_reason():
    names, tested = set(switches_read()), _names_in_tests()
    assert all(len(why) > 20 for why in UNTESTED.values())
    stale = sorted(n for n in UNTESTED if n not in names)
    assert not stale, "exemptions for switches that nothing reads: %s" % stale
    untested = sorted(names - tested - set(UNTESTED))
    assert not untested, "switches that no tests/test_*.py sets: %s" % untested
