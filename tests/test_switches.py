"""The IROTAVG_* environment switches live in ONE module (irotavg_amd/csrc/switches.hpp): the only place of the product
that calls getenv and the only place that spells a switch's name in code. Read from the sources -- no build, no GPU."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "irotavg_amd", "csrc")
MODULE = os.path.join(CSRC, "switches.hpp")

# withdrawn with their experiments (the parent of this change and docs/history/ are the record)
REMOVED = ["BCR_FORWARD8", "CG2_FP32_DENSE", "CG2_SLICES", "L1_THREADS_PER_ITERATION", "AT_MUL_CLASSIC", "STALE_SPREAD",
           "INEXACT_RTOL", "BCR_BLOCK", "DIST_DEBUG", "BCR_FORWARD_WAVE", "BCR_NARROW", "BCR_NO_FUSED_UP",
           "BCR_NO_FUSED_BACK", "BCR_NO_APPLY", "NO_FUSED_WR", "NO_LAST_GUESS", "GJ_NO_LOOKAHEAD", "NO_HOST_POOL",
           "BCR_NO_RESIDUAL_GATE"]


def read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def product_sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*")))
    files += sorted(glob.glob(os.path.join(ROOT, "include", "**", "*.h*"), recursive=True))
    files += sorted(glob.glob(os.path.join(ROOT, "tools", "*.cpp")))
    return [f for f in files if os.path.isfile(f) and f.endswith((".hip", ".cpp", ".hpp", ".h"))]


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def table():
    """The names read_switches() and the process-wide readers of the module pass to getenv."""
    names = set(re.findall(r'"IROTAVG_([A-Z0-9_]+)"', strip_comments(read(MODULE))))
    assert len(names) >= 30, names
    return names


def test_getenv_and_switch_names_occur_in_the_one_module_only():
    assert MODULE in product_sources()
    for path in product_sources():
        if path == MODULE:
            continue
        code = strip_comments(read(path))
        assert "getenv" not in code, path
        assert not re.findall(r'"[^"\n]*IROTAVG_[A-Z][^"\n]*"', code), path
    # the module itself: every getenv is given a literal name (`name`: the two small readers, fed literals only)
    code = strip_comments(read(MODULE))
    calls = re.findall(r"getenv\(([^)]*)\)", code)
    assert calls and all(re.fullmatch(r'"IROTAVG_[A-Z0-9_]+"|name', c.strip()) for c in calls), calls


def test_every_switch_that_is_set_or_documented_is_in_the_table():
    names = table()
    used = set()
    setters = [r'environ\[\s*"IROTAVG_([A-Z0-9_]+)"\s*\]\s*=', r'env\[\s*"IROTAVG_([A-Z0-9_]+)"\s*\]\s*=',
               r'setenv\(\s*"IROTAVG_([A-Z0-9_]+)"', r'delenv\(\s*"IROTAVG_([A-Z0-9_]+)"',
               r'\.pop\(\s*"IROTAVG_([A-Z0-9_]+)"', r'\bIROTAVG_([A-Z0-9_]+)=["\']?[-0-9]',
               r'[{,(]\s*"IROTAVG_([A-Z0-9_]+)"\s*[:,)]']
    files = [os.path.join(ROOT, "bench.py")]
    for sub in ("tests", "tools"):
        for ext in ("*.py", "*.sh", "*.cpp"):
            files += glob.glob(os.path.join(ROOT, sub, "**", ext), recursive=True)
    for path in files:
        if os.path.abspath(path) == os.path.abspath(__file__):
            continue
        text = read(path)
        for pat in setters:
            used.update(re.findall(pat, text))
    used.discard("BENCH_SHARE_GPU")  # bench.py's own: the library never reads it
    assert len(used) >= 20 and used <= names, sorted(used - names)
    # documented: a row of README.md's table, IROTAVG_X=... in the prose of the public header
    documented = set(re.findall(r"^\|\s*`IROTAVG_([A-Z0-9_]+)", read(os.path.join(ROOT, "README.md")), flags=re.M))
    documented.update(re.findall(r"\bIROTAVG_([A-Z0-9_]+)=", read(os.path.join(ROOT, "include", "irotavg_hip.h"))))
    assert documented and documented <= names, sorted(documented - names)


def test_every_switch_of_the_table_is_in_the_readme_table():
    rows = re.findall(r"^\|\s*`IROTAVG_([A-Z0-9_]+)[^|]*\|\s*(handle|sharded handle|view-graph|process)\s*\|",
                      read(os.path.join(ROOT, "README.md")), flags=re.M)
    assert table() == {name for name, _scope in rows}, sorted(table() ^ {name for name, _scope in rows})


def test_withdrawn_switches_are_gone():
    assert not set(REMOVED) & table()
    docs = [os.path.join(ROOT, "README.md"), os.path.join(ROOT, "INTEGRATION.md")]
    for path in product_sources() + docs:
        text = read(path)
        for name in REMOVED:
            assert not re.search(r"IROTAVG_%s\b" % name, text), (path, name)
