"""Records tests/golden/route_bits.json: what three IRLS iterations return, to the bit, on every route through the host
code of the banded direct solver (irotavg_amd/csrc/bcr.hip). tests/test_gpu_route_bits.py compares a later build with it.

A case is a small shape of tests/band_cases.py or tests/closure_cases.py with the environment switches that case carries
(plus IROTAVG_BCR_NO_UNIT_FACTOR where named here). Per case one fresh handle makes `calls` irls calls of three iterations
from the case's start rotations: the first solve of the first call fills the unit-weight store where the route keeps one,
the first solve of the second call is served from it. Recorded per call: iteration count, the score trace, SHA-256 of the
rotations and of the weights, direct_info() and the integer counters of stats().

Every case is recorded twice on fresh handles. A case whose two records differ is not deterministic: it is written as
{"nondeterministic": "<what differed>"} and the test leaves it out.

Needs a GPU and the built library. Reads nothing outside the repository.

Usage: python tests/golden/make_route_bits.py [output.json]
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (os.path.dirname(TESTS), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

SIGMA = 5 * np.pi / 180
NO_UNIT = {"IROTAVG_BCR_NO_UNIT_FACTOR": "1"}
# (name, "band" / "closure", the case of that module, extra environment, irls calls)
SPECS = [
    ("plain-b8", "band", "up-b8-nb129-s", {}, 2),              # assembling level 0, the upper launch; fill, then served
    ("plain-b16", "band", "up-b16-nb129-s", {}, 2),
    ("plain-b24", "band", "up-b24-nb129-s", {}, 2),
    ("plain-b8-4levels", "band", "up-b8-nb1025-u", {}, 2),
    ("no-unit-factor-b8", "band", "up-b8-nb129-s", NO_UNIT, 2),
    ("no-fused-asm-b8", "band", "switch-nofusedasm", {}, 2),   # K3 in a launch of its own: no store either
    ("up-cap-0-b8", "band", "switch-upcap0", {}, 2),           # a refused reservation: level by level
    ("no-top16-b8", "band", "switch-notop16", {}, 2),
    ("mixed-b8", "band", "mixed-b8", {}, 2),
    ("mixed-b32", "band", "mixed-b32", {}, 1),
    ("top16-b12", "band", "top16-b12-nb128", {}, 1),           # two levels, the single-workgroup top alone
    ("top16-b24", "band", "top16-b24-nb73", {}, 1),
    ("sep-b32", "band", "sep-b32-nb65", {}, 1),                # three levels, each a launch of its own
    ("two-b8", "band", "two-b8-nb9", {}, 1),                   # a top of two blocks
    ("one-b8", "band", "one-b8-63-u", {}, 1),                  # level 0 is the top
    ("closures-b8", "closure", "up-b8-nb129", {}, 1),
    ("closures-b16-two", "closure", "two-b16-nb9", {}, 1),
    ("closures-b32-wide", "closure", "wide-b32-cl", {}, 1),
]
STAT_KEYS = ("band_block", "direct_solves", "pcg_solves", "direct_up_fallbacks", "direct_guarded", "direct_dead_pivots",
             "outer_iters")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def case_of(kind, name):
    if kind == "band":
        import band_cases as M
    else:
        import closure_cases as M
    return M.CASE[name]


def record(spec):
    """The record of one spec on a fresh handle (what the test recomputes)."""
    from irotavg_amd import capi
    _, kind, cname, extra, calls = spec
    c = case_of(kind, cname)
    env = dict(c["env"] or {})
    env.update(extra)
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                                     # (handle-scope switches, read at creation)
    try:
        G = capi.Graph(c["I"], c["QQ"], c["n"], c["f"], band_direct=1)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    out = []
    with G:
        for _ in range(calls):
            G.set_rotations(c["Q0"])
            r = G.irls(4, SIGMA, 3, 1e-6)
            st = G.stats()
            out.append(dict(iters=int(r["iters"]), scores=[float(s).hex() for s in r["scores"]], Q=sha(G.get_rotations()),
                            w=sha(G.get_weights()), info=G.direct_info(), stats={k: int(st[k]) for k in STAT_KEYS}))
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "route_bits.json")
    doc = {}
    for spec in SPECS:
        a, b = record(spec), record(spec)
        if a == b:
            doc[spec[0]] = a
        else:
            what = sorted({k for x, y in zip(a, b) for k in x if x[k] != y[k]})
            doc[spec[0]] = {"nondeterministic": "two records on fresh handles differ in " + ", ".join(what)}
        print(spec[0], "ok" if a == b else doc[spec[0]], flush=True)
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
