"""Milliseconds per irotavg_graph_rotation_variance call (marginals + 50 pairs + scale; host time around the
synchronous call, after one warm-up call), printed as one JSON line:
  100k views / 2M edges band-only, the same with 30 / 100 / 2048 loop closures, 1M views / 20M edges band-only, the
  fixture (dense path); pairs only on 100k / 2M with 2 % random loop edges (multigrid-PCG handle). Weights are those of
  one irls (GM, 5 deg).
Usage: python tools/time_rotation_variance.py [--reps N] [--only NAME]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from irotavg_amd import capi, graphio, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402


def sequence(n, m, ncl, seed=7, p_loop=0.0):
    S = synth.make_graph(n, m, p_loop, seed=seed)
    I, QQ = S["I"], S["QQ"]
    if ncl:
        rng = np.random.default_rng(seed + 100)
        a = rng.integers(0, n - 400, size=ncl)
        b = np.minimum(a + rng.integers(200, n - a), n - 1)
        I = np.concatenate([I, np.stack([a, b], 1)])
        QQ = np.concatenate([QQ, synth.qmul(S["Qgt"][b], synth.qconj(S["Qgt"][a]))])
    return I.astype(np.int32), QQ, S["Qgt"], n, 1


def fixture():
    g = graphio.read_ravg_input(os.path.join(ROOT, "tests", "golden", "ravg_input.txt"))
    f = g["f"]
    _, Q0 = O.init_mst(g["Q"], g["QQ"], g["I"], max(g["n_abs_read"], f))
    return g["I"], g["QQ"], Q0, g["n"], f


CASES = {
    "100k_2M_band": lambda: sequence(100000, 2000000, 0),
    "100k_2M_30cl": lambda: sequence(100000, 2000000, 30),
    "100k_2M_100cl": lambda: sequence(100000, 2000000, 100),
    "100k_2M_2048cl": lambda: sequence(100000, 2000000, 2048),
    "1M_20M_band": lambda: sequence(1000000, 20000000, 0),
    "fixture": fixture,
    # multigrid-PCG handle (2 % random loop edges): pairs only
    "100k_2M_2pct_loops_pairs": lambda: sequence(100000, 2000000, 0, p_loop=0.02),
}


def time_case(name, reps):
    I, QQ, Q, n, f = CASES[name]()
    with capi.Graph(I, QQ, n, f) as G:
        G.set_rotations(Q)
        G.irls(4, 5 * np.pi / 180, 50, 1e-3)
        st = G.stats()
        ncl = G.direct_info()["closures"]
        P = np.random.default_rng(1).integers(0, n, size=(50, 2)).astype(np.int32)
        marg = st["band_block"] > 0 or n - f <= 2048
        G.rotation_variance(P, marginals=marg)  # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            G.rotation_variance(P, marginals=marg)
            ts.append(1e3 * (time.perf_counter() - t0))
    return dict(ms=round(float(np.median(ts)), 3), ms_min=round(float(np.min(ts)), 3), band_block=st["band_block"],
                closures=ncl, marginals=marg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    out = {}
    for name in CASES:
        if a.only and name not in a.only.split(","):
            continue
        out[name] = time_case(name, a.reps)
    print(json.dumps(dict(tool="time_rotation_variance", reps=a.reps, results=out)))


if __name__ == "__main__":
    main()
