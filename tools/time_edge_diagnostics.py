"""Milliseconds per irotavg_graph_edge_diagnostics call (host time around the synchronous call, after one warm-up call),
printed as one JSON line. Per case: `ms` all three outputs + scale, `ms_leverage` leverage alone, and measured in the
same run on the same handle `ms_marginals` = rotation_variance(marginals) -- the factorisation both queries share, so
the difference is the price of the edge passes and the copies. --pairs-baseline adds, for 100k / 2M band-only and + 100
closures, ONE run of the only other way to the same numbers: rotation_variance(pairs = all m edges, marginals=False)
(`ms_pairs_all_edges`), and the largest relative difference between the two answers.
  Cases: 100k views / 2M edges band-only, the same with 30 / 100 / 2048 loop closures, 1M views / 20M edges band-only,
  the fixture (dense route). Weights are those of one irls (GM, 5 deg).
Usage: python tools/time_edge_diagnostics.py [--reps N] [--only NAME[,NAME]] [--pairs-baseline]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from irotavg_amd import capi  # noqa: E402
from time_rotation_variance import CASES as VARIANCE_CASES  # noqa: E402

CASES = ["100k_2M_band", "100k_2M_30cl", "100k_2M_100cl", "100k_2M_2048cl", "1M_20M_band", "fixture"]
BASELINE_CASES = ("100k_2M_band", "100k_2M_100cl")


def med(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(ts)), 3), round(float(np.min(ts)), 3)


def time_case(name, reps, baseline):
    I, QQ, Q, n, f = VARIANCE_CASES[name]()
    with capi.Graph(I, QQ, n, f) as G:
        G.set_rotations(Q)
        G.irls(4, 5 * np.pi / 180, 50, 1e-3)
        st = G.stats()
        out = dict(m=int(len(I)), band_block=st["band_block"], closures=G.direct_info()["closures"])
        out["ms"], out["ms_min"] = med(lambda: G.edge_diagnostics(), reps)
        out["ms_leverage"], out["ms_leverage_min"] = med(lambda: G.edge_diagnostics(edge_var=False, chi2=False), reps)
        out["ms_marginals"], out["ms_marginals_min"] = med(lambda: G.rotation_variance(), reps)
        if baseline and name in BASELINE_CASES:
            ev = G.edge_diagnostics(leverage=False, chi2=False)["edge_var"]
            t0 = time.perf_counter()
            pv = G.rotation_variance(I, marginals=False)["pair_var"]
            out["ms_pairs_all_edges"] = round(1e3 * (time.perf_counter() - t0), 1)
            out["speedup_over_pairs"] = round(out["ms_pairs_all_edges"] / out["ms"], 1)
            rows = (I[:, 1] >= f) & (I[:, 0] != I[:, 1])
            out["max_rel_diff_vs_pairs"] = float(np.max(np.abs(ev[rows] - pv[rows]) / pv[rows]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--pairs-baseline", action="store_true")
    a = ap.parse_args()
    out = {}
    for name in CASES:
        if a.only and name not in a.only.split(","):
            continue
        out[name] = time_case(name, a.reps, a.pairs_baseline)
    print(json.dumps(dict(tool="time_edge_diagnostics", reps=a.reps, results=out)))


if __name__ == "__main__":
    main()
