"""Milliseconds per view-graph uncertainty query (docs/viewgraph_uncertainty.md), host time around the synchronous call
after one warm-up call, printed as one JSON line.
  window: a stream of 200 views linked to 4 predecessors; per call of the window route (win = 10) `us_variance` (var + one
          pair), `us_edges` (all three edge arrays), `us_gate` (one candidate), next to `us_rot_avg` = rotAvg(10) on the
          same graph in the same run (each rotAvg moves poses; the queries in between do not).
  global: view sequences of --views views linked to 4 predecessors with 0 and 10 loop closures; `ms_variance` /
          `ms_edges` / `ms_gate` of the global query (handle build + pose weights + handle query) next to `ms_rot_avg` =
          rotAvg(5000000) on the same graph, and `ms_handle_variance` = irotavg_graph_rotation_variance on a handle of
          the same problem that is already built (the difference to ms_variance is the handle build).
  pose_weights: irotavg_graph_time_kernel's event timing of K1 (1), K2 (2) and k_pose_weights (12) on 100k views / 2M
          edges, 50 launches each.
Usage: python tools/time_viewgraph_uncertainty.py [--reps N] [--views N[,N]] [--skip-global]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from irotavg_amd import capi, synth  # noqa: E402
from irotavg_amd.viewgraph import ViewGraph, quat2rmat  # noqa: E402

SIGMA = 5 * np.pi / 180


def med(fn, reps, scale=1e3):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(scale * (time.perf_counter() - t0))
    return round(float(np.median(ts)), 3), round(float(np.min(ts)), 3)


def stream(n, ncl, seed, k_prev=4, noise=0.01):
    rng = np.random.default_rng(seed)
    Qgt = rng.normal(size=(n, 4))
    Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    I = [(j - d, j) for j in range(1, n) for d in range(1, min(k_prev, j) + 1)]
    for _ in range(ncl):
        a = int(rng.integers(0, n - 2000))
        I.append((a, int(a + rng.integers(1000, n - a))))
    I = np.array(I, dtype=np.int32)
    QQ = synth.qmul(synth.qexp(rng.normal(scale=noise, size=(len(I), 3))), synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]])))
    Q0 = synth.qmul(synth.qexp(rng.normal(scale=0.02, size=(n, 3))), Qgt)
    vg = ViewGraph()
    for v in range(n):
        vg.addView(quat2rmat(Q0[v]))
    for (i, j), q in zip(I, QQ):
        vg.connect(int(i), int(j), quat2rmat(q))
    vg.fixPose(0, quat2rmat(Qgt[0]))
    return vg, I, QQ, Q0, Qgt


def time_window(reps):
    vg, I, QQ, Q0, Qgt = stream(200, 0, 1)
    n = 200
    R = quat2rmat(synth.qmul(Qgt[n - 1], synth.qconj(Qgt[n - 7])))
    out = {}
    out["us_variance"], out["us_variance_min"] = med(lambda: vg.rotationVariance(10, [(n - 1, n - 2)]), reps, 1e6)
    out["us_edges"], out["us_edges_min"] = med(lambda: vg.edgeDiagnostics(10, cap=64), reps, 1e6)
    out["us_gate"], out["us_gate_min"] = med(lambda: vg.gateConnections(10, [(n - 7, n - 1)], [R]), reps, 1e6)
    out["us_rot_avg"], out["us_rot_avg_min"] = med(lambda: vg.rotAvg(10), reps, 1e6)
    info = vg.rotationVariance(10)
    out.update(route=info["route"], n_views=info["n_views"], n_edges=info["n_edges"], n_fixed=info["n_fixed"])
    return out


def time_global(n, ncl, reps):
    vg, I, QQ, Q0, Qgt = stream(n, ncl, 2 + ncl)
    big = 5000000
    R = quat2rmat(synth.qmul(Qgt[n - 1], synth.qconj(Qgt[10])))
    out = dict(views=n, closures_planted=ncl, m=int(len(I)))
    out["ms_rot_avg"], out["ms_rot_avg_min"] = med(lambda: vg.rotAvg(big), reps)
    out["ms_variance"], out["ms_variance_min"] = med(lambda: vg.rotationVariance(big, [(10, n - 1)]), reps)
    out["ms_edges"], out["ms_edges_min"] = med(lambda: vg.edgeDiagnostics(big, cap=len(I)), reps)
    out["ms_gate"], out["ms_gate_min"] = med(lambda: vg.gateConnections(big, [(10, n - 1)], [R]), reps)
    info = vg.rotationVariance(big, marginals=False)
    out.update(route=info["route"], closures=info["closures"])
    Q = np.stack([capi_quat(vg.R(v)) for v in range(n)])
    with capi.Graph(I, QQ, n, 1) as G:
        G.set_rotations(Q)
        G.pose_weights(4, SIGMA)
        out["ms_handle_variance"], out["ms_handle_variance_min"] = med(lambda: G.rotation_variance([(10, n - 1)]), reps)
    return out


def capi_quat(R):
    from irotavg_amd.viewgraph import rmat2quat
    return rmat2quat(R)


def time_pose_weights(reps):
    S = synth.make_graph(100000, 2000000, 0.0, seed=5)
    with capi.Graph(S["I"], S["QQ"], 100000, 1) as G:
        G.set_rotations(S["Qgt"])
        G.edge_residual()
        out = dict(m=int(len(S["I"])), ms_k1=round(G.time_kernel(1, 50), 5), ms_k2=round(G.time_kernel(2, 50), 5),
                   ms_pose_weights=round(G.time_kernel(12, 50), 5))
        out["bytes_per_edge"] = 8 + 32 + 24 + 8
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--views", default="75000,100000")
    ap.add_argument("--skip-global", action="store_true")
    a = ap.parse_args()
    out = dict(window=time_window(max(a.reps, 50)))
    if not a.skip_global:
        for n in [int(x) for x in a.views.split(",")]:
            for ncl in (0, 10):
                out["global_%dk_%dcl" % (n // 1000, ncl)] = time_global(n, ncl, a.reps)
    out["pose_weights"] = time_pose_weights(a.reps)
    print(json.dumps(dict(tool="time_viewgraph_uncertainty", reps=a.reps, results=out)))


if __name__ == "__main__":
    main()
