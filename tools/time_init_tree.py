#!/usr/bin/env python
"""Times the two ways a caller whose I and QQ live on the device can get initial rotations (docs/init_tree.md) and prints
ONE JSON line.

    route A  D2H of I and QQ (QQ transposed on the device first, so that it arrives column-major), the host sweep
             irotavg_init_mst, H2D of Q;
    route B  irotavg_init_tree_dev on the device arrays.

Per case: after a warm-up of both, the median, minimum and maximum in milliseconds of `--reps` (at least seven) alternating
repetitions, the rounds and launches of route B, whether irotavg_init_tree gives route B's bytes, and -- up to
`--solve-max-views` views -- the iterations and the final mean residual of l1ra(5) + irls from either initialisation.
Every case runs in a child process of its own under a time limit; after a case that fails none is started.

    python tools/time_init_tree.py                        # the four documented cases
    python tools/time_init_tree.py --cases band,shuffled
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

#        views, edges, share of loop edges, edge list shuffled
CASES = {"band": (100000, 2000000, 0.0, False), "shuffled": (100000, 2000000, 0.0, True),
         "loops": (100000, 2000000, 0.02, False), "large": (1000000, 20000000, 0.0, False)}
SIG = 5 * np.pi / 180


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=len(ms))


def run_case(name, args):
    import torch
    from irotavg_amd import capi, synth
    L = capi.lib()
    if L.irotavg_device_count() <= 0:
        raise SystemExit("no HIP device: the product has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    n, m_ask, p_loop, shuffled = CASES[name]
    S = synth.make_graph(n, m_ask, p_loop, seed=args.seed)
    I = np.ascontiguousarray(S["I"], dtype=np.int32)
    QQ = np.ascontiguousarray(S["QQ"])
    if shuffled:
        perm = np.random.default_rng(args.seed + 1).permutation(len(I))
        I, QQ = np.ascontiguousarray(I[perm]), np.ascontiguousarray(QQ[perm])
    m = len(I)
    ei = torch.tensor(I, device=dev)
    qq = torch.tensor(QQ, dtype=torch.float64, device=dev)
    Q0 = np.zeros((n, 4))
    Q0[:, 3] = 1
    Q0[0] = S["Qgt"][0]
    Qa, Qb = torch.tensor(Q0, device=dev), torch.tensor(Q0, device=dev)
    info = (C.c_int64 * 4)()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    sweeps = [0]
    torch.cuda.synchronize()

    def route_a():
        t = time.perf_counter()
        Ih = ei.cpu().numpy()
        QQh = qq.t().contiguous().cpu().numpy()            # (4, m) rows: column-major m x 4 with ldqq = m
        Qh = Qa.t().contiguous().cpu().numpy()
        rc = L.irotavg_init_mst(n, m, capi._d(Qh), n, capi._d(QQh), m, capi._i(Ih), 1)
        Qa.copy_(torch.from_numpy(Qh).to(dev).t())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        capi.check(rc, "irotavg_init_mst")
        return 1e3 * dt

    def route_b():
        t = time.perf_counter()
        rc = L.irotavg_init_tree_dev(m, n, 1, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1, None,
                                     C.c_void_p(Qb.data_ptr()), 4, 1, None, info, stream)
        dt = time.perf_counter() - t                       # (the call blocks until the status is back)
        capi.check(rc, "irotavg_init_tree_dev")
        return 1e3 * dt

    for _ in range(args.warmup):
        route_a()
        route_b()
    ta, tb = [], []
    for _ in range(args.reps):
        ta.append(route_a())
        tb.append(route_b())
    launches, jumps = capi.init_tree_counters()
    Qh = Q0.copy()
    host = capi.init_tree(I, QQ, n, Qh, in_tree=False)
    row = dict(case=name, views=n, edges=m, p_loop=p_loop, shuffled=shuffled, route_a=stats(ta), route_b=stats(tb),
               rounds=int(info[0]), launches=launches, moving_jump_passes_max=jumps,
               host_form_bitwise_equal=bool(Qh.tobytes() == Qb.cpu().numpy().tobytes() and host["info"]["rounds"] == info[0]))
    row["b_over_a_median"] = round(row["route_b"]["median_ms"] / row["route_a"]["median_ms"], 4)
    row["init_distance_max_rad"] = float(synth.angular_distance(Qa.cpu().numpy(), Qb.cpu().numpy()).max())
    if n <= args.solve_max_views:
        for key, Qi in (("solve_from_a", Qa), ("solve_from_b", Qb)):
            with capi.Graph(I, QQ, n, 1) as G:
                G.set_rotations(Qi.cpu().numpy())
                a = G.l1ra(5, 1e-3)
                b = G.irls(4, SIG, 100, 1e-3)
                G.edge_residual()
                res = np.linalg.norm(G.get_residuals(), axis=1)
                row[key] = dict(l1ra_iters=int(a["iters"]), irls_iters=int(b["iters"]), mean_residual_rad=float(res.mean()))
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="band,shuffled,loops,large", help="comma-separated names of %s" % sorted(CASES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--solve-max-views", type=int, default=100000, help="l1ra + irls from either initialisation up to this size")
    ap.add_argument("--limit", type=float, default=420.0, help="seconds one case may take")
    ap.add_argument("--case", help="(internal) run this one case in this process")
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("--reps must be at least 7")
    if args.case:
        return run_case(args.case, args)
    out = dict(tool="time_init_tree", cases=[])
    for name in args.cases.split(","):
        if name not in CASES:
            ap.error("unknown case %s" % name)
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--seed", str(args.seed), "--solve-max-views", str(args.solve_max_views)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            out["cases"].append(dict(case=name, failed="time limit of %g s" % args.limit))
            break                                             # nothing more is started on the device
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            out["cases"].append(dict(case=name, failed="exit status %d" % r.returncode, stderr=r.stderr[-2000:]))
            break
        out["cases"].append(json.loads(lines[-1]))
    print(json.dumps(out))
    return 0 if all("failed" not in c for c in out["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
