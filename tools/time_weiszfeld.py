#!/usr/bin/env python
"""Times the Weiszfeld sweeps (irotavg_weiszfeld_dev, docs/local_sweeps.md) on the `band` and `loops` 100k / 2M graphs of
tools/time_cycle_check.py and prints ONE JSON line per case.

Per case, in a child process under a time limit of its own: the start is init_tree's Q (all ranks 0); after two warm-ups,
seven alternating repetitions of the blocking device-array call at sweeps = 10, at sweeps = 0 (with info: emit, sort and
the row bounds, no sweep) and of cycle_check on the same graph, as median (min - max) in milliseconds; per repetition one
sweep is the difference of the two call times over 10. Also: step[t], the mean edge residual before and after the sweeps,
and the outer iterations and time of l1ra(5) + irls from init_tree alone and from init_tree plus 10 L1 sweeps.

    python tools/time_weiszfeld.py                  # band and loops
    python tools/time_weiszfeld.py --inner 3
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

CASES = {"band": (100000, 2000000, 0.0), "loops": (100000, 2000000, 0.02)}
SIG = 5 * np.pi / 180


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=len(ms))


def case(args):
    import torch
    from irotavg_amd import capi, synth, torch_api
    L = capi.lib()
    if L.irotavg_device_count() <= 0:
        raise SystemExit("no HIP device: the product has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    n, m_ask, p_loop = CASES[args.case]
    S = synth.make_graph(n, m_ask, p_loop, seed=args.seed)
    m = len(S["I"])
    ei = torch.tensor(np.ascontiguousarray(S["I"], dtype=np.int32), device=dev)
    qq = torch.tensor(np.ascontiguousarray(S["QQ"]), dtype=torch.float64, device=dev)
    Q0 = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    Q0[:, 3] = 1.0
    torch_api.init_tree(ei, qq, n, Q0)
    Q = Q0.clone()
    tri = [torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev),
           torch.zeros(m, dtype=torch.float64, device=dev)]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    step, info, ts = (C.c_double * 10)(), (C.c_int64 * 2)(), (C.c_int64 * 4)()
    cost = capi.SWEEP_COSTS[args.cost]

    def sweep_call(sweeps):
        Q.copy_(Q0)
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc = L.irotavg_weiszfeld_dev(m, n, 1, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1, C.c_void_p(Q.data_ptr()),
                                     4, 1, None, cost, sweeps, args.inner, 1e-6, step, info, stream)
        dt = time.perf_counter() - t   # (the call blocks until step and info are back)
        capi.check(rc, "irotavg_weiszfeld_dev")
        return 1e3 * dt

    def tri_call():
        t = time.perf_counter()
        rc = L.irotavg_cycle_check_dev(m, n, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1, SIG,
                                       *[C.c_void_p(x.data_ptr()) for x in tri], ts, stream)
        dt = time.perf_counter() - t
        capi.check(rc, "irotavg_cycle_check_dev")
        return 1e3 * dt

    t10, t0, tt = [], [], []
    for rep in range(args.warmup + args.reps):
        b, c, a = sweep_call(0), tri_call(), sweep_call(10)    # (the call at 10 last: Q keeps its result)
        if rep >= args.warmup:
            t10.append(a), t0.append(b), tt.append(c)
    row = dict(tool="time_weiszfeld", device=torch.cuda.get_device_name(dev), case=args.case, views=n, edges=m, p_loop=p_loop,
               cost=args.cost, inner=args.inner, sweeps10=stats(t10), sweeps0=stats(t0),
               per_sweep=stats([(a - b) / 10 for a, b in zip(t10, t0)]), cycle_check=stats(tt),
               info=dict(zip(capi.SWEEP_INFO_FIELDS, (int(v) for v in info))), step=[round(v, 6) for v in step])
    row["sweep_over_cycle_check_median"] = round(row["per_sweep"]["median_ms"] / row["cycle_check"]["median_ms"], 4)
    row["gb_per_s_at_76_bytes_a_half_edge"] = round(76 * row["info"]["half_edges"] / (1e6 * row["per_sweep"]["median_ms"]), 1)

    def solve(start):
        with torch_api.TorchGraph(ei, qq, n, 1) as G:
            G.set_rotations(start)
            G.edge_residual()
            before = float(G.residuals().norm(dim=1).mean())
            G.synchronize()
            t = time.perf_counter()
            a = G.l1ra(5, 1e-3, allow_rc=(capi.ERR_NOT_CONVERGED,))
            b = G.irls(4, SIG, 100, 1e-3, allow_rc=(capi.ERR_NOT_CONVERGED,))
            G.synchronize()
            return dict(mean_edge_residual_at_start=round(before, 6), l1ra_iters=int(a["iters"]), irls_iters=int(b["iters"]),
                        ms=round(1e3 * (time.perf_counter() - t), 3))
    row["l1ra5_irls_from_init_tree"] = solve(Q0)
    row["l1ra5_irls_from_init_tree_and_10_sweeps"] = solve(Q)
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="band,loops", help="comma-separated names of %s" % sorted(CASES))
    ap.add_argument("--case", default=None, help="run this one case in this process (what the parent starts)")
    ap.add_argument("--cost", default="l1", choices=("l1", "l2"))
    ap.add_argument("--inner", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds a case may take")
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("--reps must be at least 7")
    if args.case:
        return case(args)
    for name in args.cases.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--cost", args.cost, "--inner", str(args.inner),
               "--reps", str(args.reps), "--warmup", str(args.warmup), "--seed", str(args.seed)]
        try:
            r = subprocess.run(cmd, timeout=args.limit)
        except subprocess.TimeoutExpired:
            raise SystemExit("case %s passed its limit of %g s: nothing more is started" % (name, args.limit))
        if r.returncode != 0:
            raise SystemExit("case %s ended with status %d: nothing more is started" % (name, r.returncode))


if __name__ == "__main__":
    main()
