#!/usr/bin/env python
"""Times irotavg_components_dev on device arrays (docs/components.md) and prints ONE JSON line per case.

Per case and per rank (all zero; 2 % of the edges negative): wall-clock around the blocking device-array call, the median,
minimum and maximum in milliseconds of `--reps` (at least seven) repetitions after `--warmup` (at least two) warm-ups, the
call's info, and whether a second call and the host form give the same arrays. Next to it, on the same arrays and in the
same way, the rank-free irotavg_init_tree_dev -- the only other code of the library that finds components, in log n rounds
with a read-back each -- with its rounds and launches, and cycle_check. The launches of components are a constant of the
implementation (docs/components.md); a kernel trace counts them. Every case runs in a child process of its own under a
time limit; after a case that fails none is started.

    python tools/time_components.py                        # the documented cases
    python tools/time_components.py --cases band,span2
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

#        views, edges, share of loop edges (span2 / span32: the same views with 2 / 32 predecessors each)
CASES = {"band": (100000, 2000000, 0.0), "loops": (100000, 2000000, 0.02), "span2": (100000, 200000, 0.0),
         "span32": (100000, 3200000, 0.0)}
LAUNCHES = 8  # the fill of the head and seven kernels (components.hip)


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=len(ms))


def timed(call, args):
    """the blocking call's wall-clock: `warmup` calls, then `reps` timed ones between two synchronises"""
    import torch
    ms = []
    for rep in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if rep >= args.warmup:
            ms.append(1e3 * (time.perf_counter() - t))
    return stats(ms)


def run_case(name, args):
    import torch
    from irotavg_amd import capi, synth, torch_api
    if capi.lib().irotavg_device_count() <= 0:
        raise SystemExit("no HIP device: the product has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    n, m_ask, p_loop = CASES[name]
    S = synth.make_graph(n, m_ask, p_loop, seed=args.seed)
    I = np.ascontiguousarray(S["I"], dtype=np.int32)
    m = len(I)
    ei = torch.tensor(I, device=dev)
    qq = torch.tensor(np.ascontiguousarray(S["QQ"]), dtype=torch.float64, device=dev)
    Q = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    Q[:, 3] = 1.0
    cut = np.zeros(m, dtype=np.int32)
    cut[np.random.default_rng(args.seed + 1).random(m) < 0.02] = -1
    row = dict(case=name, views=n, edges=m, p_loop=p_loop, launches=LAUNCHES)
    for key, rank in (("rank_zero", np.zeros(m, dtype=np.int32)), ("rank_2pct_negative", cut)):
        rk = torch.tensor(rank, device=dev)
        t = timed(lambda: torch_api.components(ei, n, 1, rk, "largest"), args)
        a, b = torch_api.components(ei, n, 1, rk, "largest"), torch_api.components(ei, n, 1, rk, "largest")
        host = capi.components(I, n, 1, rank, "largest")
        names = ("label", "view_map", "edge_map", "views", "edges")
        same = all(torch.equal(a[k], b[k]) for k in names + ("edge_index",))
        same_host = all(np.array_equal(a[k].cpu().numpy(), host[k]) for k in names) and \
            np.array_equal(a["edge_index"].cpu().numpy(), host["I"]) and host["info"] == a["info"]
        row[key] = dict(components_dev=t, info=a["info"], second_call_equal=bool(same), host_form_equal=bool(same_host))
    row["init_tree_dev_rank_free"] = timed(lambda: torch_api.init_tree(ei, qq, n, Q, allow_rc=(capi.ERR_NOT_SPANNING,)), args)
    launches, jumps = capi.init_tree_counters()
    tree = torch_api.init_tree(ei, qq, n, Q, allow_rc=(capi.ERR_NOT_SPANNING,))
    row["init_tree_dev_rank_free"].update(rounds=tree["info"]["rounds"], launches=launches, moving_jump_passes_max=jumps)
    row["cycle_check_dev"] = timed(lambda: torch_api.cycle_check(ei, qq, n), args)
    row["components_over_init_tree_median"] = round(row["rank_zero"]["components_dev"]["median_ms"] /
                                                    row["init_tree_dev_rank_free"]["median_ms"], 4)
    print(json.dumps(row))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="band,loops,span2,span32", help="comma-separated names of %s" % sorted(CASES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--limit", type=float, default=240.0, help="seconds one case may take")
    ap.add_argument("--case", help="(internal) run this one case in this process")
    args = ap.parse_args()
    if args.reps < 7 or args.warmup < 2:
        ap.error("--reps must be at least 7 and --warmup at least 2")
    if args.case:
        return run_case(args.case, args)
    ok = True
    for name in args.cases.split(","):
        if name not in CASES:
            ap.error("unknown case %s" % name)
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--seed", str(args.seed)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(case=name, failed="time limit of %g s" % args.limit)))
            return 1                                          # nothing more is started on the device
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            print(json.dumps(dict(case=name, failed="exit status %d" % r.returncode, stderr=r.stderr[-2000:])))
            return 1
        print(lines[-1], flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
