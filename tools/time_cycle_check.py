#!/usr/bin/env python
"""Times the cycle-consistency screen (irotavg_cycle_check_dev against irotavg_cycle_check, docs/cycle_check.md) and
prints ONE JSON line.

Per case (views / edges of synth.make_graph): after a warm-up, the median, minimum and maximum in milliseconds of
`--reps` (at least seven) alternating repetitions of the device-array call and the host-pointer call in the same run, the
triangles per second of the device-array call, whether the two answers are bitwise equal, and one irotavg_graph_irls call
on the same graph as context. `--groups` adds the device-array call at every group width of the triangle kernel.

    python tools/time_cycle_check.py                      # the three documented cases
    python tools/time_cycle_check.py --cases band --groups
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"band": (100000, 2000000, 0.0), "loops": (100000, 2000000, 0.02), "large": (1000000, 20000000, 0.0)}
SIG = 5 * np.pi / 180


def stats(ms):
    ms = sorted(ms)
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="band,loops,large", help="comma-separated names of %s" % sorted(CASES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=SIG)
    ap.add_argument("--groups", action="store_true", help="also time the device-array call at group widths 8, 16, 32, 64")
    ap.add_argument("--no-irls", action="store_true", help="leave the irotavg_graph_irls context out")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("--reps must be at least 7")
    import torch
    from irotavg_amd import capi, ral, synth
    L = capi.lib()
    if L.irotavg_device_count() <= 0:
        raise SystemExit("no HIP device: the product has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    out = dict(tool="time_cycle_check", device=torch.cuda.get_device_name(dev), threshold=args.threshold,
               default_group=capi.cycle_check_group(0), cases=[])
    for name in args.cases.split(","):
        n, m_ask, p_loop = CASES[name]
        S = synth.make_graph(n, m_ask, p_loop, seed=args.seed)
        I = np.ascontiguousarray(S["I"], dtype=np.int32)
        m = len(I)
        QQf = capi.fmat(S["QQ"])
        hc, ho, hm = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m)
        hs = (C.c_int64 * 4)()
        ei = torch.tensor(I, device=dev)
        qq = torch.tensor(np.ascontiguousarray(S["QQ"]), dtype=torch.float64, device=dev)
        dc, do = torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
        dm = torch.zeros(m, dtype=torch.float64, device=dev)
        ds = (C.c_int64 * 4)()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()

        def host_call():
            t = time.perf_counter()
            rc = L.irotavg_cycle_check(m, n, capi._i(I), capi._d(QQf), m, args.threshold, capi._i(hc), capi._i(ho),
                                       capi._d(hm), hs)
            dt = time.perf_counter() - t
            capi.check(rc, "irotavg_cycle_check")
            return 1e3 * dt

        def dev_call():
            t = time.perf_counter()
            rc = L.irotavg_cycle_check_dev(m, n, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1, args.threshold,
                                           C.c_void_p(dc.data_ptr()), C.c_void_p(do.data_ptr()), C.c_void_p(dm.data_ptr()),
                                           ds, stream)
            dt = time.perf_counter() - t   # (the call blocks until the summary is back)
            capi.check(rc, "irotavg_cycle_check_dev")
            return 1e3 * dt

        for _ in range(args.warmup):
            dev_call()
            host_call()
        td, th = [], []
        for _ in range(args.reps):
            td.append(dev_call())
            th.append(host_call())
        torch.cuda.synchronize()
        equal = bool(dc.cpu().numpy().tobytes() == hc.tobytes() and do.cpu().numpy().tobytes() == ho.tobytes() and
                     dm.cpu().numpy().tobytes() == hm.tobytes() and list(ds) == list(hs))
        row = dict(case=name, views=n, edges=m, p_loop=p_loop, dev=stats(td), host=stats(th), bitwise_equal=equal,
                   summary=dict(zip(capi.SUMMARY_FIELDS, (int(v) for v in ds))))
        row["triangles_per_s"] = round(row["summary"]["triangles"] / (1e-3 * row["dev"]["median_ms"]), 1)
        row["dev_over_host_median"] = round(row["dev"]["median_ms"] / row["host"]["median_ms"], 4)
        if args.groups:
            row["groups"] = {}
            for g in (8, 16, 32, 64):
                old = capi.cycle_check_group(g)
                try:
                    for _ in range(args.warmup):
                        dev_call()
                    row["groups"][str(g)] = stats([dev_call() for _ in range(args.reps)])
                finally:
                    capi.cycle_check_group(old)
        if not args.no_irls:
            Q0 = np.zeros((n, 4))
            Q0[:, 3] = 1
            Q0[0] = S["Qgt"][0]
            ral.init_mst(Q0, S["QQ"], S["I"], 1)
            with capi.Graph(I, S["QQ"], n, 1) as G:
                G.set_rotations(Q0)
                G.synchronize()
                t = time.perf_counter()
                r = G.irls(4, SIG, 100, 1e-3)
                G.synchronize()
                row["irls_context"] = dict(ms=round(1e3 * (time.perf_counter() - t), 3), iters=int(r["iters"]))
        out["cases"].append(row)
        del ei, qq, dc, do, dm
    print(json.dumps(out))


if __name__ == "__main__":
    main()
