#!/usr/bin/env python
"""Times the cycle-consistency screen (irotavg_cycle_check_dev against irotavg_cycle_check, docs/cycle_check.md) and
prints ONE JSON line.

Per case (views / edges of synth.make_graph): after a warm-up, the median, minimum and maximum in milliseconds of
`--reps` (at least seven) alternating repetitions of the device-array call and the host-pointer call in the same run, the
triangles per second of the device-array call, whether the two answers are bitwise equal, and one irotavg_graph_irls call
on the same graph as context. `--groups` adds the device-array call at every group width of the triangle kernel.

    python tools/time_cycle_check.py                      # the three documented cases
    python tools/time_cycle_check.py --cases band --groups
    python tools/time_cycle_check.py --quads --groups     # the four-cycle test (irotavg_cycle_check4_dev), same protocol
    python tools/time_cycle_check.py --cemp               # the corruption estimates (irotavg_cycle_cemp_dev), band and loops

Run each case under a time limit of its own (`timeout`): one case per invocation, `--cases NAME` or `--quads NAME`.
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


def paired_loops(S, share, seed):
    """S (band-only) with `share` of its edge count added as loop closures in pairs (a, b), (a + 1, b + 1): the cluster
    a place-recognition match comes in, whose quadrilateral with two sequence edges tests both. Noise-free closures."""
    from irotavg_amd import synth
    rng = np.random.default_rng([seed, 4])
    n, pairs = S["n"], int(round(share * len(S["I"]) / 2))
    a = rng.integers(0, n - 1, size=pairs)
    b = (a + rng.integers(n // 4, 3 * n // 4, size=pairs)) % (n - 1)
    I = np.concatenate([S["I"], np.stack([a, b], 1), np.stack([a + 1, b + 1], 1)]).astype(np.int32)
    extra = I[len(S["I"]):]
    return I, np.concatenate([S["QQ"], synth.qmul(S["Qgt"][extra[:, 1]], synth.qconj(S["Qgt"][extra[:, 0]]))])


def quads(args):
    """--quads: the four-cycle test (a) of the untested subset of a 100k / 2M band graph with 2 % paired loop edges, next
    to the triangle test of the whole graph, (b) of all edges of the band graph, (c) at every sub-group width."""
    import torch
    from irotavg_amd import capi, synth
    L = capi.lib()
    if L.irotavg_device_count() <= 0:
        raise SystemExit("no HIP device: the product has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    out = dict(tool="time_cycle_check --quads", device=torch.cuda.get_device_name(dev), threshold=args.threshold,
               default_group=capi.cycle_check4_group(0), cases=[])
    n, m_ask = args.quads_size
    S = synth.make_graph(n, m_ask, 0.0, seed=args.seed)
    for name in args.quads.split(","):
        I, QQ = paired_loops(S, 0.02, args.seed) if name == "paired" else (np.ascontiguousarray(S["I"], dtype=np.int32), S["QQ"])
        m = len(I)
        ei, qq = torch.tensor(I, device=dev), torch.tensor(np.ascontiguousarray(QQ), dtype=torch.float64, device=dev)
        tri = [torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev),
               torch.zeros(m, dtype=torch.float64, device=dev)]
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ts, qs = (C.c_int64 * 4)(), (C.c_int64 * 4)()

        def tri_call():
            t = time.perf_counter()
            rc = L.irotavg_cycle_check_dev(m, n, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1, args.threshold,
                                           *[C.c_void_p(x.data_ptr()) for x in tri], ts, stream)
            dt = time.perf_counter() - t   # (the call blocks until the summary is back)
            capi.check(rc, "irotavg_cycle_check_dev")
            return 1e3 * dt

        tri_call()
        sub = torch.nonzero(tri[0] == 0).flatten().to(torch.int32) if name == "paired" else None
        ne = m if sub is None else int(sub.shape[0])
        quad = [torch.zeros(ne, dtype=torch.int32, device=dev), torch.zeros(ne, dtype=torch.int32, device=dev),
                torch.zeros(ne, dtype=torch.float64, device=dev)]

        def quad_call():
            t = time.perf_counter()
            rc = L.irotavg_cycle_check4_dev(m, n, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1, args.threshold, ne,
                                            None if sub is None else C.c_void_p(sub.data_ptr()),
                                            *[C.c_void_p(x.data_ptr()) for x in quad], qs, stream)
            dt = time.perf_counter() - t
            capi.check(rc, "irotavg_cycle_check4_dev")
            return 1e3 * dt

        for _ in range(args.warmup):
            quad_call()
            tri_call()
        tq, tt = [], []
        for _ in range(args.reps):
            tq.append(quad_call())
            tt.append(tri_call())
        h = capi.cycle_check4(I, QQ, n, args.threshold, None if sub is None else sub.cpu().numpy())
        equal = bool(all(h[k].tobytes() == x.cpu().numpy().tobytes() for k, x in zip(("quad_count", "quad_ok", "quad_min"), quad))
                     and list(h["summary"].values()) == list(qs))
        row = dict(case=name, views=n, edges=m, tested=ne, quads=stats(tq), triangles_whole_graph=stats(tt), bitwise_equal=equal,
                   summary=dict(zip(capi.SUMMARY4_FIELDS, (int(v) for v in qs))))
        row["quadrilaterals_per_s"] = round(row["summary"]["quadrilaterals"] / (1e-3 * row["quads"]["median_ms"]), 1)
        row["share_supported"] = round(row["summary"]["supported"] / ne, 4)
        row["quads_over_triangles_median"] = round(row["quads"]["median_ms"] / row["triangles_whole_graph"]["median_ms"], 4)
        if args.groups:
            row["groups"] = {}
            for g in (8, 16, 32, 64):
                old = capi.cycle_check4_group(g)
                try:
                    for _ in range(args.warmup):
                        quad_call()
                    row["groups"][str(g)] = stats([quad_call() for _ in range(args.reps)])
                finally:
                    capi.cycle_check4_group(old)
        out["cases"].append(row)
        del ei, qq, tri, quad, sub
    print(json.dumps(out))


def cemp(args):
    """--cemp: the corruption estimates (irotavg_cycle_cemp_dev) at six iterations of the default schedule and at none,
    alternating with the triangle test on the same graph; the time of one iteration is the difference over six."""
    import torch
    from irotavg_amd import capi, synth, torch_api
    L = capi.lib()
    if L.irotavg_device_count() <= 0:
        raise SystemExit("no HIP device: the product has no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device())
    out = dict(tool="time_cycle_check --cemp", device=torch.cuda.get_device_name(dev), cases=[])
    beta = np.array(torch_api.cemp_beta(6))
    for name in args.cemp.split(","):
        n, m_ask, p_loop = CASES[name]
        S = synth.make_graph(n, m_ask, p_loop, seed=args.seed)
        m = len(S["I"])
        ei = torch.tensor(np.ascontiguousarray(S["I"], dtype=np.int32), device=dev)
        qq = torch.tensor(np.ascontiguousarray(S["QQ"]), dtype=torch.float64, device=dev)
        s, used = torch.zeros(m, dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.int32, device=dev)
        tri = [torch.zeros(m, dtype=torch.int32, device=dev), torch.zeros(m, dtype=torch.int32, device=dev),
               torch.zeros(m, dtype=torch.float64, device=dev)]
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        hs, ts = (C.c_int64 * 2)(), (C.c_int64 * 4)()
        torch.cuda.synchronize()

        def cemp_call(iters):
            t = time.perf_counter()
            rc = L.irotavg_cycle_cemp_dev(m, n, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1, iters, capi._d(beta), 0,
                                          C.c_void_p(s.data_ptr()), C.c_void_p(used.data_ptr()), hs, stream)
            dt = time.perf_counter() - t   # (the call blocks until the outputs are written)
            capi.check(rc, "irotavg_cycle_cemp_dev")
            return 1e3 * dt

        def tri_call():
            t = time.perf_counter()
            rc = L.irotavg_cycle_check_dev(m, n, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1, args.threshold,
                                           *[C.c_void_p(x.data_ptr()) for x in tri], ts, stream)
            dt = time.perf_counter() - t
            capi.check(rc, "irotavg_cycle_check_dev")
            return 1e3 * dt

        t6, t0, tt = [], [], []
        for rep in range(args.warmup + args.reps):
            a, b, c = cemp_call(6), cemp_call(0), tri_call()
            if rep >= args.warmup:
                t6.append(a), t0.append(b), tt.append(c)
        row = dict(case=name, views=n, edges=m, p_loop=p_loop, cemp_iters6=stats(t6), cemp_iters0=stats(t0),
                   per_iteration=stats([(a - b) / 6 for a, b in zip(t6, t0)]), cycle_check=stats(tt),
                   summary=dict(zip(capi.CEMP_SUMMARY_FIELDS, (int(v) for v in hs))))
        row["table_bytes"] = 16 * row["summary"]["records"]
        row["iters6_over_cycle_check_median"] = round(row["cemp_iters6"]["median_ms"] / row["cycle_check"]["median_ms"], 4)
        row["iteration_over_cycle_check_median"] = round(row["per_iteration"]["median_ms"] / row["cycle_check"]["median_ms"], 4)
        row["table_gb_per_s_of_an_iteration"] = round(row["table_bytes"] / (1e6 * row["per_iteration"]["median_ms"]), 1)
        out["cases"].append(row)
        del ei, qq, s, used, tri
    print(json.dumps(out))


def cemp4(args):
    """--cemp4 paired: the corruption estimates over four-cycles (irotavg_cycle_cemp4_dev) of the edges that triangle CEMP
    leaves NaN on the paired graph of --quads, at six iterations and at none, alternating with the four-cycle test of the
    same subset; the time of one iteration is the difference over six."""
    import torch
    from irotavg_amd import capi, synth, torch_api
    L = capi.lib()
    if L.irotavg_device_count() <= 0:
        raise SystemExit("no HIP device: the product has no CPU fallback")
    if args.cemp4 != "paired":
        raise SystemExit("--cemp4 knows the case paired alone")
    dev = torch.device("cuda", torch.cuda.current_device())
    n, m_ask = args.quads_size
    I, QQ = paired_loops(synth.make_graph(n, m_ask, 0.0, seed=args.seed), 0.02, args.seed)
    m, beta = len(I), np.array(torch_api.cemp_beta(6))
    ei, qq = torch.tensor(I, device=dev), torch.tensor(np.ascontiguousarray(QQ), dtype=torch.float64, device=dev)
    s = torch_api.cycle_cemp(ei, qq, n, used=False, summary=False)["s"]
    sub = torch.nonzero(torch.isnan(s)).flatten().to(torch.int32)
    ne = int(sub.shape[0])
    s4, used = torch.zeros(ne, dtype=torch.float64, device=dev), torch.zeros(ne, dtype=torch.int32, device=dev)
    quad = [torch.zeros(ne, dtype=torch.int32, device=dev), torch.zeros(ne, dtype=torch.int32, device=dev),
            torch.zeros(ne, dtype=torch.float64, device=dev)]
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    hs, qs, p = (C.c_int64 * 2)(), (C.c_int64 * 4)(), lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()

    def cemp4_call(iters):
        t = time.perf_counter()
        rc = L.irotavg_cycle_cemp4_dev(m, n, p(ei), p(qq), 4, 1, p(s), ne, p(sub), iters, capi._d(beta), 0, p(s4), p(used), hs, stream)
        dt = time.perf_counter() - t   # (the call blocks until the outputs are written)
        capi.check(rc, "irotavg_cycle_cemp4_dev")
        return 1e3 * dt

    def quad_call():
        t = time.perf_counter()
        rc = L.irotavg_cycle_check4_dev(m, n, p(ei), p(qq), 4, 1, args.threshold, ne, p(sub), *[p(x) for x in quad], qs, stream)
        dt = time.perf_counter() - t
        capi.check(rc, "irotavg_cycle_check4_dev")
        return 1e3 * dt

    t6, t0, tq = [], [], []
    for rep in range(args.warmup + args.reps):
        b, c, a = cemp4_call(0), quad_call(), cemp4_call(6)
        if rep >= args.warmup:
            t6.append(a), t0.append(b), tq.append(c)
    h = capi.cycle_cemp4(I, QQ, n, s.cpu().numpy(), sub.cpu().numpy(), beta)
    equal = bool(h["s"].tobytes() == s4.cpu().numpy().tobytes() and h["quad_used"].tobytes() == used.cpu().numpy().tobytes()
                 and list(h["summary"].values()) == list(hs))
    row = dict(case="paired", views=n, edges=m, listed=ne, cemp4_iters6=stats(t6), cemp4_iters0=stats(t0),
               per_iteration=stats([(a - b) / 6 for a, b in zip(t6, t0)]), cycle_check4=stats(tq), bitwise_equal=equal,
               summary=dict(zip(capi.CEMP_SUMMARY_FIELDS, (int(v) for v in hs))))
    row["table_bytes"] = 32 * row["summary"]["records"]
    row["iters6_over_cycle_check4_median"] = round(row["cemp4_iters6"]["median_ms"] / row["cycle_check4"]["median_ms"], 4)
    row["iteration_over_iters6_median"] = round(row["per_iteration"]["median_ms"] / row["cemp4_iters6"]["median_ms"], 4)
    print(json.dumps(dict(tool="time_cycle_check --cemp4", device=torch.cuda.get_device_name(dev), cases=[row])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cemp4", default=None, help="time the corruption estimates over four-cycles instead: paired")
    ap.add_argument("--cemp", nargs="?", const="band,loops", default=None,
                    help="time the corruption estimates instead: comma-separated names of band, loops (default both)")
    ap.add_argument("--quads", nargs="?", const="paired,band", default=None,
                    help="time the four-cycle test instead: comma-separated names of paired, band (default both)")
    ap.add_argument("--quads-size", type=int, nargs=2, default=(100000, 2000000), metavar=("VIEWS", "EDGES"))
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
    if args.cemp4:
        return cemp4(args)
    if args.quads:
        return quads(args)
    if args.cemp:
        return cemp(args)
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
