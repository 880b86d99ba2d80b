"""Milliseconds of ONE irotavg_window_cemp_batch_dev call next to the route a caller with device arrays has without it,
printed as one JSON line (docs/window_cemp_batch.md). The route: a loop of irotavg_cycle_cemp_dev over the problems, on
the same device arrays (each call sorts, scans, builds its triangle table, launches once per iteration and waits). The two
problem sizes of tools/time_window_init_batch.py:
  small  12 views, every view linked to its 4 predecessors (38 edges)
  limit  320 views, every view linked to its 2 predecessors (637 edges)
and nb in {1, 16, 256, 4096} problems that differ in their measurements, six iterations of cemp_beta(). Per (size, nb), in
one run: a warm-up of both, then --reps (default 7) alternating repetitions; median, min and max. Both figures are host
time from a synchronised device to a synchronised device; both calls block by themselves. `tri_used_equal` and
`max_abs_diff` compare the two answers (the order of the sums differs: close, not bitwise); `batch_not_slower` compares
the medians; `us_per_problem` is the batched median over nb.
Usage: python tools/time_window_cemp_batch.py [--reps N] [--nb 1,16,...] [--sizes small,limit]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from irotavg_amd import capi, torch_api  # noqa: E402

SIZES = {"small": (12, 2, 4, None), "limit": (320, 256, 2, 640)}   # views, fixed, predecessors, edge cap
NB = [1, 16, 256, 4096]


def topology(nv, back, cap, rng):
    E = [(v - d, v) for d in range(1, back + 1) for v in range(d, nv)]   # a cap drops the longest links of the last views
    E = np.array(E[:cap] if cap else E, dtype=np.int32)
    return E[rng.permutation(len(E))]


def summary(ts):
    return dict(median=round(float(np.median(ts)), 3), min=round(float(np.min(ts)), 3), max=round(float(np.max(ts)), 3))


def time_case(size, nb, reps):
    L = capi.lib()
    nv, f, back, cap = SIZES[size]
    rng = np.random.default_rng(1)
    I = topology(nv, back, cap, rng)
    m = len(I)
    device = torch.device("cuda", torch.cuda.current_device())
    ip = C.POINTER(C.c_int32)
    q = rng.normal(size=(nb * m, 4)) * 0.02 + np.array([0.0, 0.0, 0.0, 1.0])  # near the identity: small triangle errors
    sizes = np.tile(np.array([[nv, f, m]], dtype=np.int32), (nb, 1))
    ei = torch.tensor(np.tile(I, (nb, 1)), dtype=torch.int32, device=device)
    qq = torch.tensor(q / np.linalg.norm(q, axis=1, keepdims=True), dtype=torch.float64, device=device)
    out = {fn: (torch.zeros(nb * m, dtype=torch.float64, device=device), torch.zeros(nb * m, dtype=torch.int32, device=device))
           for fn in ("route", "batch")}
    beta = np.array(torch_api.cemp_beta(6), dtype=np.float64)
    results = np.zeros(3 * nb, dtype=np.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    at = lambda t, row: C.c_void_p(t.data_ptr() + row * t.stride(0) * t.element_size())

    def route():
        s, used = out["route"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in range(nb):
            rc = L.irotavg_cycle_cemp_dev(m, nv, at(ei, b * m), at(qq, b * m), 4, 1, len(beta), capi._d(beta), 0, at(s, b * m),
                                          at(used, b * m), None, stream)
            if rc:
                raise capi.IrotavgError(rc, "irotavg_cycle_cemp_dev")
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def batch():
        s, used = out["batch"]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.irotavg_window_cemp_batch_dev(nb, sizes.ctypes.data_as(ip), at(ei, 0), at(qq, 0), 4, 1, len(beta), capi._d(beta),
                                             at(s, 0), at(used, 0), results.ctypes.data_as(ip), stream)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if rc:
            raise capi.IrotavgError(rc, "irotavg_window_cemp_batch_dev")
        return dt

    ts = {route: [], batch: []}
    for r in range(reps + 1):
        for fn in (route, batch):
            dt = fn()
            if r > 0:  # r == 0 is the warm-up
                ts[fn].append(dt)
    (sr, ur), (sb, ub) = ((t.cpu().numpy() for t in out[fn]) for fn in ("route", "batch"))
    ro, ba = summary(ts[route]), summary(ts[batch])
    return dict(views=nv, edges=m, triangles=int(results[1::3].sum()), route_ms=ro, batch_ms=ba,
                us_per_problem=round(1e3 * ba["median"] / nb, 2), route_over_batch=round(ro["median"] / ba["median"], 1),
                batch_not_slower=bool(ba["median"] <= ro["median"]), tri_used_equal=bool((ur == ub).all()),
                nan_equal=bool((np.isnan(sr) == np.isnan(sb)).all()), max_abs_diff=float(np.nanmax(np.abs(sr - sb))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nb", default=",".join(str(n) for n in NB))
    ap.add_argument("--sizes", default="small,limit")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if capi.lib().irotavg_device_count() <= 0:
        raise SystemExit("no HIP device: nothing to time")
    out = {}
    for size in a.sizes.split(","):
        out[size] = {}
        for nb in (int(x) for x in a.nb.split(",")):
            out[size][str(nb)] = time_case(size, nb, a.reps)
    print(json.dumps(dict(tool="time_window_cemp_batch", reps=a.reps, iters=6, device=torch.cuda.get_device_name(),
                          compute_units=torch.cuda.get_device_properties(0).multi_processor_count, results=out)))


if __name__ == "__main__":
    main()
