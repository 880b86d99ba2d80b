"""Milliseconds of ONE irotavg_window_init_mst_batch_dev call next to the route a caller with device arrays has without
it, printed as one JSON line (docs/window_init_batch.md). The route: copy I, QQ and Q from the device to the host, loop
irotavg_init_mst over the problems, copy Q back, synchronise. Two problem sizes:
  small  the rotAvg(10) size: 12 views, 2 of them fixed, every view linked to its 4 predecessors (38 edges)
  limit  320 views, 256 of them fixed, every view linked to its 2 predecessors (637 edges)
and nb in {1, 2, 4, 8, 16, 64, 256, 1024, 4096} problems that differ in their measurements. The edges of every problem are listed
in a random order (seeded): one sweep at `small`, 60 sweeps and a tree 184 edges deep at `limit`. Per (size, nb), in one run: a warm-up of both, then
--reps (>= 5) alternating repetitions; median, min and max. Both figures are host time from a synchronised device to a
synchronised device with Q on the device at either end; the batched call blocks by itself. `bitwise_equal` compares the Q
of the two; `batch_not_slower` the medians; `us_per_problem` is the batched median over nb.
Usage: python tools/time_window_init_batch.py [--reps N] [--nb 1,16,...] [--sizes small,limit]"""
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

from irotavg_amd import capi  # noqa: E402

SIZES = {"small": (12, 2, 4, None), "limit": (320, 256, 2, 640)}   # views, fixed, predecessors, edge cap
NB = [1, 2, 4, 8, 16, 64, 256, 1024, 4096]


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
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    unit = lambda n: (lambda q: q / np.linalg.norm(q, axis=1, keepdims=True))(rng.normal(size=(n, 4)))
    Q0 = np.full((nb * nv, 4), np.nan)                 # free rows are never read
    for b in range(nb):
        Q0[b * nv:b * nv + f] = unit(f)
    sizes = np.tile(np.array([[nv, f, m]], dtype=np.int32), (nb, 1))
    ei = torch.tensor(np.tile(I, (nb, 1)), dtype=torch.int32, device=device)
    qq = torch.tensor(unit(nb * m), dtype=torch.float64, device=device)
    q0 = torch.tensor(Q0, dtype=torch.float64, device=device)
    q_batch, q_route = q0.clone(), q0.clone()
    status = np.zeros(nb, dtype=np.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())

    def route():
        q_route.copy_(q0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Ih, QQh, Qh = ei.cpu().numpy(), qq.cpu().numpy(), q_route.cpu().numpy()   # three device-to-host copies
        for b in range(nb):
            # irotavg_init_mst takes column-major planes: one problem's rows, transposed
            Qp, QQp = np.asfortranarray(Qh[b * nv:(b + 1) * nv]), np.asfortranarray(QQh[b * m:(b + 1) * m])
            rc = L.irotavg_init_mst(nv, m, Qp.ctypes.data_as(dp), nv, QQp.ctypes.data_as(dp), m,
                                    Ih[b * m:(b + 1) * m].ctypes.data_as(ip), f)
            if rc:
                raise capi.IrotavgError(rc, "irotavg_init_mst")
            Qh[b * nv:(b + 1) * nv] = Qp
        q_route.copy_(torch.from_numpy(Qh))                                       # the copy back
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def batch():
        q_batch.copy_(q0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.irotavg_window_init_mst_batch_dev(nb, sizes.ctypes.data_as(ip), vp(ei), vp(qq), 4, 1, vp(q_batch), 4, 1,
                                                 status.ctypes.data_as(ip), stream)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if rc:
            raise capi.IrotavgError(rc, "irotavg_window_init_mst_batch_dev")
        return dt

    ts = {route: [], batch: []}
    for r in range(reps + 1):
        for fn in (route, batch):
            dt = fn()
            if r > 0:  # r == 0 is the warm-up
                ts[fn].append(dt)
    same = q_route.cpu().numpy().tobytes() == q_batch.cpu().numpy().tobytes()
    ro, ba = summary(ts[route]), summary(ts[batch])
    return dict(views=nv, fixed=f, edges=m, route_ms=ro, batch_ms=ba, us_per_problem=round(1e3 * ba["median"] / nb, 2),
                batch_not_slower=bool(ba["median"] <= ro["median"]), bitwise_equal=bool(same),
                nan_left=bool(np.isnan(q_batch.cpu().numpy()).any()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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
    print(json.dumps(dict(tool="time_window_init_batch", reps=a.reps, device=torch.cuda.get_device_name(),
                          compute_units=torch.cuda.get_device_properties(0).multi_processor_count, results=out)))


if __name__ == "__main__":
    main()
