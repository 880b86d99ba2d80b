"""Milliseconds of ONE irotavg_window_init_tree_batch_dev call next to the two routes a caller has without it, printed as
one JSON line (docs/window_init_tree_batch.md):
  mst   irotavg_window_init_mst_batch_dev on the same arrays: what the rank costs over the sweep
  loop  irotavg_init_tree_dev on every problem in turn, with f = 1 (view 0 the only anchor: the whole problem is one tree
        at handle size): what a caller with a rank has today
Two problem sizes, those of tools/time_window_init_batch.py:
  small  12 views, 2 of them fixed, every view linked to its 4 predecessors (38 edges)
  limit  320 views, 256 of them fixed, every view linked to its 2 predecessors (637 edges)
with seeded ranks in {0, 1, 2}, the edges of every problem listed in a seeded random order, and nb in {1, 16, 256, 4096}
problems that differ in their measurements. Per (size, nb), in one run: a warm-up of all three, then --reps (>= 7)
alternating repetitions; median, min and max. Every figure is host time from a synchronised device to a synchronised
device with all arrays on the device at either end. `us_per_problem` is the tree median over nb.
Usage: python tools/time_window_init_tree_batch.py [--reps N] [--nb 1,16,...] [--sizes small,limit]"""
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
    unit = lambda n: (lambda q: q / np.linalg.norm(q, axis=1, keepdims=True))(rng.normal(size=(n, 4)))
    Q0 = np.full((nb * nv, 4), np.nan)                 # free rows are never read
    for b in range(nb):
        Q0[b * nv:b * nv + f] = unit(f)
    sizes = np.tile(np.array([[nv, f, m]], dtype=np.int32), (nb, 1))
    ei = torch.tensor(np.tile(I, (nb, 1)), dtype=torch.int32, device=device)
    qq = torch.tensor(unit(nb * m), dtype=torch.float64, device=device)
    rank = torch.tensor(rng.integers(0, 3, nb * m), dtype=torch.int32, device=device)
    q0 = torch.tensor(Q0, dtype=torch.float64, device=device)
    q = {name: q0.clone() for name in ("tree", "mst", "loop")}
    res = np.zeros(4 * nb, dtype=np.int32)
    info = (C.c_int64 * 4)()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t, row=0: C.c_void_p(t.data_ptr() + row * t.stride(0) * t.element_size())

    def timed(name, body):
        q[name].copy_(q0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = body(q[name])
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if rc:
            raise capi.IrotavgError(rc, name)
        return dt

    def tree(Q):
        return L.irotavg_window_init_tree_batch_dev(nb, sizes.ctypes.data_as(ip), vp(ei), vp(qq), 4, 1, vp(rank), vp(Q), 4, 1,
                                                    None, res.ctypes.data_as(ip), stream)

    def mst(Q):
        return L.irotavg_window_init_mst_batch_dev(nb, sizes.ctypes.data_as(ip), vp(ei), vp(qq), 4, 1, vp(Q), 4, 1,
                                                   res.ctypes.data_as(ip), stream)

    def loop(Q):
        for b in range(nb):
            rc = L.irotavg_init_tree_dev(m, nv, 1, vp(ei, b * m), vp(qq, b * m), 4, 1, vp(rank, b * m), vp(Q, b * nv), 4, 1, None,
                                         info, stream)
            if rc:
                return rc
        return 0

    routes = dict(tree=tree, mst=mst, loop=loop)
    ts = {name: [] for name in routes}
    for r in range(reps + 1):
        for name, body in routes.items():
            dt = timed(name, body)
            if r > 0:  # r == 0 is the warm-up
                ts[name].append(dt)
    out = {name + "_ms": summary(t) for name, t in ts.items()}
    med = {name: out[name + "_ms"]["median"] for name in routes}
    return dict(views=nv, fixed=f, edges=m, us_per_problem=round(1e3 * med["tree"] / nb, 2),
                tree_over_mst=round(med["tree"] / med["mst"], 2), loop_over_tree=round(med["loop"] / med["tree"], 1),
                nan_left=bool(np.isnan(q["tree"].cpu().numpy()).any()), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nb", default=",".join(str(n) for n in NB))
    ap.add_argument("--sizes", default="small,limit")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("--reps must be at least 7")
    if capi.lib().irotavg_device_count() <= 0:
        raise SystemExit("no HIP device: nothing to time")
    out = {}
    for size in a.sizes.split(","):
        out[size] = {}
        for nb in (int(x) for x in a.nb.split(",")):
            out[size][str(nb)] = time_case(size, nb, a.reps)
    print(json.dumps(dict(tool="time_window_init_tree_batch", reps=a.reps, device=torch.cuda.get_device_name(),
                          compute_units=torch.cuda.get_device_properties(0).multi_processor_count, results=out)))


if __name__ == "__main__":
    main()
