"""Milliseconds of ONE irotavg_window_solve_batch_dev call next to nb successive irotavg_window_solve calls on the same
problems, printed as one JSON line (docs/window_batch.md). Two problem sizes:
  wave     the rotAvg(10) size: 12 views, 2 of them fixed, every view linked to its 4 predecessors (38 edges) -- the
           wave-resident kernel
  general  64 free views, 2 fixed, every view linked to its 11 predecessors, cut at 640 edges -- the general LDS kernel
and nb in {1, 16, 64, 256, 1024, 4096} problems that differ in their noise. Per (size, nb), in one run: a warm-up of both,
then --reps (>= 5) alternating repetitions; median, min and max. The batched figure is host time around the raw C call
(which blocks) and a synchronise of the stream, with the inputs on the device already; the loop's is host time around
its nb calls on host arrays. `bitwise_equal` compares Q and the weights of the two; `batch_not_slower` the medians;
`us_per_problem` is the batched median over nb.
Usage: python tools/time_window_batch.py [--reps N] [--nb 1,16,...] [--sizes wave,general]"""
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

from irotavg_amd import capi, synth  # noqa: E402

SIZES = {"wave": (12, 2, 4, None), "general": (66, 2, 11, 640)}   # views, fixed, predecessors, edge cap
NB = [1, 16, 64, 256, 1024, 4096]
SIGMA = 5 * np.pi / 180


def topology(nv, back, cap):
    E = [(v - d, v) for d in range(1, back + 1) for v in range(d, nv)]   # a cap drops the longest links of the last views
    return np.array(E[:cap] if cap else E, dtype=np.int32)


def problems(size, nb, seed=1):
    nv, f, back, cap = SIZES[size]
    I = topology(nv, back, cap)
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nb):
        Qgt = rng.normal(size=(nv, 4))
        Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
        QQ = synth.qmul(synth.qexp(rng.normal(scale=0.01, size=(len(I), 3))),
                        synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]])))
        Q0 = synth.qmul(synth.qexp(rng.normal(scale=0.05, size=(nv, 3))), Qgt)
        Q0[:f] = Qgt[:f]
        out.append((QQ, Q0))
    return I, nv, f, out


def summary(ts):
    return dict(median=round(float(np.median(ts)), 3), min=round(float(np.min(ts)), 3), max=round(float(np.max(ts)), 3))


def time_case(size, nb, reps):
    L = capi.lib()
    I, nv, f, P = problems(size, nb)
    m = len(I)
    device = torch.device("cuda", torch.cuda.current_device())
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    # the loop's host arrays (column-major, as irotavg_window_solve takes them)
    Ih = capi.edges(I)
    QQh = [capi.fmat(qq) for qq, _ in P]
    Q0h = [capi.fmat(q) for _, q in P]
    Qh = [q.copy(order="F") for q in Q0h]
    wh = [np.zeros(m) for _ in P]
    a, b = C.c_int(0), C.c_int(0)
    # the batch's device arrays
    sizes = np.tile(np.array([[nv, f, m]], dtype=np.int32), (nb, 1))
    ei = torch.tensor(np.tile(I, (nb, 1)), dtype=torch.int32, device=device)
    qq = torch.tensor(np.concatenate([x for x, _ in P]), dtype=torch.float64, device=device)
    q0 = torch.tensor(np.concatenate([x for _, x in P]), dtype=torch.float64, device=device)
    q = q0.clone()
    w = torch.zeros(nb * m, dtype=torch.float64, device=device)
    res = np.zeros((nb, 4), dtype=np.int32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())

    def loop():
        for k in range(nb):
            np.copyto(Qh[k], Q0h[k])
        t0 = time.perf_counter()
        for k in range(nb):
            rc = L.irotavg_window_solve(m, nv, f, Ih.ctypes.data_as(ip), QQh[k].ctypes.data_as(dp), m,
                                        Qh[k].ctypes.data_as(dp), nv, 4, SIGMA, 100, 100, 1e-3, wh[k].ctypes.data_as(dp),
                                        C.byref(a), C.byref(b))
            if rc:
                raise capi.IrotavgError(rc, "irotavg_window_solve")
        return 1e3 * (time.perf_counter() - t0)

    def batch():
        q.copy_(q0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.irotavg_window_solve_batch_dev(nb, sizes.ctypes.data_as(C.POINTER(C.c_int32)), vp(ei), vp(qq), 4, 1, vp(q), 4,
                                              1, 4, SIGMA, 100, 100, 1e-3, vp(w), res.ctypes.data_as(C.POINTER(C.c_int32)),
                                              0, stream)
        torch.cuda.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if rc:
            raise capi.IrotavgError(rc, "irotavg_window_solve_batch_dev")
        return dt

    ts = {loop: [], batch: []}
    for r in range(reps + 1):
        for fn in (loop, batch):
            dt = fn()
            if r > 0:  # r == 0 is the warm-up
                ts[fn].append(dt)
    same = (np.concatenate([np.ascontiguousarray(x) for x in Qh]).tobytes() == q.cpu().numpy().tobytes()
            and np.concatenate(wh).tobytes() == w.cpu().numpy().tobytes())
    lo, ba = summary(ts[loop]), summary(ts[batch])
    return dict(views=nv, fixed=f, edges=m, kernel=int(res[0, 3]), l1_iters=[int(res[:, 1].min()), int(res[:, 1].max())],
                irls_iters=[int(res[:, 2].min()), int(res[:, 2].max())], loop_ms=lo, batch_ms=ba,
                us_per_problem=round(1e3 * ba["median"] / nb, 2), batch_not_slower=bool(ba["median"] <= lo["median"]),
                bitwise_equal=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nb", default=",".join(str(n) for n in NB))
    ap.add_argument("--sizes", default="wave,general")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    out = {}
    for size in a.sizes.split(","):
        out[size] = {}
        for nb in (int(x) for x in a.nb.split(",")):
            out[size][str(nb)] = time_case(size, nb, a.reps)
    print(json.dumps(dict(tool="time_window_batch", reps=a.reps, device=torch.cuda.get_device_name(),
                          compute_units=torch.cuda.get_device_properties(0).multi_processor_count, results=out)))


if __name__ == "__main__":
    main()
