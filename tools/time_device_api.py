"""Milliseconds per call of the device-pointer handle API next to its host-pointer sibling, printed as one JSON line
(docs/device_api.md). Per case, in ONE run and -- create apart -- on ONE handle (built by irotavg_graph_create_dev,
weights of one irls, GM 5 deg):
  create            irotavg_graph_create (host arrays)            vs  irotavg_graph_create_dev (tensors on the device)
  edge_diagnostics  irotavg_graph_edge_diagnostics (3 arrays)     vs  irotavg_graph_edge_diagnostics_dev
  variance          irotavg_graph_rotation_variance (marginals)   vs  irotavg_graph_rotation_variance_dev
  get_rotations     irotavg_graph_get_rotations                   vs  irotavg_graph_get_rotations_dev
Every figure is host time around the raw C call into preallocated buffers, the device calls followed by a synchronise
of the caller's stream (the copy calls return before their work has run); the two calls of a pair alternate, after one
warm-up call each: median, min and max of --reps (>= 5) repetitions. `dev_not_slower` compares the medians.
  Cases: 100k views / 2M edges band-only and with 100 loop closures, 1M views / 20M edges band-only.
Usage: python tools/time_device_api.py [--reps N] [--only NAME[,NAME]]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from irotavg_amd import capi  # noqa: E402
from irotavg_amd.torch_api import TorchGraph  # noqa: E402
from time_rotation_variance import CASES as VARIANCE_CASES  # noqa: E402

CASES = ["100k_2M_band", "100k_2M_100cl", "1M_20M_band"]


def summary(ts):
    return dict(median=round(float(np.median(ts)), 3), min=round(float(np.min(ts)), 3), max=round(float(np.max(ts)), 3))


def pair(host_fn, dev_fn, reps, after=lambda fn: None):
    """The two calls alternate (host, dev, host, dev, ...) after one warm-up each; `after` runs untimed behind each."""
    ts = {host_fn: [], dev_fn: []}
    for r in range(reps + 1):
        for fn in (host_fn, dev_fn):
            t0 = time.perf_counter()
            fn()
            dt = 1e3 * (time.perf_counter() - t0)
            after(fn)
            if r > 0:  # r == 0 is the warm-up
                ts[fn].append(dt)
    host, dev = summary(ts[host_fn]), summary(ts[dev_fn])
    return dict(host=host, dev=dev, dev_not_slower=bool(dev["median"] <= host["median"]))


def time_case(name, reps):
    I, QQ, Q, n, f = VARIANCE_CASES[name]()
    L = capi.lib()
    device = torch.device("cuda", torch.cuda.current_device())
    I = capi.edges(I)
    QQf = capi.fmat(QQ)
    m = len(I)
    ei = torch.tensor(I, device=device)
    qq = torch.tensor(np.ascontiguousarray(QQ), dtype=torch.float64, device=device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    o = capi.default_options()
    out = dict(m=m, n=n)

    def create_host():
        h = C.c_void_p()
        capi.check(L.irotavg_graph_create(C.byref(h), m, n, f, capi._i(I), capi._d(QQf), m, C.byref(o)), "create")
        create_host.h = h

    def create_dev():
        h = C.c_void_p()
        capi.check(L.irotavg_graph_create_dev(C.byref(h), m, n, f, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()),
                                              4, 1, C.byref(o), stream), "create_dev")
        torch.cuda.synchronize()
        create_dev.h = h

    out["create"] = pair(create_host, create_dev, reps, after=lambda fn: L.irotavg_graph_destroy(fn.h))

    with TorchGraph(ei, qq, n, f) as G:
        G.set_rotations(torch.tensor(np.ascontiguousarray(Q), dtype=torch.float64, device=device))
        G.irls(4, 5 * np.pi / 180, 50, 1e-3)
        out["band_block"] = G.stats()["band_block"]
        out["closures"] = G.direct_info()["closures"]
        h = G._h
        s = C.c_double(0)
        he = [np.zeros(m) for _ in range(3)]
        de = [torch.zeros(m, dtype=torch.float64, device=device) for _ in range(3)]

        def ed_host():
            capi.check(L.irotavg_graph_edge_diagnostics(h, *[capi._d(a) for a in he], C.byref(s)), "edge_diagnostics")

        def ed_dev():
            capi.check(L.irotavg_graph_edge_diagnostics_dev(h, *[C.c_void_p(t.data_ptr()) for t in de], C.byref(s), stream),
                       "edge_diagnostics_dev")
            torch.cuda.synchronize()

        out["edge_diagnostics"] = pair(ed_host, ed_dev, reps)
        out["edge_diagnostics"]["bitwise_equal"] = all(np.array_equal(a, t.cpu().numpy(), equal_nan=True)
                                                       for a, t in zip(he, de))
        hv = np.zeros(n)
        dv = torch.zeros(n, dtype=torch.float64, device=device)
        pv = np.zeros(1)

        def var_host():
            capi.check(L.irotavg_graph_rotation_variance(h, capi._d(hv), 0, None, capi._d(pv), C.byref(s)), "variance")

        def var_dev():
            capi.check(L.irotavg_graph_rotation_variance_dev(h, C.c_void_p(dv.data_ptr()), C.byref(s), stream),
                       "variance_dev")
            torch.cuda.synchronize()

        out["variance"] = pair(var_host, var_dev, reps)
        out["variance"]["bitwise_equal"] = bool(np.array_equal(hv, dv.cpu().numpy()))
        hq = np.zeros((n, 4), order="F")
        dq = torch.zeros((n, 4), dtype=torch.float64, device=device)

        def rot_host():
            capi.check(L.irotavg_graph_get_rotations(h, capi._d(hq), n), "get_rotations")

        def rot_dev():
            capi.check(L.irotavg_graph_get_rotations_dev(h, C.c_void_p(dq.data_ptr()), 4, 1, stream), "get_rotations_dev")
            torch.cuda.synchronize()

        out["get_rotations"] = pair(rot_host, rot_dev, reps)
        out["get_rotations"]["bitwise_equal"] = bool(np.array_equal(hq, dq.cpu().numpy()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    out = {}
    for name in CASES:
        if a.only and name not in a.only.split(","):
            continue
        out[name] = time_case(name, a.reps)
    print(json.dumps(dict(tool="time_device_api", reps=a.reps, results=out)))


if __name__ == "__main__":
    main()
