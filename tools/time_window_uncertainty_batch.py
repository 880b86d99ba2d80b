"""Milliseconds of ONE irotavg_window_uncertainty_batch_dev call next to the route the library offered before it for the
same numbers: per problem a handle from device arrays (TorchGraph), its rotations and weights set, variance() and
edge_diagnostics() on the dense route. One JSON line (docs/window_uncertainty_batch.md). Two problem sizes:
  window   the rotAvg(10) size: 12 views, 2 of them fixed, every view linked to its 4 predecessors (38 edges)
  general  64 free views, 2 fixed, every view linked to its 11 predecessors, cut at 640 edges
and nb in {1, 2, 16, 64, 256, 1024, 4096} problems that differ in their noise. The rotations and weights are what
window_solve_batch leaves for them (computed once, outside the timed region). Per (size, nb), in one run: a warm-up of
both, then --reps (>= 5) alternating repetitions; median, min and max. Both figures are host time around calls that end
in a synchronise of the stream, with every input on the device already. The loop is timed over the first
min(nb, --loop-cap) problems and reported per problem (`loop_us_per_problem`); `loop_ms` scales that to nb and says so in
`loop_problems_timed`. `max_rel_diff` compares var, edge_var, leverage, chi2 and the scale of the two over the problems
the loop ran (NaN / inf / 0 positions must agree); `agree` is max_rel_diff < 1e-9; `batch_faster` compares the medians.
Usage: python tools/time_window_uncertainty_batch.py [--reps N] [--nb 1,2,...] [--sizes window,general] [--loop-cap N]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from irotavg_amd import torch_api  # noqa: E402
from time_window_batch import problems  # noqa: E402

SIZES = {"window": "wave", "general": "general"}   # the problem generators of tools/time_window_batch.py
NB = [1, 2, 16, 64, 256, 1024, 4096]
SIGMA = 5 * np.pi / 180
KEYS = ("var", "edge_var", "leverage", "chi2")


def summary(ts):
    return dict(median=round(float(np.median(ts)), 3), min=round(float(np.min(ts)), 3), max=round(float(np.max(ts)), 3))


def rel_diff(a, b):
    """max relative difference where b is finite and non-zero; inf where the NaN / inf / 0 positions differ"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    for cls in (np.isnan, np.isposinf, lambda x: x == 0):
        if not np.array_equal(cls(a), cls(b)):
            return float("inf")
    fin = np.isfinite(b) & (b != 0)
    return float((np.abs(a[fin] - b[fin]) / np.abs(b[fin])).max()) if fin.any() else 0.0


def time_case(size, nb, reps, loop_cap):
    I, nv, f, P = problems(SIZES[size], nb)
    m = len(I)
    device = torch.device("cuda", torch.cuda.current_device())
    sizes = np.tile(np.array([[nv, f, m]], dtype=np.int32), (nb, 1))
    ei = torch.tensor(np.tile(I, (nb, 1)), dtype=torch.int32, device=device)
    one = ei[:m].contiguous()
    qq = torch.tensor(np.concatenate([x for x, _ in P]), dtype=torch.float64, device=device)
    q = torch.tensor(np.concatenate([x for _, x in P]), dtype=torch.float64, device=device)
    w = torch_api.window_solve_batch(sizes, ei, qq, q, 4, SIGMA)["weights"]
    outs = {k: torch.empty(nb * (nv if k == "var" else m), dtype=torch.float64, device=device) for k in KEYS}
    nloop = min(nb, loop_cap)
    loop_out = []

    def loop():
        del loop_out[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(nloop):
            g = torch_api.TorchGraph(one, qq[k * m:(k + 1) * m], nv, f)
            g.set_rotations(q[k * nv:(k + 1) * nv])
            g.set_weights(w[k * m:(k + 1) * m])
            v = g.variance()
            e = g.edge_diagnostics()
            loop_out.append((v, e))
            g.close()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    last = {}

    def batch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = torch_api.window_uncertainty_batch(sizes, ei, qq, q, w, SIGMA, None, None, outs["var"], outs["edge_var"],
                                               outs["leverage"], outs["chi2"])
        torch.cuda.synchronize()
        last["r"] = r
        return 1e3 * (time.perf_counter() - t0)

    ts = {loop: [], batch: []}
    for r in range(reps + 1):
        for fn in (loop, batch):
            dt = fn()
            if r > 0:  # r == 0 is the warm-up
                ts[fn].append(dt)
    host = {k: outs[k].cpu().numpy() for k in KEYS}
    worst = 0.0
    for k, (v, e) in enumerate(loop_out):
        worst = max(worst, rel_diff(host["var"][k * nv:(k + 1) * nv], v["var"].cpu().numpy()))
        for name in KEYS[1:]:
            worst = max(worst, rel_diff(host[name][k * m:(k + 1) * m], e[name].cpu().numpy()))
        worst = max(worst, rel_diff([last["r"]["scale"][k]], [v["scale"]]), rel_diff([last["r"]["scale"][k]], [e["scale"]]))
    lo, ba = summary(ts[loop]), summary(ts[batch])
    per = 1e3 * lo["median"] / nloop
    scaled = {k: round(v * nb / nloop, 3) for k, v in lo.items()}
    return dict(views=nv, fixed=f, edges=m, loop_problems_timed=nloop, loop_us_per_problem=round(per, 2), loop_ms=scaled,
                batch_ms=ba, us_per_problem=round(1e3 * ba["median"] / nb, 2),
                batch_faster=bool(ba["median"] < scaled["median"]), max_rel_diff=worst, agree=bool(worst < 1e-9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nb", default=",".join(str(n) for n in NB))
    ap.add_argument("--sizes", default="window,general")
    ap.add_argument("--loop-cap", type=int, default=128)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    out = {}
    for size in a.sizes.split(","):
        out[size] = {}
        for nb in (int(x) for x in a.nb.split(",")):
            out[size][str(nb)] = time_case(size, nb, a.reps, a.loop_cap)
    print(json.dumps(dict(tool="time_window_uncertainty_batch", reps=a.reps, device=torch.cuda.get_device_name(),
                          compute_units=torch.cuda.get_device_properties(0).multi_processor_count, results=out)))


if __name__ == "__main__":
    main()
