"""Milliseconds of ONE irotavg_window_gate_batch_dev call next to the loop of capi.window_gate (irotavg_window_gate, one
problem on host arrays) over the same problems. One JSON line (docs/window_gate_batch.md). Two problem sizes:
  window   the rotAvg(10) size: 12 views, 2 of them fixed, every view linked to its 4 predecessors (38 edges)
  general  64 free views, 2 fixed, every view linked to its 11 predecessors, cut at 640 edges
and nb in {1, 2, 16, 64, 256, 1024, 4096} problems that differ in their noise, 8 candidates each: random pairs of
distinct views, measured 0 .. 0.3 rad away from the poses. The rotations and weights are what window_solve_batch leaves
(computed once, outside the timed region). Per (size, nb), in one run: a warm-up of both, then --reps (>= 5) alternating
repetitions; median, min and max. The batch is host time around a call that ends in a synchronise of the stream, with
every input on the device already; the loop is host time around calls on host arrays (each one stages its problem
itself). By default the loop runs over all nb problems. With --loop-cap N > 0 it is timed over the first min(nb, N)
problems only and `loop_ms` is that time scaled to nb, an extrapolation that `loop_problems_timed` discloses
(`loop_us_per_problem` is the measured figure). `bitwise` says whether angle, pair_var, chi2 and the scale of the two are
equal bit for bit over the problems the loop ran; `batch_not_slower` compares the medians.
Usage: python tools/time_window_gate_batch.py [--reps N] [--nb 1,2,...] [--sizes window,general] [--loop-cap N]"""
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

from irotavg_amd import capi, synth, torch_api  # noqa: E402
from time_window_batch import problems  # noqa: E402

SIZES = {"window": "wave", "general": "general"}   # the problem generators of tools/time_window_batch.py
NB = [1, 2, 16, 64, 256, 1024, 4096]
SIGMA = 5 * np.pi / 180
KEYS = ("angle", "pair_var", "chi2")
NCAND = 8


def summary(ts):
    return dict(median=round(float(np.median(ts)), 3), min=round(float(np.min(ts)), 3), max=round(float(np.max(ts)), 3))


def candidates(nv, Q, rng):
    """NCAND pairs of distinct views and their measurements, 0 .. 0.3 rad away from the poses Q"""
    cI = np.array([rng.choice(nv, size=2, replace=False) for _ in range(NCAND)], dtype=np.int32)
    ax = rng.normal(size=(NCAND, 3))
    off = ax / np.linalg.norm(ax, axis=1, keepdims=True) * (0.3 * rng.random((NCAND, 1)))
    return cI, synth.qmul(synth.qexp(off), synth.qmul(Q[cI[:, 1]], synth.qconj(Q[cI[:, 0]])))


def time_case(size, nb, reps, loop_cap):
    I, nv, f, P = problems(SIZES[size], nb)
    m = len(I)
    device = torch.device("cuda", torch.cuda.current_device())
    sizes = np.tile(np.array([[nv, f, m]], dtype=np.int32), (nb, 1))
    ei = torch.tensor(np.tile(I, (nb, 1)), dtype=torch.int32, device=device)
    qq = torch.tensor(np.concatenate([x for x, _ in P]), dtype=torch.float64, device=device)
    q = torch.tensor(np.concatenate([x for _, x in P]), dtype=torch.float64, device=device)
    w = torch_api.window_solve_batch(sizes, ei, qq, q, 4, SIGMA)["weights"]
    Qh, wh = q.cpu().numpy(), w.cpu().numpy()
    rng = np.random.default_rng(5)
    cands = [candidates(nv, Qh[k * nv:(k + 1) * nv], rng) for k in range(nb)]
    ci = torch.tensor(np.concatenate([a for a, _ in cands]), dtype=torch.int32, device=device)
    cq = torch.tensor(np.concatenate([b for _, b in cands]), dtype=torch.float64, device=device)
    ncand = np.full(nb, NCAND, dtype=np.int32)
    outs = {k: torch.empty(nb * NCAND, dtype=torch.float64, device=device) for k in KEYS}
    nloop = min(nb, loop_cap) if loop_cap > 0 else nb
    loop_out = []

    def loop():
        del loop_out[:]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(nloop):
            loop_out.append(capi.window_gate(I, P[k][0], Qh[k * nv:(k + 1) * nv], f, cands[k][0], cands[k][1],
                                             weights=wh[k * m:(k + 1) * m], sigma=SIGMA))
        return 1e3 * (time.perf_counter() - t0)

    last = {}

    def batch():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = torch_api.window_gate_batch(sizes, ei, qq, q, ci, cq, ncand, w, SIGMA, outs["angle"], outs["pair_var"], outs["chi2"])
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
    same = True
    for k, g in enumerate(loop_out):
        for name in KEYS:
            same = same and host[name][k * NCAND:(k + 1) * NCAND].tobytes() == g[name].tobytes()
        same = same and np.array([last["r"]["scale"][k]]).tobytes() == np.array([g["scale"]]).tobytes()
    lo, ba = summary(ts[loop]), summary(ts[batch])
    per = 1e3 * lo["median"] / nloop
    scaled = {k: round(v * nb / nloop, 3) for k, v in lo.items()}
    return dict(views=nv, fixed=f, edges=m, candidates=NCAND, loop_problems_timed=nloop, loop_us_per_problem=round(per, 2),
                loop_ms=scaled, batch_ms=ba, us_per_problem=round(1e3 * ba["median"] / nb, 2),
                batch_not_slower=bool(ba["median"] <= scaled["median"]), bitwise=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nb", default=",".join(str(n) for n in NB))
    ap.add_argument("--sizes", default="window,general")
    ap.add_argument("--loop-cap", type=int, default=0, help="0: the loop runs over every problem")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    out = {}
    for size in a.sizes.split(","):
        out[size] = {}
        for nb in (int(x) for x in a.nb.split(",")):
            out[size][str(nb)] = time_case(size, nb, a.reps, a.loop_cap)
    print(json.dumps(dict(tool="time_window_gate_batch", reps=a.reps, device=torch.cuda.get_device_name(),
                          compute_units=torch.cuda.get_device_properties(0).multi_processor_count, results=out)))


if __name__ == "__main__":
    main()
