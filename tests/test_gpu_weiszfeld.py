"""irotavg_weiszfeld / irotavg_weiszfeld_dev (irotavg_amd/csrc/sweep.hip, sweep.hpp, devapi.hip; torch_api.weiszfeld;
docs/local_sweeps.md): Weiszfeld sweeps over the sorted half-edges, on the device.

The reference is the definition restated here in np.longdouble from dictionaries of neighbours, independent of sweep.hpp
and of any sort. The device rotation of every free view is compared with the reference's by the angle between them; step is
held to the same tolerance and info must be equal.

Tolerance. The same restatement run in float64 differs from the long-double one, measured on the CPU, by at most 1.21e-15
rad on every graph of this file but the behavioural one (the largest: star7, L2, two sweeps): 100 times that is below the
floor, so TOL = 1e-12 rad (the project's rule from test_gpu_cycle_cemp.py). On the behavioural graph 20 L1 sweeps differ by
5.89e-10 rad (a tree start leaves the tree edges with residual 0: their coefficients sit at 1 / floor and a last-bit
difference is multiplied by 1e6), so that graph alone has TOL_PLANTED = 5.89e-8 rad. The factor covers another atan2 /
sincos and another summation order. The only discontinuity of the definition is the wrap at pi: every graph here keeps the
reference's own residual angles below 3 rad at every sweep and inner iteration, and the reference asserts it.

The behavioural graph is planted(seed=25): the first seed from 0 on at which the reference keeps that condition through 20 L1
and 20 L2 sweeps (most seeds turn an edge by more than 3 rad). Mean angle to the ground truth, aligned at view 0, in the
reference: 0.39960 rad from the rank-free tree, 0.18145 rad after 20 L1 sweeps, 0.21799 rad after 20 L2 sweeps."""
import ctypes as C

import numpy as np
import pytest
import torch

from irotavg_amd import capi, torch_api

pytestmark = pytest.mark.gpu
TOL = max(100 * 1.21e-15, 1e-12)
TOL_PLANTED = max(100 * 5.89e-10, 1e-12)
G, STAGE = 8, 48                                                 # the group width and staging cap sweep.hip is compiled with
LD = np.longdouble


def t64(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def t32(a):
    return t64(a, torch.int32)


def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def conj(q):
    return q * np.array([-1, -1, -1, 1], dtype=q.dtype)


def qexp(r):
    r = np.asarray(r)
    th = np.sqrt((r * r).sum(-1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.concatenate([np.where(th > 0, r * np.sin(th / 2) / th, 0 * r), np.cos(th / 2)], axis=-1)


def angle(a, b):
    d = qmul(conj(a), b)
    return 2 * np.arctan2(np.sqrt((d[..., :3] ** 2).sum(-1)), np.abs(d[..., 3]))


def reference(I, QQ, Q, f=1, w=None, cost="l1", sweeps=1, inner=1, floor=1e-6, real=LD):
    pi = real(np.pi) if real is np.float64 else 4 * np.arctan(LD(1))
    QQ, Q, nb = QQ.astype(real), Q.astype(real), {}
    for k, (a, b) in enumerate(np.asarray(I).tolist()):
        if a != b:
            nb.setdefault(a, []).append((b, k, -1))                  # the half-edge a -> b: q(k, b -> a) has w negated
            nb.setdefault(b, []).append((a, k, 1))
    step = np.zeros(sweeps, dtype=real)
    for t in range(sweeps):
        new = Q.copy()
        for v in range(f, len(Q)):
            row = sorted(nb.get(v, []), key=lambda e: e[0])        # neighbours ascending, parallel edges in edge order
            if not row:
                continue
            u, k, sg = (np.array(c) for c in zip(*row))
            P = qmul(QQ[k] * np.stack([1 + 0 * sg, 1 + 0 * sg, 1 + 0 * sg, sg], 1).astype(real), Q[u])
            wk = np.ones(len(k), dtype=real) if w is None else np.asarray(w, dtype=real)[k]
            y = Q[v]
            for j in range(inner):
                with np.errstate(invalid="ignore", divide="ignore"):
                    d = qmul(conj(y), P)
                    s = np.sqrt((d[:, :3] ** 2).sum(1))
                    th = 2 * np.arctan2(s, d[:, 3])
                    th = np.where(th >= pi, th - 2 * pi, th)
                    assert (np.abs(th[np.isfinite(th)]) < 3).all(), "a residual near the wrap at pi"
                    r = np.where((s < 2.2204e-16)[:, None], 0, d[:, :3] * (th / s)[:, None])
                    keep = np.isfinite(r).all(1) & np.isfinite(wk) & (wk > 0)
                    rho = np.sqrt((r ** 2).sum(1))
                    c = np.where(keep, wk / np.maximum(rho, real(floor)) if cost == "l1" else wk, 0)
                x = (c[keep, None] * r[keep]).sum(0) / c[keep].sum() if keep.any() else np.zeros(3, dtype=real)
                if j == 0:
                    step[t] = np.fmax(step[t], np.sqrt((x * x).sum()))
                y = qmul(y, qexp(x))
            new[v] = y
        Q = new
    rows = [len(nb.get(v, [])) for v in range(f, len(Q))]
    return dict(Q=Q, step=step, info=dict(half_edges=sum(rows), empty_rows=rows.count(0)))


def run_dev(g, Q0, **kw):
    Q, w = t64(Q0), kw.pop("w", None)
    r = torch_api.weiszfeld(t32(g["I"]), t64(g["QQ"]), len(Q0), Q, w=None if w is None else t64(w), **kw)
    torch.cuda.synchronize()
    return dict(Q=Q.cpu().numpy(), step=r["step"], info=r["info"])


def check(g, Q0, tol=TOL, **kw):
    """the device against the reference: every free view, step, info; the fixed rows bitwise as they were"""
    r, e = run_dev(g, Q0, **kw), reference(g["I"], g["QQ"], Q0, **kw)
    f = kw.get("f", 1)
    worst = float(angle(r["Q"][f:].astype(LD), e["Q"][f:]).max()) if f < len(Q0) else 0.0
    dstep = float(np.abs(np.array(r["step"], dtype=LD) - e["step"]).max()) if len(e["step"]) else 0.0
    print("%s %s: worst angle %.3e rad, worst step difference %.3e" % (g["name"], kw, worst, dstep))
    assert r["Q"][:f].tobytes() == Q0[:f].tobytes() and r["info"] == e["info"]
    assert worst <= tol and dstep <= tol
    return r, e


def unit(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def graph(name, I, Qgt, noise=0.0, seed=0):
    """measurements Q_b (x) inverse(Q_a), each turned by about `noise` rad"""
    I, rng = np.array(I, dtype=np.int32).reshape(-1, 2), np.random.default_rng(seed)
    QQ = qmul(qexp(noise * rng.normal(size=(len(I), 3))), qmul(Qgt[I[:, 1]], conj(Qgt[I[:, 0]])))
    return dict(name=name, I=I, QQ=np.ascontiguousarray(QQ), Qgt=Qgt)


def start(g, spread=0.2, seed=1):
    return np.ascontiguousarray(qmul(g["Qgt"], qexp(spread * np.random.default_rng(seed).normal(size=(len(g["Qgt"]), 3)))))


def star(d):
    """view 0 fixed, the leaves 1 .. d (edges in alternating directions), the centre d + 1 with a self loop"""
    I = [(l, d + 1) if l % 2 else (d + 1, l) for l in range(1, d + 1)] + [(d + 1, d + 1)] + [(0, 1)] * (d > 0)
    return graph("star%d" % d, I, unit(np.random.default_rng(d), d + 2), 0.05)


def ring(n):
    """a ring with chords; a parallel and a reversed duplicate edge, a self loop, and a chord whose QQ row holds a NaN"""
    I = [(i, (i + 1) % n) for i in range(n)] + [(i, (i + 5) % n) for i in range(0, n, 3)] + [(1, 2), (2, 1), (4, 4)]
    g = graph("ring%d" % n, I, unit(np.random.default_rng(n), n), 0.05)
    g["QQ"][n, 1] = np.nan
    return g


def planted(seed=25, n=48, bw=6, p_out=0.1, noise=0.01):
    """the separation graph of test_gpu_cycle_cemp.py: every pair of views at distance <= bw joined, 0.01 rad noise, 10 % of
    the edges turned by a further 0.5 .. pi rad about a random axis"""
    rng = np.random.default_rng(seed)
    I = np.array([(a, b) for a in range(n) for b in range(a + 1, min(n, a + bw + 1))], dtype=np.int32)
    g = graph("planted", I, unit(rng, n))
    axis = unit(rng, len(I))[:, :3]
    ang = noise * rng.normal(size=len(I)) + np.where(rng.random(len(I)) < p_out, rng.uniform(0.5, np.pi, size=len(I)), 0.0)
    g["QQ"] = qmul(qexp(axis / np.linalg.norm(axis, axis=1, keepdims=True) * ang[:, None]), g["QQ"])
    return g


RING = ring(12)


@pytest.mark.parametrize("cost", ["l1", "l2"])
def test_one_free_view_whose_predictions_agree_lands_on_them(cost):
    g = graph("agree", [(0, 3), (3, 1), (2, 3)], unit(np.random.default_rng(5), 4))
    Q0 = g["Qgt"].copy()
    Q0[3] = start(g, 0.5)[3]
    r, _ = check(g, Q0, f=3, cost=cost, sweeps=1)
    assert angle(r["Q"][3], g["Qgt"][3]) <= TOL


@pytest.mark.parametrize("cost", ["l1", "l2"])
def test_a_consistent_graph_is_a_fixed_point(cost):
    g = graph("consistent", RING["I"], RING["Qgt"])
    r, _ = check(g, g["Qgt"].copy(), cost=cost, sweeps=3, inner=2)
    assert max(r["step"]) <= TOL and angle(r["Q"], g["Qgt"]).max() <= TOL


def test_two_agreeing_neighbours_and_one_a_radian_off():
    g = graph("two and one", [(0, 3), (1, 3), (2, 3)], unit(np.random.default_rng(6), 4))
    g["QQ"][2] = qmul(qmul(g["Qgt"][3], qexp(np.array([1.0, 0, 0]))), conj(g["Qgt"][2]))     # view 2 predicts A (x) exp(1 rad)
    r, _ = check(g, g["Qgt"].copy(), f=3, cost="l2", sweeps=1)
    assert abs(angle(r["Q"][3], g["Qgt"][3]) - 1 / 3) <= TOL                                 # the mean: a third of the way
    Q0 = g["Qgt"].copy()
    Q0[3] = qmul(Q0[3], qexp(np.array([0, 1e-3, 0])))               # (the distance to the pair halves per inner iteration)
    r, _ = check(g, Q0, f=3, cost="l1", sweeps=1, inner=16)
    assert 1e-7 < angle(r["Q"][3], g["Qgt"][3]) <= 1e-6             # the median: the pair, to within the floor (1 / (2 / floor + 1))


@pytest.mark.parametrize("cost", ["l1", "l2"])
@pytest.mark.parametrize("inner", [1, 3])
@pytest.mark.parametrize("d", [0, 1, G - 1, G, G + 1, STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 3])
def test_row_lengths_across_the_group_width_and_the_staging_cap(d, inner, cost):
    g = star(d)
    _, e = check(g, start(g), cost=cost, sweeps=2, inner=inner)
    assert e["info"] == dict(half_edges=2 * d + (d > 0), empty_rows=int(d == 0))


@pytest.mark.parametrize("nfree", [1, 31, 32, 33, 129])
def test_free_views_around_a_workgroup_pass(nfree):
    g = ring(nfree + 8)                      # 1: the lone chunk is a single view; 129: the last pass of the last chunk is
    check(g, start(g), f=8, sweeps=2, inner=2)


@pytest.mark.parametrize("f", [1, 3, 12])
@pytest.mark.parametrize("sweeps", [1, 2, 3])
def test_both_parities_of_the_planes_and_the_fixed_views(sweeps, f):
    r, _ = check(RING, start(RING), f=f, sweeps=sweeps)
    assert f < 12 or r["step"] == [0.0] * sweeps


def test_weights_that_leave_terms_out_and_empty_a_row_and_a_residual_below_the_floor():
    w = np.linspace(0.5, 2.0, len(RING["I"]))
    check(RING, start(RING), w=w, sweeps=2, cost="l2")
    mine = [k for k, (a, b) in enumerate(RING["I"].tolist()) if 8 in (a, b)]
    assert len(mine) == 3                                          # view 8: (7, 8), (8, 9) and the chord (3, 8)
    w[mine] = [0.0, -1.0, np.nan]
    Q0 = start(RING)
    r, _ = check(RING, Q0, w=w, sweeps=2, inner=2)
    assert r["Q"][8].tobytes() == Q0[8].tobytes()                  # no term left: the view keeps its rotation
    g = graph("near", RING["I"], RING["Qgt"])
    r, e = check(g, start(g, 1e-4), sweeps=2, floor=1e-3)
    assert 0 < max(e["step"]) < 1e-3


def raw(g, I, Q, sweeps=2, step=None, info=None, stream=None, f=1):
    ei, qq = t32(I), t64(g["QQ"])
    rc = capi.lib().irotavg_weiszfeld_dev(len(I), len(Q), f, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1,
                                          C.c_void_p(Q.data_ptr()), int(Q.stride(0)), int(Q.stride(1)), None, 1, sweeps, 1, 1e-6,
                                          step, info, stream)
    torch.cuda.synchronize()
    return rc


def test_layouts_null_step_no_sweep_a_bad_id_the_host_form_and_two_calls():
    g, Q0 = RING, start(RING)
    want = run_dev(g, Q0, sweeps=2)
    planes, qq_planes = t64(Q0.T).t(), t64(g["QQ"].T).t()          # column-major: strides (1, n)
    r = torch_api.weiszfeld(t64(g["I"], torch.int64), qq_planes, 12, planes, sweeps=2, step=False)
    assert r["step"] is None and planes.cpu().numpy().tobytes() == want["Q"].tobytes()       # either layout, two calls
    Q, info = t64(Q0), (C.c_int64 * 2)(-1, -2)
    assert raw(g, g["I"], Q, sweeps=0, info=info) == capi.OK and list(info) == [want["info"]["half_edges"], 0]
    assert raw(g, g["I"], Q, sweeps=0) == capi.OK and Q.cpu().numpy().tobytes() == Q0.tobytes()
    bad = g["I"].copy()
    bad[-1, 1] = 12
    step = (C.c_double * 2)(-1.0, -2.0)
    assert raw(g, bad, Q, step=step, info=info) == capi.ERR_BAD_ARG == raw(g, bad, Q, sweeps=0)
    assert Q.cpu().numpy().tobytes() == Q0.tobytes() and list(step) == [-1.0, -2.0] and info[0] == want["info"]["half_edges"]
    assert raw(g, g["I"], Q, step=step) == capi.OK and Q.cpu().numpy().tobytes() == want["Q"].tobytes()
    assert list(step) == want["step"]
    h = capi.weiszfeld(g["I"], g["QQ"], 12, Q0.copy(), sweeps=2)     # the host form stages through the same kernels
    assert h["Q"].tobytes() == want["Q"].tobytes() and h["step"].tolist() == want["step"] and h["info"] == want["info"]


def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream():
    g, Q0 = RING, start(RING)
    want = run_dev(g, Q0, sweeps=3)
    ei, qq, half = t32(g["I"]), t64(g["QQ"]), t64(Q0 * 0.5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        Q = half * 2.0                                             # exact: the start of the synchronised run, produced on the stream
        torch_api.weiszfeld(ei, qq, 12, Q, sweeps=3)
        doubled = Q * 2                                            # consumed right behind the call, no synchronise
    side.synchronize()
    assert Q.cpu().numpy().tobytes() == want["Q"].tobytes() and (doubled.cpu().numpy() == 2 * want["Q"]).all()


def test_l1_sweeps_after_init_tree_beat_the_tree_and_the_mean():
    g = planted()
    ei, qq, Q = t32(g["I"]), t64(g["QQ"]), t64(np.zeros((48, 4)))
    Q[:, 3] = 1.0
    torch_api.init_tree(ei, qq, 48, Q)
    Q0 = Q.cpu().numpy()

    def err(q):
        return float(angle(qmul(q, conj(q[0])), qmul(g["Qgt"], conj(g["Qgt"][0]))).mean())
    l1, _ = check(g, Q0, TOL_PLANTED, cost="l1", sweeps=20)
    l2, _ = check(g, Q0, TOL_PLANTED, cost="l2", sweeps=20)
    print("mean angle to the truth: tree %.5f, 20 L1 sweeps %.5f, 20 L2 sweeps %.5f" % (err(Q0), err(l1["Q"]), err(l2["Q"])))
    assert err(l1["Q"]) < err(Q0) and err(l1["Q"]) < err(l2["Q"])
