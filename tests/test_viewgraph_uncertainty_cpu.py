"""View-graph uncertainty queries (irotavg_viewgraph_rotation_variance / _edge_diagnostics / _gate_connections,
docs/viewgraph_uncertainty.md): the NumPy reference the GPU tests compare against -- ViewGraphOracle's extraction, the
oracle's residuals, Geman-McClure weights at a zero step, then the references of the two handle queries --, its
properties, the planted-closure input of the GPU test run through the reference alone, and the ABI. No GPU."""
import os
import re

import numpy as np
import pytest

from irotavg_amd import capi, synth
from irotavg_amd.viewgraph import ViewGraph
from oracle import oracle as O
from oracle.viewgraph_oracle import ViewGraphOracle
from test_edge_diagnostics_cpu import band_edge_reference, edge_reference
from test_rotation_variance_cpu import band_reference, dense_reference
from test_viewgraph import build_sequence, rot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 5 * np.pi / 180


# ---- the reference ------------------------------------------------------------------------------------------------
def extract_problem(vo, winSize):
    """The problem ViewGraphOracle.rotAvg(winSize) would solve (oracle/viewgraph_oracle.py:42-81), not solved. With no
    fixed pose in it, row 0 keeps the pose it has (rotAvg would set the identity): a query moves nothing."""
    assert winSize > 2
    m = len(vo.R)
    win = min(m, winSize)
    if win < 2:
        return dict(skipped=1)
    E, qq, vertices = [], [], set()
    for j in range(m - win, m):
        for i in sorted(vo.conn[j]):
            if i < j:
                E.append((i, j))
                vertices.update((i, j))
                qq.append(O.rmat2quat(vo.conn[j][i]))
    ne, nv = len(qq), len(vertices)
    if ne < win:
        return dict(skipped=2)
    if nv < win:
        return dict(skipped=3)
    f = nv - win + sum(1 for x in vertices if x >= m - win and vo.fixed[x])
    v2i, i2v = {}, {}
    t, k = 0, f
    for x in sorted(vertices):
        if x >= m - win and not vo.fixed[x]:
            i2v[k] = x; v2i[x] = k; k += 1
        else:
            i2v[t] = x; v2i[x] = t; t += 1
    I = np.array([(v2i[a], v2i[b]) for a, b in E], dtype=np.int32)
    Q = np.zeros((nv, 4))
    for x in vertices:
        Q[v2i[x]] = O.rmat2quat(vo.R[x])
    f = max(f, 1)
    if nv - f < 1:
        return dict(skipped=4)
    return dict(skipped=0, I=I, conn=np.array(E, dtype=np.int32), QQ=np.array(qq), Q=Q, f=f, nv=nv, ne=ne, v2i=v2i,
                i2v=i2v)


def residuals(I, QQ, Q):
    return O.log_map(O.delta_rel(I, QQ, Q))[:, :3]


def viewgraph_uncertainty_reference(vo, winSize, pairs=(), cands=(), band_block=0):
    """Everything the three queries return. pairs: (i, j) view ids; cands: (i, j, R_ij) as connect takes them.
    band_block > 0: the block recurrences of test_rotation_variance_cpu.py instead of a dense inverse (large problems).
    `consistency` = ||M Sigma - I||_max of the dense route (how far the reference itself can be trusted)."""
    m = len(vo.R)
    nan = lambda n: np.full(n, np.nan)
    P = extract_problem(vo, winSize)
    if P["skipped"]:
        return dict(skipped=P["skipped"], var=nan(m), pair_var=nan(len(pairs)), n=0, angle=nan(len(cands)),
                    cand_var=nan(len(cands)), cand_chi2=nan(len(cands)), scale=np.nan)
    I, QQ, Q, f, nv, v2i = P["I"], P["QQ"], P["Q"], P["f"], P["nv"], P["v2i"]
    res = residuals(I, QQ, Q)
    d = 1.0 / (np.sum(res ** 2, axis=1) + SIGMA ** 2)
    # pairs and candidates as rows of the problem; (0, 0) stands in where a view is absent
    rows, absent, ang = [], [], []
    for a, b in pairs:
        absent.append(a not in v2i or b not in v2i)
        rows.append((0, 0) if absent[-1] else (v2i[a], v2i[b]))
    for a, b, R in cands:
        lo, hi = min(a, b), max(a, b)
        R = np.asarray(R, dtype=np.float64).reshape(3, 3)
        q3 = O.rmat2quat(R if a < b else R.T)
        r = residuals(np.array([[0, 1]], dtype=np.int32), q3[None], np.stack([O.rmat2quat(vo.R[lo]), O.rmat2quat(vo.R[hi])]))
        ang.append(np.linalg.norm(r))
        absent.append(lo not in v2i or hi not in v2i)
        rows.append((0, 0) if absent[-1] else (v2i[hi], v2i[lo]))
    if band_block:
        varl, pv, _ = band_reference(I, nv, f, d, band_block, rows)
        E = band_edge_reference(I, nv, f, d, band_block, res)
        cons = np.nan
    else:
        varl, pv = dense_reference(I, nv, f, d, rows)
        E = edge_reference(I, nv, f, d, res)
        i, j = I[:, 0] - f, I[:, 1] - f
        keep, w = j >= 0, d ** 2
        two = keep & (i >= 0)
        M = np.zeros((nv - f, nv - f))
        np.add.at(M, (j[keep], j[keep]), w[keep])
        np.add.at(M, (i[two], i[two]), w[two])
        np.add.at(M, (j[two], i[two]), -w[two])
        np.add.at(M, (i[two], j[two]), -w[two])
        cons = float(np.abs(M @ np.linalg.inv(M) - np.eye(nv - f)).max())
    pv = np.asarray(pv, dtype=np.float64).reshape(-1).copy()
    pv[np.array(absent, dtype=bool)] = np.nan
    var = nan(m)
    for x, r in v2i.items():
        var[x] = varl[r]            # 0 for the rows below f
    ang = np.array(ang)
    cv = pv[len(pairs):]
    with np.errstate(divide="ignore", invalid="ignore"):
        cchi = ang ** 2 / (E["scale"] * (cv + SIGMA ** 4))
    return dict(skipped=0, n_views=nv, n_edges=P["ne"], n_fixed=f, var=var, pair_var=pv[:len(pairs)], n=P["ne"],
                conn=P["conn"], edge_var=E["edge_var"], leverage=E["leverage"], chi2=E["chi2"], scale=E["scale"],
                angle=ang, cand_var=cv, cand_chi2=cchi, consistency=cons, problem=P, weights=d)


def make_pair(n, seed, fixed=(), k_prev=4, n_loops=6, noise=0.01, start=0.05, vg_opts=None):
    """The same stream in a ViewGraph and a ViewGraphOracle: build_sequence's connections, initial poses = ground truth
    perturbed by `start` rad, ground-truth fixes at `fixed`."""
    Qgt, relr = build_sequence(n, seed=seed, k_prev=k_prev, n_loops=n_loops, noise=noise)
    vg, vo = ViewGraph(**(vg_opts or {})), ViewGraphOracle()
    rng = np.random.default_rng(seed + 1000)
    for v in range(n):
        R0 = rot(synth.qmul(synth.qexp(rng.normal(scale=start, size=(1, 3)))[0], Qgt[v]))
        vg.addView(R0); vo.addView(R0)
    for (i, j), R in relr.items():
        assert vg.connect(i, j, R) == vo.connect(i, j, R)
    for idx in fixed:
        vg.fixPose(idx, rot(Qgt[idx])); vo.fixPose(idx, rot(Qgt[idx]))
    return vg, vo, Qgt


# the window cases of the GPU test: (views, seed, fixed views, window)
WINDOW_CASES = [(40, 7, (0,), 10), (40, 7, (0, 20, 35), 10), (40, 7, (), 10), (40, 8, (0, 33, 36), 10),
                (90, 9, (0,), 60), (90, 9, (), 64), (30, 5, (), 5000000), (30, 5, (3,), 5000000)]


# ---- properties of the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,fixed,win", WINDOW_CASES)
def test_reference_properties(n, seed, fixed, win):
    vg, vo, _ = make_pair(n, seed, fixed)
    pairs = [(n - 1, n - 2), (n - 1, 0), (n - 1, n - 1), (n - 3, max(n - win - 1, 0)), (0, 1)]
    r = viewgraph_uncertainty_reference(vo, win, pairs)
    P = r["problem"]
    nu = P["nv"] - P["f"]
    assert r["consistency"] < 1e-9                       # the reference is consistent on these inputs
    assert abs(r["leverage"].sum() - nu) <= 1e-9 * nu
    held = [x for x, row in P["v2i"].items() if row < P["f"]]
    free = [x for x, row in P["v2i"].items() if row >= P["f"]]
    absent = [x for x in range(n) if x not in P["v2i"]]
    assert np.all(r["var"][held] == 0) and np.all(r["var"][free] > 0) and np.all(np.isnan(r["var"][absent]))
    assert bool(absent) == (win < n), "a window leaves views out, a global problem none"
    gauge = len(fixed) == 0 and win >= n                  # no fixed pose in the problem: row 0 is held
    assert all(x < n - win or vo.fixed[x] or (gauge and P["v2i"][x] == 0) for x in held)
    assert r["pair_var"][2] == 0                          # i == j
    assert np.isnan(r["pair_var"][4]) == (win < n)        # views 0, 1 are not in a window at the end
    # the quirk rows: an edge whose second view is held has no row of A
    zero = P["I"][:, 1] < P["f"]
    assert np.all(r["edge_var"][zero] == 0)
    if gauge:                                             # the f == 0 rule: row 0 is held at the pose it has
        assert P["f"] == 1
        x0 = P["i2v"][0]
        np.testing.assert_array_equal(P["Q"][0], O.rmat2quat(vo.R[x0]))
        assert r["var"][x0] == 0


@pytest.mark.parametrize("seed,fixed", [(7, (0,)), (7, (0, 20, 35)), (8, (0, 33, 36))])
def test_window_conditions_on_held_views(seed, fixed):
    """Holding the views outside the window is conditioning: for a view inside, the window's Sigma entry cannot exceed
    the global one. Both references use their robust weights; those coincide edge by edge (same poses, same residuals),
    so the window's M is a principal submatrix of the global M and the inequality is exact up to rounding."""
    vg, vo, _ = make_pair(40, seed, fixed)
    w, g = viewgraph_uncertainty_reference(vo, 10), viewgraph_uncertainty_reference(vo, 5000000)
    inside = [x for x, row in w["problem"]["v2i"].items() if row >= w["problem"]["f"]]
    assert inside
    for x in inside:
        assert g["var"][x] > 0 and w["var"][x] <= g["var"][x] * (1 + 1e-9)


def test_skipped_problems_are_all_nan():
    vo = ViewGraphOracle()
    for _ in range(3):
        vo.addView()
    vo.connect(0, 1, np.eye(3))
    r = viewgraph_uncertainty_reference(vo, 10, [(0, 1)], [(0, 2, np.eye(3))])
    assert r["skipped"] == 2 and np.all(np.isnan(r["var"])) and np.isnan(r["pair_var"][0]) and np.isnan(r["cand_chi2"][0])


# ---- the planted-closure input of the GPU test ---------------------------------------------------------------------
GATE_N, GATE_SEED, GATE_TRUE, GATE_WRONG, GATE_ANGLE = 300, 21, 20, 5, 0.3
GATE_GAP = 10.0   # smallest wrong chi2 / largest true chi2 that the reference must show (it shows more, see the test)


def gate_input():
    """A noisy sequence (0.01 rad) at its ground-truth poses perturbed by 0.01 rad (a stand-in for a converged global
    solve that needs no GPU), GATE_TRUE far-apart candidate closures consistent with ground truth (same noise) and
    GATE_WRONG that are off by a rotation of >= GATE_ANGLE rad."""
    vg, vo, Qgt = make_pair(GATE_N, GATE_SEED, (0,), noise=0.01, start=0.01)
    rng = np.random.default_rng(GATE_SEED)
    cands = []
    for t in range(GATE_TRUE + GATE_WRONG):
        a = int(rng.integers(0, GATE_N - 60))
        b = int(a + rng.integers(50, GATE_N - a))
        ang = 0.01 * rng.normal(size=(1, 3))
        if t >= GATE_TRUE:
            ax = rng.normal(size=(1, 3))
            ang = ax * (GATE_ANGLE + 0.3 * rng.random()) / np.linalg.norm(ax)
        R = rot(synth.qmul(synth.qexp(ang)[0], synth.qmul(Qgt[b], synth.qconj(Qgt[a]))))
        cands.append((a, b, R) if t % 2 == 0 else (b, a, R.T))       # both orders, as connect takes them
    return vg, vo, cands


def test_gate_separates_planted_wrong_closures_in_the_reference():
    _, vo, cands = gate_input()
    r = viewgraph_uncertainty_reference(vo, 5000000, cands=cands)
    chi = r["cand_chi2"]
    assert np.all(np.isfinite(chi)) and np.all(r["angle"][GATE_TRUE:] >= GATE_ANGLE - 0.1)
    gap = chi[GATE_TRUE:].min() / chi[:GATE_TRUE].max()
    print("planted-closure gap of the reference: %.1f (true max %.2f, wrong min %.1f)" % (gap, chi[:GATE_TRUE].max(),
                                                                                         chi[GATE_TRUE:].min()))
    assert gap > GATE_GAP


# ---- ABI ----------------------------------------------------------------------------------------------------------
def test_header_declares_the_queries_and_binding_lists_them():
    src = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    for s, ret in (("irotavg_viewgraph_rotation_variance", "int"), ("irotavg_viewgraph_num_connections", "int64_t"),
                   ("irotavg_viewgraph_edge_diagnostics", "int64_t"), ("irotavg_viewgraph_gate_connections", "int"),
                   ("irotavg_graph_pose_weights", "int")):
        assert re.search(r"\b" + ret + r"\s+" + s + r"\s*\(", src), s
        assert s in capi.SYMBOLS
        assert hasattr(capi.lib(), s)
    body = re.search(r"typedef struct irotavg_uncertainty_info \{(.*?)\} irotavg_uncertainty_info;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, rest = decl.split(None, 1)
            names += [(n.strip(), ctype) for n in rest.split(",")]
    want = {"int": "c_int", "double": "c_double"}
    assert [(n, want[t]) for n, t in names] == [(n, t.__name__) for n, t in capi.UncertaintyInfo._fields_]
    for meth in ("rotationVariance", "numConnections", "edgeDiagnostics", "gateConnections"):
        assert callable(getattr(ViewGraph, meth))


def test_bad_arguments_and_skips_need_no_device():
    vg = ViewGraph()
    for _ in range(3):
        vg.addView()
    vg.connect(0, 1, np.eye(3))
    with pytest.raises(capi.IrotavgError):
        vg.rotationVariance(2)                                   # winSize > 2, as rotAvg
    assert vg.rotationVariance(10, pairs=[(0, 3)], allow_rc=(capi.ERR_BAD_ARG,))["rc"] == capi.ERR_BAD_ARG
    assert vg.gateConnections(10, [(1, 1)], [np.eye(3)], allow_rc=(capi.ERR_BAD_ARG,))["rc"] == capi.ERR_BAD_ARG
    assert vg.gateConnections(10, [(0, 7)], [np.eye(3)], allow_rc=(capi.ERR_BAD_ARG,))["rc"] == capi.ERR_BAD_ARG
    L = capi.lib()
    assert L.irotavg_viewgraph_rotation_variance(vg._h, 10, None, -1, None, None, None) == capi.ERR_BAD_ARG
    assert L.irotavg_viewgraph_gate_connections(vg._h, 10, -1, None, None, None, None, None, None) == capi.ERR_BAD_ARG
    # where rotAvg would skip (1 edge < winSize 3): OK, skipped set, every output NaN -- without a device
    r = vg.rotationVariance(10, pairs=[(0, 1)])
    assert r["rc"] == capi.OK and r["skipped"] == 2 and np.all(np.isnan(r["var"])) and np.isnan(r["pair_var"][0])
    assert vg.numConnections(10) == 0
    e = vg.edgeDiagnostics(10, cap=4)
    assert e["skipped"] == 2 and e["n"] == 0 and np.all(np.isnan(e["chi2"])) and np.all(e["conn"] == -1)
    g = vg.gateConnections(10, [(0, 2)], [np.eye(3)])
    assert g["skipped"] == 2 and np.isnan(g["angle"][0]) and np.isnan(g["chi2"][0]) and np.isnan(g["pair_var"][0])
    one = ViewGraph(); one.addView()
    assert one.rotationVariance(10)["skipped"] == 1
