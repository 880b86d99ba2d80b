"""View-graph uncertainty queries on the device (docs/viewgraph_uncertainty.md) against the NumPy reference of
test_viewgraph_uncertainty_cpu.py: the single-kernel window route (irotavg_amd/csrc/wincov.hip), the handle routes
(dense, band with closures, PCG), irotavg_graph_pose_weights, read-only and deterministic behaviour, the planted wrong
closures and the errors. Tolerance: relative 1e-9 where finite, NaN / inf / 0 positions exact (the figure of the two
handle-query test files)."""
import os

import numpy as np
import pytest

from irotavg_amd import capi, synth
from irotavg_amd.viewgraph import ViewGraph
from oracle import np_twin as T
from oracle import oracle as O
from oracle.viewgraph_oracle import ViewGraphOracle
from test_gpu_rotation_variance import pcg_graph, sequence
from test_viewgraph import rot
from test_viewgraph_uncertainty_cpu import (GATE_TRUE, SIGMA, WINDOW_CASES, gate_input, make_pair,
                                            viewgraph_uncertainty_reference)

pytestmark = pytest.mark.gpu
BIG = 5000000


def assert_same(got, ref, what, rtol=1e-9):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    for cls in (np.isnan, np.isposinf, lambda x: x == 0):
        np.testing.assert_array_equal(cls(got), cls(ref), err_msg=what)
    fin = np.isfinite(ref) & (ref != 0)
    err = np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])
    worst = float(err.max()) if err.size else 0.0
    print("%s: max relative error over %d entries: %.3e" % (what, int(fin.sum()), worst))
    assert worst < rtol, what


def query_all(vg, win, pairs, cands):
    v = vg.rotationVariance(win, pairs)
    e = vg.edgeDiagnostics(win)
    g = vg.gateConnections(win, [c[:2] for c in cands], [c[2] for c in cands])
    return v, e, g


def check_against_reference(vg, ref, win, pairs, cands, route):
    v, e, g = query_all(vg, win, pairs, cands)
    for r in (v, e, g):
        assert r["skipped"] == 0 and r["route"] == route
        assert (r["n_views"], r["n_edges"], r["n_fixed"]) == (ref["n_views"], ref["n_edges"], ref["n_fixed"])
        assert r["scale"] == pytest.approx(ref["scale"], rel=1e-9, nan_ok=True)
    assert_same(v["var"], ref["var"], "var")
    assert_same(v["pair_var"], ref["pair_var"], "pair_var")
    assert e["n"] == ref["n"] == vg.numConnections(win)
    np.testing.assert_array_equal(e["conn"], ref["conn"])
    for k in ("edge_var", "leverage", "chi2"):
        assert_same(e[k], ref[k], k)
    nu = ref["n_views"] - ref["n_fixed"]
    assert abs(e["leverage"].sum() - nu) <= 1e-9 * nu
    assert_same(g["angle"], ref["angle"], "angle")
    assert_same(g["pair_var"], ref["cand_var"], "candidate pair_var")
    assert_same(g["chi2"], ref["cand_chi2"], "candidate chi2")
    # two identical queries: bitwise equal
    v2, e2, g2 = query_all(vg, win, pairs, cands)
    for a, b in ((v, v2), (e, e2), (g, g2)):
        for k in a:
            if isinstance(a[k], np.ndarray):
                np.testing.assert_array_equal(a[k], b[k])
    return v, e, g


def some_candidates(n, rng, k=6):
    out = []
    for t in range(k):
        a, b = rng.choice(n, size=2, replace=False)
        R = rot(synth.qexp(rng.normal(scale=0.2, size=(1, 3)))[0])
        out.append((int(a), int(b), R))
    return out


# ---- 1. the window route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed,fixed,win", WINDOW_CASES)
def test_window_route_against_reference(n, seed, fixed, win):
    vg, vo, _ = make_pair(n, seed, fixed)
    rng = np.random.default_rng(seed)
    pairs = [(n - 1, n - 2), (n - 1, 0), (n - 1, n - 1), (n - 3, max(n - win - 1, 0)), (0, 1), (n - 2, n - 5)]
    cands = some_candidates(n, rng) + [(n - 1, n - 4, np.eye(3)), (n - 2, n - 1, vo.conn[n - 1][n - 2])]
    ref = viewgraph_uncertainty_reference(vo, win, pairs, cands)
    assert ref["consistency"] < 1e-9
    check_against_reference(vg, ref, win, pairs, cands, route=1)
    poses = [vg.R(v) for v in range(n)]
    for v in range(n):                                            # nothing moved
        np.testing.assert_array_equal(poses[v], vo.R[v])


def test_window_route_more_pairs_and_candidates_than_one_launch_stages():
    vg, vo, _ = make_pair(40, 7, (0,))
    rng = np.random.default_rng(3)
    pairs = [tuple(int(x) for x in rng.integers(25, 40, size=2)) for _ in range(2500)]
    cands = some_candidates(40, rng, k=600)
    ref = viewgraph_uncertainty_reference(vo, 10, pairs, cands)
    v = vg.rotationVariance(10, pairs)
    g = vg.gateConnections(10, [c[:2] for c in cands], [c[2] for c in cands])
    assert_same(v["pair_var"], ref["pair_var"], "pair_var")
    assert_same(g["chi2"], ref["cand_chi2"], "candidate chi2")
    assert_same(g["angle"], ref["angle"], "angle")


# ---- 2. the handle routes ------------------------------------------------------------------------------------------------
def test_dense_route_against_reference():
    n = 300
    vg, vo, _ = make_pair(n, 12, (0, 150))
    rng = np.random.default_rng(12)
    pairs = [tuple(int(x) for x in rng.integers(0, n, size=2)) for _ in range(20)] + [(0, 150), (7, 7)]
    cands = some_candidates(n, rng)
    ref = viewgraph_uncertainty_reference(vo, BIG, pairs, cands)
    assert ref["consistency"] < 1e-9
    check_against_reference(vg, ref, BIG, pairs, cands, route=2)


def from_arrays(I, QQ, Q0, fixed=(0,), oracle=True, **opts):
    vg, vo = ViewGraph(**opts), (ViewGraphOracle() if oracle else None)
    for v in range(len(Q0)):
        R = rot(Q0[v])
        vg.addView(R)
        if vo:
            vo.addView(R)
    for (i, j), q in zip(I, QQ):
        R = rot(q)
        vg.connect(int(i), int(j), R)
        if vo:
            vo.connect(int(i), int(j), R)
    for x in fixed:
        vg.fixPose(x, rot(Q0[x]))
        if vo:
            vo.fixPose(x, rot(Q0[x]))
    return vg, vo


def perturbed(Qgt, seed, scale=0.02):
    rng = np.random.default_rng(seed)
    return synth.qmul(synth.qexp(rng.normal(scale=scale, size=(len(Qgt), 3))), Qgt)


@pytest.mark.parametrize("ncl", [0, 5, 100])
def test_band_route_against_block_reference(ncl):
    n = 3000
    I, QQ, Qgt = sequence(n, 6 * n - 21, ncl, seed=3)
    vg, vo = from_arrays(I, QQ, perturbed(Qgt, 4))
    rng = np.random.default_rng(ncl)
    pairs = [tuple(int(x) for x in rng.integers(0, n, size=2)) for _ in range(20)] + [(0, 0), (0, n - 1)]
    cands = some_candidates(n, rng)
    ref = viewgraph_uncertainty_reference(vo, BIG, pairs, cands, band_block=24)
    v, e, g = check_against_reference(vg, ref, BIG, pairs, cands, route=3)
    assert (v["closures"] > 0) == (ncl > 0)


def test_large_band_problem_resident_and_rebuilt_agree_with_the_handle_queries(capfd):
    """>= 20 000 connections: the handle of the global problem is built on the device from the resident records
    (IROTAVG_NO_RESIDENT unset) or from a host extraction (= 1). The two answers must be bitwise equal to each other, and
    equal to a handle built from the same (I, QQ, Q) with irotavg_graph_pose_weights and the handle queries. That the
    two runs really take different paths is read off the phase lines IROTAVG_ROTAVG_TIMING=1 makes the resident path
    print; a second query on the resident graph must find nothing left to send."""
    n = 4000
    I, QQ, Qgt = sequence(n, 6 * n - 21, 10, seed=6)
    Q0 = perturbed(Qgt, 7)
    rng = np.random.default_rng(8)
    pairs = [tuple(int(x) for x in rng.integers(0, n, size=2)) for _ in range(20)]
    got = []
    keep = {k: os.environ.pop(k, None) for k in ("IROTAVG_NO_RESIDENT", "IROTAVG_ROTAVG_TIMING")}
    try:
        os.environ["IROTAVG_ROTAVG_TIMING"] = "1"
        for no_res in (None, "1"):
            if no_res:
                os.environ["IROTAVG_NO_RESIDENT"] = no_res
            vg, vo = from_arrays(I, QQ, Q0, oracle=(no_res is None))
            if vo:
                ref_vo = vo
            assert vg.numConnections(BIG) >= 20000
            capfd.readouterr()
            v = vg.rotationVariance(BIG, pairs)
            err1 = capfd.readouterr().err
            e = vg.edgeDiagnostics(BIG)
            err2 = capfd.readouterr().err
            got.append((v, e))
            if no_res:
                assert "delta packing" not in err1 + err2
            else:
                assert "delta packing" in err1 and "(%d views, %d edges sent)" % (n, vg.numConnections(BIG)) in err1
                assert "(0 views, 0 edges sent)" in err2
    finally:
        for k, val in keep.items():
            os.environ.pop(k, None)
            if val is not None:
                os.environ[k] = val
    (v0, e0), (v1, e1) = got
    for a, b in ((v0, v1), (e0, e1)):
        for k in a:
            if isinstance(a[k], np.ndarray):
                np.testing.assert_array_equal(a[k], b[k])
    from test_viewgraph_uncertainty_cpu import extract_problem
    P = extract_problem(ref_vo, BIG)
    with capi.Graph(P["I"], P["QQ"], P["nv"], P["f"]) as G:
        G.set_rotations(P["Q"])
        G.pose_weights(4, SIGMA)
        rows = [(P["v2i"][a], P["v2i"][b]) for a, b in pairs]
        hv = G.rotation_variance(rows)
        he = G.edge_diagnostics()
    var = np.array([hv["var"][P["v2i"][x]] for x in range(n)])
    np.testing.assert_array_equal(v0["var"], var)
    np.testing.assert_array_equal(v0["pair_var"], hv["pair_var"])
    assert v0["scale"] == hv["scale"] and v0["route"] == 3 and v0["closures"] > 0
    for k in ("edge_var", "leverage", "chi2"):
        np.testing.assert_array_equal(e0[k], he[k])


def test_pcg_route_serves_pairs_and_the_gate_only():
    I, QQ, Qgt, n = pcg_graph()
    Q0 = perturbed(Qgt, 13)
    vg, vo = from_arrays(I, QQ, Q0, band_direct=-1)
    rng = np.random.default_rng(14)
    pairs = [tuple(int(x) for x in rng.integers(0, n, size=2)) for _ in range(7)]
    cands = some_candidates(n, rng, k=4)
    r = vg.rotationVariance(BIG, pairs, allow_rc=(capi.ERR_UNSUPPORTED,))
    assert r["rc"] == capi.ERR_UNSUPPORTED and r["route"] == 4 and np.all(r["var"] == -1.0)      # outputs untouched
    e = vg.edgeDiagnostics(BIG, allow_rc=(capi.ERR_UNSUPPORTED,))
    assert e["rc"] == capi.ERR_UNSUPPORTED
    ref = viewgraph_uncertainty_reference(vo, BIG, pairs, cands)
    v = vg.rotationVariance(BIG, pairs, marginals=False)
    g = vg.gateConnections(BIG, [c[:2] for c in cands], [c[2] for c in cands])
    assert v["route"] == g["route"] == 4
    # the handle test's tolerance for PCG pairs (solves to pcg_rtol)
    np.testing.assert_allclose(v["pair_var"], ref["pair_var"], rtol=1e-6)
    np.testing.assert_allclose(g["pair_var"], ref["cand_var"], rtol=1e-6)
    np.testing.assert_allclose(g["chi2"], ref["cand_chi2"], rtol=1e-6)
    assert_same(g["angle"], ref["angle"], "angle")


# ---- 3. irotavg_graph_pose_weights -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", range(14))
def test_pose_weights_every_cost(cost):
    S = synth.make_graph(3000, 36000, 0.05, seed=2)
    I, QQ = S["I"], S["QQ"]
    Q = perturbed(S["Qgt"], 5, 0.05)
    m = len(I)
    with capi.Graph(I, QQ, 3000, 1) as G:
        G.set_rotations(Q)
        G.edge_residual()
        r1 = G.get_residuals()
        prev = np.random.default_rng(1).uniform(0.5, 2, size=m)
        G.set_weights(prev)
        G.set_rotations(Q)
        G.pose_weights(cost, SIGMA)
        w = G.get_weights()
        r2 = G.get_residuals()
    np.testing.assert_array_equal(r1, r2)                          # K1's planes, bit for bit
    ro = O.log_map(O.delta_rel(I, QQ, Q))[:, :3]
    wo = T.weights_update(cost, SIGMA, -ro, prev)                  # a zero step: E = A 0 - r
    np.testing.assert_allclose(w, wo, rtol=1e-11, atol=1e-300)     # test_gpu_parity.py::test_weight_update_every_cost's


# ---- 4. read-only ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_resident", [False, True])
def test_queries_leave_every_later_result_bitwise_unchanged(no_resident):
    n = 4000
    I, QQ, Qgt = sequence(n, 6 * n - 21, 10, seed=9)
    Q0 = perturbed(Qgt, 10)
    keep = os.environ.pop("IROTAVG_NO_RESIDENT", None)
    try:
        if no_resident:
            os.environ["IROTAVG_NO_RESIDENT"] = "1"
        a, _ = from_arrays(I, QQ, Q0, oracle=False)
        b, _ = from_arrays(I, QQ, Q0, oracle=False)
    finally:
        os.environ.pop("IROTAVG_NO_RESIDENT", None)
        if keep is not None:
            os.environ["IROTAVG_NO_RESIDENT"] = keep
    R = rot(Qgt[n - 1]) @ rot(Qgt[5]).T
    for vg, ask in ((a, True), (b, False)):
        assert vg.rotAvg(BIG)["skipped"] == 0
        if ask:
            vg.rotationVariance(BIG, [(5, n - 1)])
            vg.edgeDiagnostics(BIG)
            vg.gateConnections(BIG, [(5, n - 1)], [R])
            vg.rotationVariance(10, [(n - 1, n - 2)])
            vg.edgeDiagnostics(10)
        vg.connect(5, n - 1, R)
        assert vg.rotAvg(BIG)["skipped"] == 0
        if ask:
            vg.gateConnections(10, [(n - 3, n - 1)], [np.eye(3)])
        assert vg.rotAvg(10)["skipped"] == 0
    for v in range(n):
        np.testing.assert_array_equal(a.R(v), b.R(v))


# ---- 5. the gate ---------------------------------------------------------------------------------------------------------
def test_gate_ranks_planted_wrong_closures_above_every_true_one():
    vg, vo, cands = gate_input()
    assert vg.rotAvg(BIG)["skipped"] == 0                          # globally solved
    g = vg.gateConnections(BIG, [c[:2] for c in cands], [c[2] for c in cands])
    chi = g["chi2"]
    print("true max %.3f, wrong min %.3f" % (chi[:GATE_TRUE].max(), chi[GATE_TRUE:].min()))
    assert np.all(np.isfinite(chi))
    assert chi[GATE_TRUE:].min() > chi[:GATE_TRUE].max()
    assert vg.numConnections(BIG) == len([1 for j in range(len(vo.R)) for i in vo.conn[j] if i < j])   # nothing added


# ---- 6. errors -------------------------------------------------------------------------------------------------------------
def test_cap_too_small_is_refused():
    vg, vo, _ = make_pair(40, 7, (0,))
    n = vg.numConnections(10)
    assert n > 1
    assert vg.edgeDiagnostics(10, cap=n - 1, allow_rc=(capi.ERR_BAD_ARG,))["rc"] == capi.ERR_BAD_ARG
    assert vg.edgeDiagnostics(10, cap=n + 3)["n"] == n


@pytest.mark.parametrize("n_half", [10, 60])
def test_singular_problem_is_reported_and_outputs_stay_untouched(n_half):
    """Two components, the second without a fixed view: M is singular (window route at 20 views, dense route at 120)."""
    vg = ViewGraph()
    for _ in range(2 * n_half):
        vg.addView()
    for base in (0, n_half):
        for j in range(1, n_half):
            vg.connect(base + j - 1, base + j, np.eye(3))
            if j >= 2:
                vg.connect(base + j - 2, base + j, np.eye(3))
    vg.fixPose(0, np.eye(3))
    v = vg.rotationVariance(BIG, [(1, 2)], allow_rc=(capi.ERR_SOLVER,))
    assert v["rc"] == capi.ERR_SOLVER and v["route"] == (1 if n_half == 10 else 2)
    assert np.all(v["var"] == -1.0) and v["pair_var"][0] == -1.0
    e = vg.edgeDiagnostics(BIG, allow_rc=(capi.ERR_SOLVER,))
    assert e["rc"] == capi.ERR_SOLVER and np.all(e["chi2"] == -1.0) and np.all(e["conn"] == -7)
    g = vg.gateConnections(BIG, [(1, n_half + 1)], [np.eye(3)], allow_rc=(capi.ERR_SOLVER,))
    assert g["rc"] == capi.ERR_SOLVER and g["chi2"][0] == -1.0
