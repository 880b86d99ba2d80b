"""Rotation-variance query on the device (irotavg_graph_rotation_variance, irotavg_amd/csrc/marginals.hip) against the
NumPy references of test_rotation_variance_cpu.py: dense path, banded direct-solver path with and without loop closures,
refusal on PCG handles, read-only and deterministic behaviour, the singular case and the one-shot call."""
import os

import numpy as np
import pytest

from irotavg_amd import capi, graphio, ral, synth
from oracle import oracle as O
from test_rotation_variance_cpu import band_reference, dense_reference, scale_reference

pytestmark = pytest.mark.gpu

SIGMA = 5 * np.pi / 180


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


def fixture_state(fixture_graph):
    g = fixture_graph
    f = g["f"]
    rc, Q0 = O.init_mst(g["Q"], g["QQ"], g["I"], max(g["n_abs_read"], f))
    assert rc == 0
    return g["I"], g["QQ"], g["n"], f, Q0


def solved_handle(I, QQ, n, f, Q0, l1=5, **opts):
    G = capi.Graph(I, QQ, n, f, **opts)
    G.set_rotations(Q0)
    if l1:
        G.l1ra(l1, 1e-3)
    G.irls(4, SIGMA, 50, 1e-3)
    return G


def pick_pairs(n, f, rng, I, k=50):
    """random pairs + a fixed view, i == j and edge endpoints"""
    P = rng.integers(0, n, size=(k - 6, 2))
    e = I[rng.integers(0, len(I), size=3)]
    P = np.concatenate([P, [[0, 0], [f, f], [0, n - 1]], e]).astype(np.int32)
    return P


def sequence(n, m, ncl=0, seed=1):
    S = synth.make_graph(n, m, 0.0, seed=seed)
    I, QQ = S["I"], S["QQ"]
    if ncl:
        rng = np.random.default_rng(seed + 100)
        a = rng.integers(0, n - 400, size=ncl)
        b = a + rng.integers(200, n - a)
        b = np.minimum(b, n - 1)
        I = np.concatenate([I, np.stack([a, b], 1)]).astype(np.int32)
        QQ = np.concatenate([QQ, synth.qmul(S["Qgt"][b], synth.qconj(S["Qgt"][a]))])
    return I.astype(np.int32), QQ, S["Qgt"]


def start_rotations(Qgt, QQ, I, f=1):
    Qs = np.zeros_like(Qgt)
    Qs[:, 3] = 1
    Qs[:f] = Qgt[:f]
    rc, Qs = O.init_mst(Qs, QQ, I, f)
    assert rc == 0
    return Qs


# ---- 1. dense path: the fixture through l1ra + irls ------------------------------------------------------------------
def test_dense_path_fixture(fixture_graph):
    I, QQ, n, f, Q0 = fixture_state(fixture_graph)
    with solved_handle(I, QQ, n, f, Q0) as G:
        P = pick_pairs(n, f, np.random.default_rng(0), I)
        # the seams of the sweep's 64 x 64 tiles: rows 64 k - 1 and 64 k, each pair across its own seam and one across
        # the whole matrix (entries of tiles next to and far off the diagonal)
        k = 64 * np.arange(1, (n - f + 63) // 64)
        P = np.concatenate([P, np.stack([f + k - 1, f + k], 1), np.stack([f + k, f + k[::-1] - 1], 1)]).astype(np.int32)
        r = G.rotation_variance(P)
        d = G.get_weights()
        G.edge_residual()
        res = G.get_residuals()
    var, pv = dense_reference(I, n, f, d, [tuple(p) for p in P])
    assert np.all(r["var"][:f] == 0) and rel(r["var"][f:], var[f:]) < 1e-9
    nz = pv != 0
    assert rel(r["pair_var"][nz], pv[nz]) < 1e-9 and np.all(r["pair_var"][~nz] == 0)
    assert r["scale"] == pytest.approx(scale_reference(I, f, d, res, n - f), rel=1e-9)


# ---- 2. band path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,deg,seed", [(2600, 6, 1), (2600, 24, 2), (20000, 30, 3), (20000, 8, 4)])
def test_band_path_random_weights(n, deg, seed):
    I, QQ, Qgt = sequence(n, deg * n - deg * (deg + 1) // 2, seed=seed)
    rng = np.random.default_rng(seed)
    with capi.Graph(I, QQ, n, 1) as G:
        B = G.stats()["band_block"]
        assert B > 0
        G.set_rotations(Qgt)
        d = rng.uniform(0.1, 3.0, size=len(I))
        G.set_weights(d)
        P = pick_pairs(n, 1, rng, I)
        r = G.rotation_variance(P)
    var, pv, _ = band_reference(I, n, 1, d, B, [tuple(p) for p in P])
    assert rel(r["var"][1:], var[1:]) < 1e-9 and r["var"][0] == 0
    nz = pv != 0
    assert rel(r["pair_var"][nz], pv[nz]) < 1e-9


def test_band_path_after_irls_full_size():
    n = 100000
    I, QQ, Qgt = sequence(n, 2000000, seed=5)
    with capi.Graph(I, QQ, n, 1) as G:
        B = G.stats()["band_block"]
        assert B > 0
        G.set_rotations(start_rotations(Qgt, QQ, I))
        G.irls(4, SIGMA, 50, 1e-3)
        d = G.get_weights()
        P = pick_pairs(n, 1, np.random.default_rng(5), I)
        r = G.rotation_variance(P)
    var, pv, _ = band_reference(I, n, 1, d, B, [tuple(p) for p in P])
    assert rel(r["var"][1:], var[1:]) < 1e-9
    nz = pv != 0
    assert rel(r["pair_var"][nz], pv[nz]) < 1e-9
    assert np.isfinite(r["scale"]) and r["scale"] > 0


# ---- 3. closures ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncl", [1, 30, 100, 1000])
def test_closures_against_dense_inverse(ncl):
    n = 3000
    I, QQ, Qgt = sequence(n, 12 * n - 78, ncl=ncl, seed=ncl)
    with capi.Graph(I, QQ, n, 1) as G:
        st = G.stats()
        assert st["band_block"] > 0 and G.direct_info()["closures"] == ncl
        G.set_rotations(start_rotations(Qgt, QQ, I))
        G.irls(4, SIGMA, 50, 1e-3)
        d = G.get_weights()
        P = pick_pairs(n, 1, np.random.default_rng(ncl), I)
        r = G.rotation_variance(P)
    var, pv = dense_reference(I, n, 1, d, [tuple(p) for p in P])
    assert rel(r["var"][1:], var[1:]) < 1e-9
    nz = pv != 0
    assert rel(r["pair_var"][nz], pv[nz]) < 1e-9
    _, _, band = band_reference(I, n, 1, d, st["band_block"])
    assert np.all(r["var"][1:] <= band[1:] * (1 + 1e-12))


@pytest.mark.parametrize("n,ncl", [(8400, 2048), (100000, 30), (100000, 100)])
def test_closures_against_block_reference(n, ncl):
    I, QQ, Qgt = sequence(n, 20 * n - 210, ncl=ncl, seed=7)
    with capi.Graph(I, QQ, n, 1) as G:
        B = G.stats()["band_block"]
        assert B > 0 and G.direct_info()["closures"] == ncl
        G.set_rotations(Qgt)
        d = np.random.default_rng(ncl).uniform(0.1, 3.0, size=len(I))
        G.set_weights(d)
        P = pick_pairs(n, 1, np.random.default_rng(ncl), I)
        r = G.rotation_variance(P)
    var, pv, band = band_reference(I, n, 1, d, B, [tuple(p) for p in P])
    assert rel(r["var"][1:], var[1:]) < 1e-9
    nz = pv != 0
    assert rel(r["pair_var"][nz], pv[nz]) < 1e-9
    assert np.all(r["var"][1:] <= band[1:] * (1 + 1e-12))


# ---- 4. PCG handles: pairs through the handle's own solver; marginals refused, nothing written -------------------
def pcg_graph():
    n = 5000
    S = synth.make_graph(n, 20 * n, 0.02, seed=11)
    return S["I"].astype(np.int32), S["QQ"], S["Qgt"], n


def test_pcg_pairs_against_dense_inverse():
    I, QQ, Qgt, n = pcg_graph()
    with capi.Graph(I, QQ, n, 1, band_direct=-1) as G:
        assert G.stats()["band_block"] == 0
        G.set_rotations(start_rotations(Qgt, QQ, I))
        G.irls(4, SIGMA, 50, 1e-3)
        assert G.stats()["pcg_solves"] > 0
        d = G.get_weights()
        P = pick_pairs(n, 1, np.random.default_rng(12), I)
        r = G.rotation_variance(P, marginals=False)
        assert r["var"] is None and np.isfinite(r["scale"])
        r2 = G.rotation_variance(P[:7], marginals=False)   # a short last group of three
        np.testing.assert_array_equal(r2["pair_var"], r["pair_var"][:7])
        rv = G.rotation_variance(P, allow_rc=(capi.ERR_UNSUPPORTED,))
        assert rv["rc"] == capi.ERR_UNSUPPORTED
        assert np.isnan(rv["var"]).all() and np.isnan(rv["pair_var"]).all() and np.isnan(rv["scale"])
    _, pv = dense_reference(I, n, 1, d, [tuple(p) for p in P])
    nz = pv != 0
    assert rel(r["pair_var"][nz], pv[nz]) < 1e-6 and np.all(r["pair_var"][~nz] == 0)


# ---- 5. read-only, 6. deterministic -------------------------------------------------------------------------------
def _stats_wo_time(G):
    s = G.stats()
    return {k: v for k, v in s.items() if not k.startswith("seconds")}


def _cases():
    return ["dense", "band", "closures", "pcg"]


def _build(case):
    if case == "dense":
        g = graphio.read_ravg_input(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ravg_input.txt"))
        f = g["f"]
        rc, Q0 = O.init_mst(g["Q"], g["QQ"], g["I"], max(g["n_abs_read"], f))
        return g["I"], g["QQ"], g["n"], f, Q0, {}
    if case == "pcg":
        I, QQ, Qgt, n = pcg_graph()
        return I, QQ, n, 1, start_rotations(Qgt, QQ, I), dict(band_direct=-1)
    I, QQ, Qgt = sequence(3000, 12 * 3000 - 78, ncl=(40 if case == "closures" else 0), seed=21)
    return I, QQ, 3000, 1, start_rotations(Qgt, QQ, I), {}


@pytest.mark.parametrize("case", _cases())
def test_query_is_read_only_and_deterministic(case):
    I, QQ, n, f, Q0, opts = _build(case)
    with solved_handle(I, QQ, n, f, Q0, l1=2, **opts) as A, solved_handle(I, QQ, n, f, Q0, l1=2, **opts) as Bt:
        Qa, wa, sa = A.get_rotations(), A.get_weights(), _stats_wo_time(A)
        A.edge_residual()
        ra = A.get_residuals()
        Bt.edge_residual()
        P = pick_pairs(n, f, np.random.default_rng(3), I)
        marg = case != "pcg"   # a PCG handle answers pairs only
        r1 = A.rotation_variance(P, marginals=marg)
        r2 = A.rotation_variance(P, marginals=marg)
        for k in ("var", "pair_var") if marg else ("pair_var",):
            np.testing.assert_array_equal(r1[k], r2[k])
        assert r1["scale"] == r2["scale"] or (np.isnan(r1["scale"]) and np.isnan(r2["scale"]))
        np.testing.assert_array_equal(A.get_rotations(), Qa)
        np.testing.assert_array_equal(A.get_weights(), wa)
        np.testing.assert_array_equal(A.get_residuals(), ra)
        assert _stats_wo_time(A) == sa
        # a following irls (from perturbed rotations, so that it iterates) is bitwise the twin's
        Qp = synth.qmul(synth.qexp(np.random.default_rng(4).normal(scale=0.01, size=(n, 3))), Qa)
        Qp[:f] = Qa[:f]
        outs = []
        for G in (A, Bt):
            G.set_rotations(Qp)
            o = G.irls(4, SIGMA, 50, 1e-3)
            outs.append((G.get_rotations(), G.get_weights(), o["iters"], o["scores"]))
        np.testing.assert_array_equal(outs[0][0], outs[1][0])
        np.testing.assert_array_equal(outs[0][1], outs[1][1])
        assert outs[0][2] == outs[1][2]
        np.testing.assert_array_equal(outs[0][3], outs[1][3])


# ---- 7. singular operator -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dense", "band", "closures"])
def test_singular_view_is_an_error(case):
    I, QQ, n, f, Q0, opts = _build(case)
    with capi.Graph(I, QQ, n, f, **opts) as G:
        G.set_rotations(Q0)
        v = f + (n - f) // 2
        d = np.ones(len(I))
        d[(I[:, 0] == v) | (I[:, 1] == v)] = 0.0
        G.set_weights(d)
        r = G.rotation_variance([[v, f]], allow_rc=(capi.ERR_SOLVER,))
        assert r["rc"] == capi.ERR_SOLVER
        assert np.isnan(r["var"]).all() and np.isnan(r["pair_var"]).all() and np.isnan(r["scale"])


def test_dense_weakly_tied_view_is_regular():
    # the dead-pivot rule is relative to the row's own diagonal: a view tied only by tiny weights is still regular
    I, QQ, n, f, Q0, _ = _build("dense")
    v = f + (n - f) // 2
    d = np.ones(len(I))
    d[(I[:, 0] == v) | (I[:, 1] == v)] = 1e-7
    with capi.Graph(I, QQ, n, f) as G:
        G.set_rotations(Q0)
        G.set_weights(d)
        r = G.rotation_variance()
    var, _ = dense_reference(I, n, f, d)
    assert rel(r["var"][f:], var[f:]) < 1e-6 and r["var"][v] > 1e12


# ---- 8. one-shot ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dense", "closures"])
def test_oneshot_equals_handle(case):
    I, QQ, n, f, Q0, _ = _build(case)
    capi.oneshot_cache(True)
    capi.oneshot_cache_clear()
    Q = Q0.copy()
    w = np.zeros(len(I))
    ral.l1ra(QQ, I, None, Q, f, 2, 1e-3)
    ral.irls(QQ, I, None, 4, SIGMA, Q, f, 50, 1e-3, w)
    h0, _ = capi.oneshot_cache_stats()
    P = pick_pairs(n, f, np.random.default_rng(8), I)
    r = capi.rotation_variance(I, QQ, Q, w, f, P)
    h1, _ = capi.oneshot_cache_stats()
    assert h1 == h0 + 1
    with capi.Graph(I, QQ, n, f) as G:
        G.set_rotations(Q)
        G.set_weights(w)
        rh = G.rotation_variance(P)
    np.testing.assert_array_equal(r["var"], rh["var"])
    np.testing.assert_array_equal(r["pair_var"], rh["pair_var"])
    assert r["scale"] == rh["scale"]
