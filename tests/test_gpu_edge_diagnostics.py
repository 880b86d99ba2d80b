"""Edge diagnostics on the device (irotavg_graph_edge_diagnostics, irotavg_amd/csrc/edgediag.hip) against the NumPy
references of test_edge_diagnostics_cpu.py, over ALL edges: dense route, band route with and without loop closures, full
size against the variance query's pairs, errors, read-only and deterministic behaviour, the one-shot call and the
planted-outlier ranking. Tolerance: relative 1e-9, the figure of the rotation-variance tests."""
import numpy as np
import pytest

from irotavg_amd import capi, ral, synth
from test_edge_diagnostics_cpu import (OUTLIER_GAP, OUTLIER_K, band_edge_reference, edge_reference, outlier_graph,
                                       quirk_graph)
from test_gpu_rotation_variance import (SIGMA, _build, _stats_wo_time, fixture_state, pcg_graph, sequence,
                                        solved_handle, start_rotations)

pytestmark = pytest.mark.gpu

KEYS = ("edge_var", "leverage", "chi2")


def assert_same(got, ref, rtol=1e-9):
    """All m entries: equal class where the definition gives 0 / inf / NaN, relative rtol elsewhere."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    for cls in (np.isnan, np.isposinf, lambda x: x == 0):
        np.testing.assert_array_equal(cls(got), cls(ref))
    fin = np.isfinite(ref) & (ref != 0)
    err = np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])
    worst = float(err.max()) if err.size else 0.0
    print("max relative error over %d entries: %.3e" % (int(fin.sum()), worst))
    assert worst < rtol


def check_all(r, ref, nu):
    for k in KEYS:
        assert_same(r[k], ref[k])
    assert r["scale"] == pytest.approx(ref["scale"], rel=1e-9, nan_ok=True)
    lev = r["leverage"]
    assert abs(lev.sum() - nu) <= 1e-9 * nu
    assert lev.min() >= 0 and lev.max() <= 1 + 1e-9


def state_of(G):
    d = G.get_weights()
    G.edge_residual()
    return d, G.get_residuals()


# ---- 1. dense route --------------------------------------------------------------------------------------------------
def test_dense_route_fixture(fixture_graph):
    I, QQ, n, f, Q0 = fixture_state(fixture_graph)
    with solved_handle(I, QQ, n, f, Q0) as G:
        r = G.edge_diagnostics()
        d, res = state_of(G)
    check_all(r, edge_reference(I, n, f, d, res), n - f)


def test_dense_route_three_fixed_views_and_the_edge_drop_quirk():
    I, d, n, f = quirk_graph(3, n=300)
    rng = np.random.default_rng(3)
    Q = synth.qexp(rng.normal(scale=0.3, size=(n, 3)))
    QQ = synth.qmul(synth.qmul(synth.qexp(rng.normal(scale=0.02, size=(len(I), 3))), Q[I[:, 1]]), synth.qconj(Q[I[:, 0]]))
    with capi.Graph(I, QQ, n, f) as G:
        G.set_rotations(Q)
        G.set_weights(d)
        r = G.edge_diagnostics()
        _, res = state_of(G)
    ref = edge_reference(I, n, f, d, res)
    zero = I[:, 1] < f
    assert zero.any() and np.all(r["edge_var"][zero] == 0) and np.all(r["leverage"][zero] == 0)
    check_all(r, ref, n - f)


# ---- 2. band route without closures ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,deg,seed", [(2600, 6, 1), (2600, 24, 2), (20000, 30, 3), (20000, 8, 4)])
def test_band_route_random_weights(n, deg, seed):
    I, QQ, Qgt = sequence(n, deg * n - deg * (deg + 1) // 2, seed=seed)
    rng = np.random.default_rng(seed)
    with capi.Graph(I, QQ, n, 1) as G:
        B = G.stats()["band_block"]
        assert B > 0
        G.set_rotations(Qgt)
        d = rng.uniform(0.1, 3.0, size=len(I))
        G.set_weights(d)
        r = G.edge_diagnostics()
        _, res = state_of(G)
    ref = edge_reference(I, n, 1, d, res) if n <= 3000 else band_edge_reference(I, n, 1, d, B, res)
    check_all(r, ref, n - 1)


# ---- 3. band route with closures ---------------------------------------------------------------------------------------
def closure_case(n, deg, ncl, seed, irls):
    I, QQ, Qgt = sequence(n, deg * n - deg * (deg + 1) // 2, ncl=ncl, seed=seed)
    with capi.Graph(I, QQ, n, 1) as G:
        B = G.stats()["band_block"]
        assert B > 0 and G.direct_info()["closures"] == ncl
        if irls:
            G.set_rotations(start_rotations(Qgt, QQ, I))
            G.irls(4, SIGMA, 50, 1e-3)
            d = G.get_weights()
        else:
            G.set_rotations(Qgt)
            d = np.random.default_rng(ncl).uniform(0.1, 3.0, size=len(I))
        d[len(I) - ncl:len(I) - ncl + max(1, ncl // 10)] = 0.0   # closure edges of weight zero among them
        G.set_weights(d)
        r = G.edge_diagnostics()
        _, res = state_of(G)
    return I, d, res, B, r


@pytest.mark.parametrize("ncl", [5, 100, 1000])
def test_closures_against_dense_inverse(ncl):
    n = 3000
    I, d, res, B, r = closure_case(n, 12, ncl, ncl, True)
    check_all(r, edge_reference(I, n, 1, d, res), n - 1)


def test_2048_closures_against_block_reference():
    n = 8400
    I, d, res, B, r = closure_case(n, 20, 2048, 7, False)
    check_all(r, band_edge_reference(I, n, 1, d, B, res), n - 1)


# ---- 4. full size: the trace, the range, and the variance query's pairs --------------------------------------------------
@pytest.mark.parametrize("ncl", [0, 100])
def test_full_size_after_irls(ncl):
    n = 100000
    I, QQ, Qgt = sequence(n, 2000000, ncl=ncl, seed=5)
    rng = np.random.default_rng(5)
    with capi.Graph(I, QQ, n, 1) as G:
        assert G.stats()["band_block"] > 0 and G.direct_info()["closures"] == ncl
        G.set_rotations(start_rotations(Qgt, QQ, I))
        G.irls(4, SIGMA, 50, 1e-3)
        r = G.edge_diagnostics()
        pick = np.concatenate([rng.choice(len(I) - ncl, 2000, replace=False), np.arange(len(I) - ncl, len(I))])
        pv = G.rotation_variance(I[pick], marginals=False)["pair_var"]
    nu = n - 1
    lev = r["leverage"]
    print("sum leverage - nu = %.3e (nu = %d), leverage in [%.3e, 1 + %.3e]" % (lev.sum() - nu, nu, lev.min(),
                                                                                 lev.max() - 1))
    assert abs(lev.sum() - nu) <= 1e-9 * nu
    assert lev.min() >= 0 and lev.max() <= 1 + 1e-9
    assert np.all(I[pick, 1] >= 1) and np.all(I[pick, 0] != I[pick, 1])
    assert_same(r["edge_var"][pick], pv)


# ---- 5. errors ---------------------------------------------------------------------------------------------------------
def untouched(r):
    return all(np.isnan(r[k]).all() for k in KEYS) and np.isnan(r["scale"])


def test_pcg_handle_is_unsupported():
    I, QQ, Qgt, n = pcg_graph()
    with capi.Graph(I, QQ, n, 1, band_direct=-1) as G:
        assert G.stats()["band_block"] == 0
        G.set_rotations(Qgt)
        r = G.edge_diagnostics(allow_rc=(capi.ERR_UNSUPPORTED,))
        assert r["rc"] == capi.ERR_UNSUPPORTED and untouched(r)


@pytest.mark.parametrize("case", ["dense", "band", "closures"])
def test_singular_view_is_an_error(case):
    I, QQ, n, f, Q0, opts = _build(case)
    with capi.Graph(I, QQ, n, f, **opts) as G:
        G.set_rotations(Q0)
        v = f + (n - f) // 2
        d = np.ones(len(I))
        d[(I[:, 0] == v) | (I[:, 1] == v)] = 0.0
        G.set_weights(d)
        r = G.edge_diagnostics(allow_rc=(capi.ERR_SOLVER,))
        assert r["rc"] == capi.ERR_SOLVER and untouched(r)


def test_nothing_asked_is_a_bad_argument(fixture_graph):
    I, QQ, n, f, Q0 = fixture_state(fixture_graph)
    with capi.Graph(I, QQ, n, f) as G:
        G.set_rotations(Q0)
        assert capi.lib().irotavg_graph_edge_diagnostics(G._h, None, None, None, None) == capi.ERR_BAD_ARG
        # any subset is served, and only that subset
        full = G.edge_diagnostics()
        one = G.edge_diagnostics(edge_var=False, chi2=False)
        assert one["edge_var"] is None and one["chi2"] is None
        np.testing.assert_array_equal(one["leverage"], full["leverage"])
        c = G.edge_diagnostics(edge_var=False, leverage=False)
        np.testing.assert_array_equal(c["chi2"], full["chi2"])
        assert c["scale"] == full["scale"]


# ---- 6. read-only and deterministic ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["dense", "band", "closures"])
def test_query_is_read_only_and_deterministic(case):
    I, QQ, n, f, Q0, opts = _build(case)
    with solved_handle(I, QQ, n, f, Q0, l1=2, **opts) as A, solved_handle(I, QQ, n, f, Q0, l1=2, **opts) as Bt:
        Qa, wa, sa = A.get_rotations(), A.get_weights(), _stats_wo_time(A)
        A.edge_residual()
        ra = A.get_residuals()
        Bt.edge_residual()
        r1 = A.edge_diagnostics()
        r2 = A.edge_diagnostics()
        rb = Bt.edge_diagnostics()   # the twin's answer: bitwise between handles on the same graph ...
        for k in KEYS:
            np.testing.assert_array_equal(r1[k], r2[k])
            np.testing.assert_array_equal(r1[k], rb[k])
        assert r1["scale"] == r2["scale"] == rb["scale"]
        np.testing.assert_array_equal(A.get_rotations(), Qa)
        np.testing.assert_array_equal(A.get_weights(), wa)
        np.testing.assert_array_equal(A.get_residuals(), ra)
        assert _stats_wo_time(A) == sa
    # ... and a twin that never ran the query: a following rotation_variance and irls are bitwise the same
    with solved_handle(I, QQ, n, f, Q0, l1=2, **opts) as A, solved_handle(I, QQ, n, f, Q0, l1=2, **opts) as Bt:
        A.edge_diagnostics()
        P = I[np.random.default_rng(3).integers(0, len(I), size=40)]
        va, vb = A.rotation_variance(P), Bt.rotation_variance(P)
        for k in ("var", "pair_var"):
            np.testing.assert_array_equal(va[k], vb[k])
        assert va["scale"] == vb["scale"]
        A.edge_diagnostics()
        Qa = A.get_rotations()
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


# ---- 7. one-shot ---------------------------------------------------------------------------------------------------------
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
    r = capi.edge_diagnostics(I, QQ, Q, w, f)
    h1, _ = capi.oneshot_cache_stats()
    assert h1 == h0 + 1
    with capi.Graph(I, QQ, n, f) as G:
        G.set_rotations(Q)
        G.set_weights(w)
        rh = G.edge_diagnostics()
    for k in KEYS:
        np.testing.assert_array_equal(r[k], rh[k])
    assert r["scale"] == rh["scale"]


# ---- 8. planted outliers -------------------------------------------------------------------------------------------------
def test_planted_outliers_rank_first():
    """The input of test_planted_outliers_rank_first_in_the_reference (where the NumPy reference alone ranks the 20
    planted edges on top, smallest planted chi2 / largest other = 65): L2 weights, the GPU's own irls."""
    I, QQ, n, Qs, planted = outlier_graph()
    with capi.Graph(I, QQ, n, 1) as G:
        assert G.stats()["band_block"] > 0
        G.set_rotations(Qs)
        G.irls(0, SIGMA, 50, 1e-6)
        r = G.edge_diagnostics()
        d, res = state_of(G)
    np.testing.assert_array_equal(d, 1.0)
    check_all(r, edge_reference(I, n, 1, d, res), n - 1)
    order = np.argsort(-r["chi2"])
    assert set(order[:OUTLIER_K]) == set(planted)
    gap = r["chi2"][planted].min() / np.delete(r["chi2"], planted).max()
    print("planted-outlier gap on the device: %.2f" % gap)
    assert gap > OUTLIER_GAP
