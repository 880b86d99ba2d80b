"""Edge diagnostics (irotavg_graph_edge_diagnostics): the NumPy reference the GPU tests compare against, checked here
for the properties of a hat matrix (trace, range, zero rows, bridges) and against the rotation-variance reference, the
planted-outlier input of the GPU test run through the reference alone, and the ABI of the query. No GPU."""
import os
import re

import numpy as np
import pytest

from irotavg_amd import capi, synth
from oracle import oracle as O
from test_rotation_variance_cpu import (block_ldl, block_solve, dense_reference, edge_terms, random_band_graph,
                                         scale_reference, split_band, takahashi_diag)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------
def edge_reference(I, n_total, f, d, res):
    """dict(edge_var, leverage, chi2, scale) over all edges from np.linalg.inv of M = A' diag(d^2) A.
    res: (m, 3) edge residuals. Row k of A: +1 at j - f unless j is fixed (then the row is zero, ral/l1_irls.cpp:770-771),
    -1 at i - f when i is free too; a self loop keeps the -1 alone."""
    I = np.asarray(I, dtype=np.int64)
    d = np.asarray(d, dtype=np.float64)
    nu = n_total - f
    i, j = I[:, 0] - f, I[:, 1] - f
    keep = j >= 0
    two = keep & (i >= 0) & (i != j)
    w = d ** 2
    M = np.zeros((nu, nu))
    np.add.at(M, (j[keep], j[keep]), w[keep])
    np.add.at(M, (i[two], i[two]), w[two])
    np.add.at(M, (j[two], i[two]), -w[two])
    np.add.at(M, (i[two], j[two]), -w[two])
    Sig = np.linalg.inv(M)
    ev = np.zeros(len(I))
    ev[keep] = Sig[j[keep], j[keep]]
    ev[two] += Sig[i[two], i[two]] - (Sig[i[two], j[two]] + Sig[j[two], i[two]])
    lev = w * ev
    s2 = scale_reference(I, f, d, res, nu)
    with np.errstate(divide="ignore", invalid="ignore"):
        chi2 = w * np.sum(np.asarray(res) ** 2, axis=1) / (s2 * np.maximum(0.0, 1.0 - lev))
    return dict(edge_var=ev, leverage=lev, chi2=chi2, scale=s2)


def band_edge_reference(I, n_total, f, d, B, res):
    """The same dict from the block recurrences of the variance reference, for graphs too large for a dense inverse:
    block LDL' of the block-tridiagonal part, Takahashi's recurrence for Sigma_kk and Sigma_k,k+1 = -G_k Sigma_k+1,k+1
    (every band edge lies inside one block or two neighbouring ones), the closure edges through block_solve, and the
    Woodbury term (Z_a - Z_b) S^-1 (Z_a - Z_b)' of every edge."""
    I = np.asarray(I, dtype=np.int64)
    d = np.asarray(d, dtype=np.float64)
    nu = n_total - f
    i, j = I[:, 0] - f, I[:, 1] - f
    keep = j >= 0
    two = keep & (i >= 0) & (i != j)
    p, q, w = edge_terms(I, f, d)
    D, U, (cp, cq, cw) = split_band(p, q, w, nu, B)
    nz = cw != 0
    cp, cq, cw = cp[nz], cq[nz], cw[nz]
    Sinv = block_ldl(D, U)
    SD = takahashi_diag(U, Sinv)
    SU = np.zeros_like(SD)
    for k in range(len(D) - 1):
        SU[k] = -(Sinv[k] @ U[k]) @ SD[k + 1]
    a = np.where(keep, j, 0)
    b = np.where(two, i, 0)
    ev = np.where(keep, SD[a // B, a % B, a % B], 0.0)
    ev += np.where(two, SD[b // B, b % B, b % B], 0.0)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    same = two & (lo // B == hi // B)
    up = two & (hi // B == lo // B + 1)
    far = two & (hi // B >= lo // B + 2)
    ev[same] -= 2 * SD[lo[same] // B, lo[same] % B, hi[same] % B]
    ev[up] -= 2 * SU[lo[up] // B, lo[up] % B, hi[up] % B]
    nrow = len(D) * B
    if far.any():
        t = np.flatnonzero(far)
        Uu = np.zeros((nrow, len(t)))
        Uu[a[t], np.arange(len(t))] = 1.0
        Uu[b[t], np.arange(len(t))] = -1.0
        ev[t] = np.einsum("it,it->t", Uu, block_solve(U, Sinv, Uu))
    if len(cp):
        V = np.zeros((nrow, len(cp)))
        V[cp, np.arange(len(cp))] = 1.0
        V[cq, np.arange(len(cp))] = -1.0
        Z = block_solve(U, Sinv, V)
        Si = np.linalg.inv(np.diag(1.0 / cw) + V.T @ Z)
        for t0 in range(0, len(I), 16384):
            sl = slice(t0, t0 + 16384)
            E = np.where(keep[sl, None], Z[a[sl]], 0.0) - np.where(two[sl, None], Z[b[sl]], 0.0)
            ev[sl] -= np.einsum("tc,tc->t", E @ Si, E)
    lev = d ** 2 * ev
    s2 = scale_reference(I, f, d, res, nu)
    with np.errstate(divide="ignore", invalid="ignore"):
        chi2 = d ** 2 * np.sum(np.asarray(res) ** 2, axis=1) / (s2 * np.maximum(0.0, 1.0 - lev))
    return dict(edge_var=ev, leverage=lev, chi2=chi2, scale=s2)


def quirk_graph(seed=3, n=90, f=3):
    """A small sequence with 3 fixed views and every kind of row: (free, fixed) dropped, (fixed, free), (fixed, fixed),
    a self loop, a closure."""
    rng = np.random.default_rng(seed)
    I, d = random_band_graph(rng, n, f, 5, 4)
    extra = np.array([[7, 1], [2, 11], [0, 2], [13, 13], [1, 40], [50, 0]], dtype=np.int32)
    I = np.concatenate([I, extra]).astype(np.int32)
    d = np.concatenate([d, rng.uniform(0.2, 2.0, size=len(extra))])
    return I, d, n, f


# ---- properties of the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_is_a_hat_matrix_diagonal(seed):
    I, d, n, f = quirk_graph(seed)
    res = np.random.default_rng(seed).normal(size=(len(I), 3))
    r = edge_reference(I, n, f, d, res)
    nu = n - f
    assert abs(r["leverage"].sum() - nu) <= 1e-9 * nu
    assert np.all(r["leverage"] >= 0) and np.all(r["leverage"] <= 1 + 1e-9)
    zero = I[:, 1] < f
    assert zero.any() and np.all(r["edge_var"][zero] == 0) and np.all(r["leverage"][zero] == 0)
    # an edge with only its first view fixed: Sigma_jj
    var, _ = dense_reference(I, n, f, d)
    first = (I[:, 0] < f) & (I[:, 1] >= f)
    assert first.any()
    np.testing.assert_allclose(r["edge_var"][first], var[I[first, 1]], rtol=1e-12)
    # the same numbers as the variance reference gives for the edges as pairs (rows of A that are not zero)
    # (a self loop is u = 0 as a pair but a single -1 as a row of A: left out here, it is Sigma_ii)
    rows = ~zero & (I[:, 0] != I[:, 1])
    _, pv = dense_reference(I, n, f, d, [tuple(e) for e in I[rows]])
    np.testing.assert_allclose(r["edge_var"][rows], pv, rtol=1e-9, atol=0)
    loop = I[:, 0] == I[:, 1]
    assert loop.any()
    np.testing.assert_allclose(r["edge_var"][loop], var[I[loop, 1]], rtol=1e-12)
    assert np.all(np.isfinite(r["chi2"])) and np.all(r["chi2"] >= 0)


@pytest.mark.parametrize("B,ncl,seed", [(8, 0, 0), (8, 20, 1), (16, 50, 2), (24, 0, 3), (24, 35, 4), (32, 50, 5)])
def test_band_edge_reference_matches_dense_inverse(B, ncl, seed):
    rng = np.random.default_rng(seed)
    n, f = 400 + 37 * seed, 1 + seed % 2
    I, d = random_band_graph(rng, n, f, min(B, 6), ncl)
    I = np.concatenate([I, [[0, 9], [12, 0], [15, 15]]]).astype(np.int32)
    d = np.concatenate([d, [1.5, 0.5, 0.0]])
    if ncl:
        d[np.flatnonzero(np.abs(I[:, 0] - I[:, 1]) > 64)[:2]] = 0.0   # closures of weight zero
    res = rng.normal(size=(len(I), 3))
    r, rb = edge_reference(I, n, f, d, res), band_edge_reference(I, n, f, d, B, res)
    for k in ("edge_var", "leverage", "chi2"):
        np.testing.assert_allclose(rb[k], r[k], rtol=1e-9, atol=0)
    assert rb["scale"] == r["scale"]


def test_bridge_edges_have_leverage_one():
    # view n hangs on one edge from a fixed view (weight 2: 1 / 4 and 4 x 1 / 4 are exact), view n + 1 on one from a
    # free view, view n + 2 likewise with a zero residual
    I, d, n, f = quirk_graph(5)
    m0 = len(I)
    I = np.concatenate([I, [[0, n], [20, n + 1], [21, n + 2]]]).astype(np.int32)
    d = np.concatenate([d, [2.0, 0.7, 1.3]])
    res = np.random.default_rng(5).normal(size=(len(I), 3))
    res[m0 + 2] = 0.0
    r = edge_reference(I, n + 3, f, d, res)
    assert r["leverage"][m0] == 1.0 and np.isposinf(r["chi2"][m0])
    np.testing.assert_allclose(r["leverage"][m0 + 1:], 1.0, rtol=1e-9)
    assert abs(r["leverage"].sum() - (n + 3 - f)) <= 1e-9 * (n + 3 - f)
    res[m0] = 0.0
    r = edge_reference(I, n + 3, f, d, res)
    assert np.isnan(r["chi2"][m0])          # 0 / 0
    assert r["chi2"][m0 + 2] == 0.0 or np.isnan(r["chi2"][m0 + 2])   # 0 / (s^2 max(0, rounding))
    # s^2 NaN (no redundancy at all): every chi2 is NaN
    I2 = np.array([[0, 1], [1, 2]], dtype=np.int32)
    r = edge_reference(I2, 3, 1, np.ones(2), np.ones((2, 3)))
    assert np.isnan(r["scale"]) and np.isnan(r["chi2"]).all()
    np.testing.assert_allclose(r["leverage"], 1.0, rtol=1e-12)


# ---- the planted-outlier input of the GPU test ---------------------------------------------------------------------------
OUTLIER_N, OUTLIER_DEG, OUTLIER_K, OUTLIER_ANGLE, OUTLIER_SEED = 3000, 10, 20, 0.5, 17
OUTLIER_GAP = 3.0   # smallest planted chi2 / largest other chi2 that the reference must show (it shows more, see the test)


def outlier_graph():
    """A noisy view sequence (make_graph: sigma 0.01 rad, no outliers of its own) in which OUTLIER_K edges are replaced
    by the true relative rotation times a rotation of OUTLIER_ANGLE rad about a random axis."""
    n = OUTLIER_N
    S = synth.make_graph(n, OUTLIER_DEG * n - OUTLIER_DEG * (OUTLIER_DEG + 1) // 2, 0.0, p_out=0.0, seed=OUTLIER_SEED)
    I, QQ, Qgt = S["I"].astype(np.int32), S["QQ"].copy(), S["Qgt"]
    rng = np.random.default_rng(OUTLIER_SEED)
    planted = np.sort(rng.choice(len(I), OUTLIER_K, replace=False))
    ax = rng.normal(size=(OUTLIER_K, 3))
    ax *= OUTLIER_ANGLE / np.linalg.norm(ax, axis=1, keepdims=True)
    a, b = I[planted, 0], I[planted, 1]
    QQ[planted] = synth.qmul(synth.qexp(ax), synth.qmul(Qgt[b], synth.qconj(Qgt[a])))
    Qs = np.zeros_like(Qgt)
    Qs[:, 3] = 1
    Qs[0] = Qgt[0]
    rc, Qs = O.init_mst(Qs, QQ, I, 1)
    assert rc == 0
    return I, QQ, n, Qs, planted


def residual_norms(I, QQ, Q):
    """|r_k|: the angle between QQ_k Q_i and Q_j (the norm of the edge residual whatever its sign convention)."""
    return synth.angular_distance(synth.qmul(QQ, Q[I[:, 0]]), Q[I[:, 1]])


def test_planted_outliers_rank_first_in_the_reference():
    I, QQ, n, Qs, planted = outlier_graph()
    r = O.irls(QQ, I, Qs, 1, 0, 5 * np.pi / 180, 50, 1e-6)   # cost 0: L2, d = 1
    assert r["rc"] == 0
    np.testing.assert_array_equal(r["weights"], 1.0)
    res = np.zeros((len(I), 3))
    res[:, 0] = residual_norms(I, QQ, r["Q"])
    ref = edge_reference(I, n, 1, r["weights"], res)
    order = np.argsort(-ref["chi2"])
    assert set(order[:OUTLIER_K]) == set(planted)
    gap = ref["chi2"][planted].min() / np.delete(ref["chi2"], planted).max()
    print("planted-outlier gap of the reference: %.2f" % gap)
    assert gap > OUTLIER_GAP


# ---- ABI ----------------------------------------------------------------------------------------------------------
def test_header_declares_the_query_and_binding_lists_it():
    src = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    for s in ("irotavg_graph_edge_diagnostics", "irotavg_edge_diagnostics"):
        assert re.search(r"\bint\s+" + s + r"\s*\(", src), s
        assert s in capi.SYMBOLS
        assert hasattr(capi.lib(), s)
    assert callable(capi.Graph.edge_diagnostics) and callable(capi.edge_diagnostics)


def test_bad_arguments_are_refused_before_device_work():
    L = capi.lib()
    I = np.array([[0, 1], [1, 2]], dtype=np.int32)
    QQ = capi.fmat(np.tile([0, 0, 0, 1.0], (2, 1)))
    Q = capi.fmat(np.tile([0, 0, 0, 1.0], (3, 1)))
    w = np.ones(2)
    out = np.zeros(2)
    # nothing asked for
    rc = L.irotavg_edge_diagnostics(2, 3, 1, capi._i(I), capi._d(QQ), 2, capi._d(Q), 3, capi._d(w), None, None, None, None)
    assert rc == capi.ERR_BAD_ARG
    # no rotations / weights
    rc = L.irotavg_edge_diagnostics(2, 3, 1, capi._i(I), capi._d(QQ), 2, None, 3, capi._d(w), capi._d(out), None, None,
                                    None)
    assert rc == capi.ERR_BAD_ARG
    assert L.irotavg_graph_edge_diagnostics(None, capi._d(out), None, None, None) == capi.ERR_BAD_ARG


def test_unsupported_error_string_names_both_queries():
    msg = capi.lib().irotavg_error_string(capi.ERR_UNSUPPORTED)
    assert b"not supported" in msg and b"edge diagnostics" in msg and b"rotation variance" in msg
