"""Rotation-variance query (irotavg_graph_rotation_variance): the NumPy reference the GPU tests compare against
(block-tridiagonal LDL' + Takahashi recurrence for diag(A_b^-1), Woodbury for the loop closures), checked here against
np.linalg.inv, and the ABI of the query. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from irotavg_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------
def normal_matrix(I, n_total, f, d):
    """M = A' diag(d^2) A, dense, A from irotavg_make_A (the library's host-side make_A, ral/l1_irls.cpp:755-780)."""
    I = np.ascontiguousarray(I, dtype=np.int32)
    m, nu = len(I), n_total - f
    colptr = np.zeros(nu + 1, dtype=np.int64)
    rowidx = np.zeros(2 * m, dtype=np.int64)
    vals = np.zeros(2 * m)
    nnz = capi.lib().irotavg_make_A(n_total, f, m, capi._i(I), colptr.ctypes.data_as(capi._i64p),
                                    rowidx.ctypes.data_as(capi._i64p), capi._d(vals))
    assert nnz >= 0
    A = np.zeros((m, nu))
    for c in range(nu):
        for t in range(colptr[c], colptr[c + 1]):
            A[rowidx[t], c] += vals[t]
    return A.T @ (np.asarray(d)[:, None] ** 2 * A)


def edge_terms(I, f, d):
    """make_A's rows as (p, q, w): M = sum_k w_k (e_p - e_q)(e_p - e_q)' with q = -1 for a single coefficient."""
    I = np.asarray(I, dtype=np.int64)
    i, j = I[:, 0] - f, I[:, 1] - f
    w = np.asarray(d, dtype=np.float64) ** 2
    keep = j >= 0                                   # :770-771: no row when j is fixed
    single = keep & ((i < 0) | (i == j))            # one coefficient: +1 at j (i fixed) / -1 at i (self loop)
    p = np.where(keep, j, -1)
    q = np.where(keep & ~single, i, -1)
    return p[keep], q[keep], w[keep]


def split_band(p, q, w, nu, B):
    """Block-tridiagonal part (D, U: nb x B x B, padding rows = identity) and closures (block distance >= 2)."""
    nb = (nu + B - 1) // B
    far = (q >= 0) & (np.abs(p // B - q // B) >= 2)
    D = np.zeros((nb, B, B))
    U = np.zeros((nb, B, B))
    pb, qb, wb = p[~far], q[~far], w[~far]
    np.add.at(D, (pb // B, pb % B, pb % B), wb)
    two = qb >= 0
    pp, qq, ww = pb[two], qb[two], wb[two]
    np.add.at(D, (qq // B, qq % B, qq % B), ww)
    for a, b in ((pp, qq), (qq, pp)):
        same = a // B == b // B
        np.add.at(D, (a[same] // B, a[same] % B, b[same] % B), -ww[same])
        up = b // B == a // B + 1
        np.add.at(U, (a[up] // B, a[up] % B, b[up] % B), -ww[up])
    for r in range(nu, nb * B):
        D[r // B, r % B, r % B] = 1.0
    return D, U, (p[far], q[far], w[far])


def block_ldl(D, U):
    """Forward Schur complements S_k of the block tridiagonal matrix and their inverses."""
    nb = len(D)
    Sinv = np.zeros_like(D)
    for k in range(nb):
        S = D[k] - (U[k - 1].T @ Sinv[k - 1] @ U[k - 1] if k else 0.0)
        Sinv[k] = np.linalg.inv(S)
    return Sinv


def takahashi_diag(U, Sinv):
    """Diagonal blocks of the inverse: Sigma_kk = S_k^-1 + G_k Sigma_{k+1,k+1} G_k', G_k = S_k^-1 U_k."""
    nb = len(Sinv)
    Sig = np.zeros_like(Sinv)
    Sig[-1] = Sinv[-1]
    for k in range(nb - 2, -1, -1):
        G = Sinv[k] @ U[k]
        Sig[k] = Sinv[k] + G @ Sig[k + 1] @ G.T
    return Sig


def block_solve(U, Sinv, Y):
    """A_b^-1 Y (Y: nb B x ncol) through the block LDL'."""
    nb, B = len(Sinv), Sinv.shape[1]
    Y = Y.reshape(nb, B, -1).copy()
    for k in range(1, nb):
        Y[k] -= U[k - 1].T @ (Sinv[k - 1] @ Y[k - 1])
    X = np.zeros_like(Y)
    X[-1] = Sinv[-1] @ Y[-1]
    for k in range(nb - 2, -1, -1):
        X[k] = Sinv[k] @ (Y[k] - U[k] @ X[k + 1])
    return X.reshape(nb * B, -1)


def band_reference(I, n_total, f, d, B, pairs=()):
    """(var over n_total views, pair variances, band-only var) from the block recurrences + Woodbury."""
    nu = n_total - f
    p, q, w = edge_terms(I, f, d)
    D, U, (cp, cq, cw) = split_band(p, q, w, nu, B)
    nz = cw != 0
    cp, cq, cw = cp[nz], cq[nz], cw[nz]
    Sinv = block_ldl(D, U)
    band = np.einsum("kii->ki", takahashi_diag(U, Sinv)).ravel()[:nu]
    var = band.copy()
    nrow = len(D) * B
    k = len(cp)
    if k:
        V = np.zeros((nrow, k))
        V[cp, np.arange(k)] = 1.0
        V[cq, np.arange(k)] = -1.0
        Z = block_solve(U, Sinv, V)
        S = np.diag(1.0 / cw) + V.T @ Z
        Si = np.linalg.inv(S)
        var -= np.einsum("ij,ij->i", Z @ Si, Z)[:nu]
    pv = np.zeros(len(pairs))
    if len(pairs):
        Uu = np.zeros((nrow, len(pairs)))
        for t, (i, j) in enumerate(pairs):
            if i >= f:
                Uu[i - f, t] += 1.0
            if j >= f:
                Uu[j - f, t] -= 1.0
        Y = block_solve(U, Sinv, Uu)
        pv = np.einsum("it,it->t", Uu, Y)
        if k:
            T = V.T @ Y
            pv = pv - np.einsum("it,it->t", T, Si @ T)
    out = np.zeros(n_total)
    out[f:] = var
    band_out = np.zeros(n_total)
    band_out[f:] = band
    return out, pv, band_out


def dense_reference(I, n_total, f, d, pairs=()):
    """(var, pair variances) from np.linalg.inv of the dense normal matrix (assembled from make_A's rows)."""
    nu = n_total - f
    p, q, w = edge_terms(I, f, d)
    M = np.zeros((nu, nu))
    np.add.at(M, (p, p), w)
    two = q >= 0
    np.add.at(M, (q[two], q[two]), w[two])
    np.add.at(M, (p[two], q[two]), -w[two])
    np.add.at(M, (q[two], p[two]), -w[two])
    Sig = np.linalg.inv(M)
    var = np.zeros(n_total)
    var[f:] = np.diag(Sig)
    pv = []
    for i, j in pairs:
        u = np.zeros(n_total - f)
        if i >= f:
            u[i - f] += 1.0
        if j >= f:
            u[j - f] -= 1.0
        pv.append(u @ Sig @ u)
    return var, np.array(pv)


def scale_reference(I, f, d, residuals, nu):
    """s^2 = sum d^2 |r|^2 / (3 (m_A - nu)) over the edges whose row of A is not zero."""
    keep = np.asarray(I)[:, 1] >= f
    mA = int(keep.sum())
    if mA <= nu:
        return np.nan
    return float(np.sum(np.asarray(d)[keep] ** 2 * np.sum(residuals[keep] ** 2, axis=1)) / (3 * (mA - nu)))


def random_band_graph(rng, n, f, band, ncl):
    """A view sequence (every view tied to its predecessors within `band`) with ncl random long-range edges."""
    I = []
    for j in range(1, n):
        for dd in range(1, band + 1):
            if j - dd >= 0 and rng.random() < 0.8 or dd == 1:
                I.append((j - dd, j))
    for _ in range(ncl):
        a, b = sorted(rng.choice(n, 2, replace=False))
        if b - a > 2 * band + 64:
            I.append((a, b))
    I = np.array(I, dtype=np.int32)
    d = rng.uniform(0.2, 2.0, size=len(I))
    return I, d


# ---- the reference against np.linalg.inv --------------------------------------------------------------------------
@pytest.mark.parametrize("B,ncl,seed", [(8, 0, 0), (8, 20, 1), (16, 50, 2), (24, 0, 3), (24, 35, 4), (32, 50, 5),
                                        (32, 1, 6)])
def test_band_reference_matches_dense_inverse(B, ncl, seed):
    rng = np.random.default_rng(seed)
    n, f = 400 + 37 * seed, 1 + seed % 2
    I, d = random_band_graph(rng, n, f, min(B, 6), ncl)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, n, size=(12, 2))] + [(0, 0), (5, 5), (0, n - 1)]
    var, pv, band = band_reference(I, n, f, d, B, pairs)
    vd, pd = dense_reference(I, n, f, d, pairs)
    np.testing.assert_allclose(var, vd, rtol=1e-9, atol=0)
    np.testing.assert_allclose(pv, pd, rtol=1e-9, atol=1e-15)
    assert np.all(var[f:] <= band[f:] * (1 + 1e-12))   # closures only add information


def test_edge_terms_follow_make_A_quirk():
    # (i free, j fixed) is dropped, (i fixed, j free) keeps +1 at j, a self loop keeps -1 at i
    I = np.array([[3, 0], [0, 3], [2, 2], [1, 2], [2, 3]], dtype=np.int32)
    d = np.array([5.0, 2.0, 3.0, 1.5, 0.5])
    p, q, w = edge_terms(I, 1, d)
    M = np.zeros((3, 3))
    for a, b, ww in zip(p, q, w):
        u = np.zeros(3)
        u[a] += 1
        if b >= 0:
            u[b] -= 1
        M += ww * np.outer(u, u)
    np.testing.assert_allclose(M, normal_matrix(I, 4, 1, d), rtol=1e-15)
    rng = np.random.default_rng(9)
    I, d = random_band_graph(rng, 60, 2, 4, 5)
    I = np.concatenate([I, [[0, 7], [9, 1], [11, 11]]]).astype(np.int32)
    d = np.concatenate([d, [1.0, 2.0, 0.5]])
    var, _ = dense_reference(I, 60, 2, d)
    np.testing.assert_allclose(var[2:], np.diag(np.linalg.inv(normal_matrix(I, 60, 2, d))), rtol=1e-12)


def test_scale_reference_counts_only_rows_of_A():
    I = np.array([[0, 1], [1, 2], [2, 0]], dtype=np.int32)
    r = np.ones((3, 3))
    s = scale_reference(I, 1, np.ones(3), r, 2)
    assert np.isnan(s)   # m_A = 2 <= nu = 2
    I = np.array([[0, 1], [1, 2], [0, 2], [2, 1]], dtype=np.int32)
    assert scale_reference(I, 1, np.ones(4), np.ones((4, 3)), 2) == pytest.approx(4 * 3 / (3 * 2))


# ---- ABI ----------------------------------------------------------------------------------------------------------
def test_header_declares_the_query_and_binding_lists_it():
    src = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    for s in ("irotavg_graph_rotation_variance", "irotavg_rotation_variance"):
        assert re.search(r"\bint\s+" + s + r"\s*\(", src), s
        assert s in capi.SYMBOLS
        assert hasattr(capi.lib(), s)
    assert re.search(r"#define\s+IROTAVG_ERR_UNSUPPORTED\s+\(-9\)", src)
    assert capi.ERR_UNSUPPORTED == -9


def test_unsupported_error_string():
    msg = capi.lib().irotavg_error_string(capi.ERR_UNSUPPORTED)
    assert msg != capi.lib().irotavg_error_string(-100) and b"not supported" in msg


def test_bad_arguments_are_refused_before_device_work():
    L = capi.lib()
    I = np.array([[0, 1], [1, 2]], dtype=np.int32)
    QQ = capi.fmat(np.tile([0, 0, 0, 1.0], (2, 1)))
    Q = capi.fmat(np.tile([0, 0, 0, 1.0], (3, 1)))
    w = np.ones(2)
    pv = np.zeros(1)
    bad = np.array([0, 3], dtype=np.int32)      # view 3 of 3
    rc = L.irotavg_rotation_variance(2, 3, 1, capi._i(I), capi._d(QQ), 2, capi._d(Q), 3, capi._d(w), None, 1,
                                     capi._i(bad), capi._d(pv), None)
    assert rc == capi.ERR_BAD_ARG
    rc = L.irotavg_rotation_variance(2, 3, 1, capi._i(I), capi._d(QQ), 2, capi._d(Q), 3, capi._d(w), None, -1,
                                     None, None, None)
    assert rc == capi.ERR_BAD_ARG
    assert L.irotavg_graph_rotation_variance(None, None, 0, None, None, None) == capi.ERR_BAD_ARG
