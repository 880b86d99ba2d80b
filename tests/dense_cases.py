"""Graphs whose inverse normal matrix is known exactly, for the blocked Gauss-Jordan sweep of irotavg_amd/csrc/dense.hip,
shared by the CPU test of the cases themselves (test_dense_cases_cpu.py) and the GPU test (test_gpu_dense_inverse.py).
A plain module: building a case needs no device.

M = A' diag(d^2) A is the scalar Dirichlet Laplacian of the handle (A = make_A's incidence: an edge whose SECOND view is
fixed has no row, one whose first view is fixed keeps a single coefficient), S = M^-1. Every generator returns a dict
with I, QQ, Q0, d, f, n and the exact S as np.longdouble (free views x free views, row = view - f):

* forest   -- every free view hangs by one edge on a view created earlier, the f fixed views are the roots, the free ids
              are permuted at random (sparsity scattered over all tiles). S_ij = sum of 1 / d_e^2 over the edges that the
              root paths of i and j share, 0 for views under different roots: sums only, no cancellation;
* rank_one -- an edge from fixed view 0 to every free view (weights c_v) and the complete graph on the free views (one
              weight b): M = P - b^2 11', P = diag(c^2 + nu b^2), S by Sherman-Morrison. Fully dense;
* band     -- a view sequence whose edges span at most bw views, weights over two decades; S by a long-double Cholesky
              with two rounds of refinement (the manner of tools/referee.py), for small nu only (band_solve serves the
              large ones).

The relative rotations are noise-free (QQ from random ground truth); Q0 is the ground truth moved by ~0.05 rad on the free
views, so that a linear solve from Q0 has a right-hand side.

The comparison (scaled_reference / entry_error) is the one the issue of this test fixes: errors are measured on the
Jacobi-scaled inverse D^1/2 S D^1/2, D = diag(M) -- what k_mv_dense_scale makes the sweep invert -- relative to its
largest entry, and the bound is 8 x max(e_ref, nu 2^-52) with e_ref the error of numpy's LAPACK inverse of the same
scaled fp64 matrix on that norm.
"""
import numpy as np

from irotavg_amd import synth

LD = np.longdouble
EPS = 2.0 ** -52
FACTOR = 8.0        # allowance over the reference's own error for an unpivoted sweep with a Newton reciprocal


# ---- the operator -------------------------------------------------------------------------------------------------
def edge_terms(I, f, w):
    """make_A's rows as (p, q, w): M = sum_k w_k (e_p - e_q)(e_p - e_q)', q = -1 for a single coefficient."""
    I = np.asarray(I, dtype=np.int64)
    i, j = I[:, 0] - f, I[:, 1] - f
    keep = j >= 0
    single = keep & ((i < 0) | (i == j))
    p = np.where(keep, j, -1)
    q = np.where(keep & ~single, i, -1)
    return p[keep], q[keep], w[keep]


def normal_matrix(case, dtype=np.float64):
    """M (nu x nu) accumulated in `dtype` from the squares of the fp64 weights."""
    nu = case["n"] - case["f"]
    d = np.asarray(case["d"], dtype=dtype)
    p, q, w = edge_terms(case["I"], case["f"], d * d)
    M = np.zeros((nu, nu), dtype=dtype)
    np.add.at(M, (p, p), w)
    two = q >= 0
    np.add.at(M, (q[two], q[two]), w[two])
    np.add.at(M, (p[two], q[two]), -w[two])
    np.add.at(M, (q[two], p[two]), -w[two])
    return M


def _finish(rng, I, d, n, f, S, **extra):
    I = np.asarray(I, dtype=np.int32).reshape(-1, 2)
    Qgt = rng.normal(size=(n, 4))
    Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    QQ = synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]]))
    Q0 = synth.qmul(synth.qexp(rng.normal(scale=0.05, size=(n, 3))), Qgt)
    Q0[:f] = Qgt[:f]
    case = dict(I=I, QQ=QQ, Q0=Q0, d=np.asarray(d, dtype=np.float64), f=f, n=n, S=S)
    case.update(extra)
    return case


# ---- long-double Cholesky (dense, or within a half-bandwidth) -------------------------------------------------------
def chol_ld(M, bw=None):
    L = np.array(M, dtype=LD)
    n = L.shape[0]
    bw = n if bw is None else bw
    for j in range(n):
        lo, hi = max(0, j - bw), min(n, j + bw + 1)
        L[j, j] = np.sqrt(L[j, j] - L[j, lo:j] @ L[j, lo:j])
        if j + 1 < hi:
            L[j + 1:hi, j] = (L[j + 1:hi, j] - L[j + 1:hi, lo:j] @ L[j, lo:j]) / L[j, j]
    return np.tril(L)


def chol_solve_ld(M, B, bw=None):
    """M^-1 B in long double: Cholesky (entries beyond the half-bandwidth bw are zero) + two rounds of refinement."""
    M = np.array(M, dtype=LD)
    n = M.shape[0]
    L = chol_ld(M, bw)
    bw = n if bw is None else bw

    def solve(R):
        Y = np.array(R, dtype=LD)
        for j in range(n):
            lo = max(0, j - bw)
            Y[j] = (Y[j] - L[j, lo:j] @ Y[lo:j]) / L[j, j]
        for j in range(n - 1, -1, -1):
            hi = min(n, j + bw + 1)
            Y[j] = (Y[j] - L[j + 1:hi, j] @ Y[j + 1:hi]) / L[j, j]
        return Y
    B = np.array(B, dtype=LD)
    X = solve(B)
    for _ in range(2):
        X = X + solve(B - M @ X)
    return X


# ---- the three families ---------------------------------------------------------------------------------------------
def forest(nu, f, seed=0):
    rng = np.random.default_rng([101, nu, f, seed])
    n = nu + f
    parent = np.array([rng.integers(0, f + c) for c in range(nu)])   # creation order: the roots, then the free views
    perm = rng.permutation(nu)                                       # creation index -> row of the operator
    d = rng.uniform(0.3, 3.0, size=nu)
    view = np.concatenate([np.arange(f), f + perm])
    I = np.stack([view[parent], view[f + np.arange(nu)]], axis=1)
    Sc = np.zeros((nu, nu), dtype=LD)
    for c in range(nu):
        inv = 1 / (LD(d[c]) * LD(d[c]))
        pk = parent[c] - f
        if pk >= 0:                                   # shares its parent's root path with every earlier view
            Sc[c, :c] = Sc[pk, :c]
            Sc[:c, c] = Sc[pk, :c]
            inv = inv + Sc[pk, pk]
        Sc[c, c] = inv
    S = np.zeros_like(Sc)
    S[np.ix_(perm, perm)] = Sc
    return _finish(rng, I, d, n, f, S, family="forest")


def rank_one(nu, seed=0):
    assert nu <= 256
    rng = np.random.default_rng([102, nu, seed])
    f, n = 1, nu + 1
    c = rng.uniform(0.5, 2.0, size=nu)
    b = 0.7
    iu, ju = np.triu_indices(nu, 1)
    I = np.concatenate([np.stack([np.zeros(nu, dtype=np.int64), 1 + np.arange(nu)], 1), np.stack([1 + iu, 1 + ju], 1)])
    d = np.concatenate([c, np.full(len(iu), b)])
    b2 = LD(b) * LD(b)
    pinv = 1 / (np.asarray(c, dtype=LD) ** 2 + nu * b2)
    S = np.diag(pinv) + b2 * np.outer(pinv, pinv) / (1 - b2 * pinv.sum())
    return _finish(rng, I, d, n, f, S, family="rank_one")


def band(nu, bw, f=2, seed=0, inverse=True):
    """Half-bandwidth exactly min(bw, nu - 1) between free views. inverse=False: S is None (a large nu: band_solve)."""
    rng = np.random.default_rng([103, nu, bw, f, seed])
    n = nu + f
    I = []
    for j in range(f, n):
        for dd in range(1, bw + 1):
            if j - dd >= 0 and (dd == 1 or dd == bw or rng.random() < 0.8):
                I.append((j - dd, j))
    d = 10.0 ** rng.uniform(-1.0, 1.0, size=len(I))
    case = _finish(rng, I, d, n, f, None, family="band", bw=bw)
    if inverse:
        assert nu <= 193
        S = chol_solve_ld(normal_matrix(case, LD), np.eye(nu), bw)
        case["S"] = (S + S.T) / 2
    return case


def band_solve(case, B):
    """M^-1 B of a band case in long double."""
    return chol_solve_ld(normal_matrix(case, LD), B, case["bw"])


# ---- the outputs of the query, and the comparison -------------------------------------------------------------------
def all_pairs(n):
    a, b = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.stack([a.ravel(), b.ravel()], 1).astype(np.int32)


def seam_rows(nu):
    """Rows 32 k - 1 and 32 k (which include 64 k - 1 and 64 k): the seams of the sweep's blocks and tiles."""
    k = np.arange(0, nu // 32 + 2) * 32
    r = np.unique(np.concatenate([k - 1, k]))
    return r[(r >= 0) & (r < nu)]


def sample_pairs(case, count, seed=0):
    """`count` random pairs of views + every ordered pair among the views on a block or tile seam."""
    n, f = case["n"], case["f"]
    rng = np.random.default_rng([104, n, seed])
    s = f + seam_rows(n - f)
    a, b = np.meshgrid(s, s, indexing="ij")
    return np.concatenate([rng.integers(0, n, size=(count, 2)), np.stack([a.ravel(), b.ravel()], 1)]).astype(np.int32)


def outputs_from(S, f, P):
    """What the query returns for an inverse S, in fp64 and by its own formula: var = S_vv, pair_var = S_ii + S_jj - 2 S_ij
    with a fixed endpoint dropped."""
    S = np.asarray(S, dtype=np.float64)
    nu = len(S)
    var = np.concatenate([np.zeros(f), np.diag(S)])
    i, j = P[:, 0] - f, P[:, 1] - f
    ci, cj = np.clip(i, 0, nu - 1), np.clip(j, 0, nu - 1)
    pv = np.where(i >= 0, S[ci, ci], 0.0) + np.where(j >= 0, S[cj, cj], 0.0)
    both = (i >= 0) & (j >= 0)
    pv = pv - np.where(both, S[ci, cj] + S[cj, ci], 0.0)
    pv[i == j] = 0.0
    return var, pv


def scaled_reference(case):
    """e_ref, the norm and the bound for a case (see the module docstring)."""
    nu = case["n"] - case["f"]
    M = normal_matrix(case)
    sc = 1.0 / np.sqrt(np.diag(M))
    Ms = M * sc[:, None] * sc[None, :]
    np.fill_diagonal(Ms, 1.0)
    sq = np.sqrt(np.diag(normal_matrix(case, LD)))
    Ss = case["S"] * sq[:, None] * sq[None, :]
    smax = np.abs(Ss).max()
    e_ref = float(np.abs(np.linalg.inv(Ms) - Ss).max() / smax)
    return dict(e_ref=e_ref, smax=smax, sq=sq, tol=FACTOR * max(e_ref, nu * EPS))


def entry_error(case, ref, var, P, pv):
    """(error, zeros_exact): the largest error of the marginals and of every entry S_ij recovered from the outputs, on the
    norm of e_ref; whether var of the fixed views and pair_var of i == j / two fixed views are exactly 0."""
    f, S, sq, smax = case["f"], case["S"], ref["sq"], ref["smax"]
    assert len(S) == len(sq)
    var, pv = np.asarray(var, dtype=LD), np.asarray(pv, dtype=LD)
    err = [np.abs(var[f:] - np.diag(S)) * sq * sq]
    i, j = P[:, 0].astype(np.int64) - f, P[:, 1].astype(np.int64) - f
    zero = (i == j) | ((i < 0) & (j < 0))
    zeros_exact = bool(np.all(var[:f] == 0) and np.all(pv[zero] == 0))
    one = ~zero & ((i < 0) | (j < 0))
    k = np.maximum(i, j)[one]
    err.append(np.abs(pv[one] - S[k, k]) * sq[k] * sq[k])
    two = ~zero & ~one
    a, b = i[two], j[two]
    rec = (var[f + a] + var[f + b] - pv[two]) / 2          # S_ij from three outputs
    err.append(np.abs(rec - S[a, b]) * sq[a] * sq[b])
    return float(max(e.max() for e in err if e.size) / smax), zeros_exact
