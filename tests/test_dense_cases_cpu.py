"""The known-answer cases of dense_cases.py checked on the CPU: the exact inverses invert, the pair formula gives back
every entry, and the comparison the GPU test uses (dense_cases.entry_error against dense_cases.scaled_reference) passes on
the exact answer and fails on an inverse with one entry moved by 1e-9 relative. No GPU."""
import numpy as np
import pytest

import dense_cases as DC

CASES = {
    "forest-64-f1": lambda: DC.forest(64, 1),
    "forest-193-f3": lambda: DC.forest(193, 3),
    "rank_one-65": lambda: DC.rank_one(65),
    "rank_one-256": lambda: DC.rank_one(256),
    "band6-63": lambda: DC.band(63, 6),
    "band6-193": lambda: DC.band(193, 6),
}
_made = {}


def case_of(name):
    if name not in _made:
        c = CASES[name]()
        _made[name] = (c, DC.scaled_reference(c))
    return _made[name]


@pytest.mark.parametrize("name", list(CASES))
def test_exact_inverse_inverts(name):
    c, ref = case_of(name)
    nu = c["n"] - c["f"]
    M = DC.normal_matrix(c)
    S = np.asarray(c["S"], dtype=np.float64)
    r = np.abs(M @ S - np.eye(nu)).max()
    cond = np.linalg.cond(M)
    bound = 64 * nu * DC.EPS * cond
    print("%s: max|M S - I| = %.2e (bound %.2e), cond %.2e, e_ref %.2e" % (name, r, bound, cond, ref["e_ref"]))
    assert r < bound
    assert np.array_equal(c["S"], c["S"].T)


def test_forest_has_the_stated_shape():
    c = DC.forest(2048, 3)
    I, f = c["I"], c["f"]
    assert len(I) == 2048 and np.all(I[:, 1] >= f) and len(np.unique(I[:, 1])) == 2048   # one edge above every free view
    assert (I[:, 0] < f).sum() >= 1 and c["d"].min() >= 0.3 and c["d"].max() <= 3.0
    S = c["S"]
    assert (S == 0).any() and np.all(np.diag(S) > 0)                                     # views under different roots
    # spans of the free-free edges are scattered: most are loop-closure long
    ff = I[I[:, 0] >= f]
    assert (np.abs(ff[:, 0] - ff[:, 1]) > 32).mean() > 0.9
    M = DC.normal_matrix(c)
    r = np.abs(M @ np.asarray(S, dtype=np.float64) - np.eye(2048)).max()
    assert r < 64 * 2048 * DC.EPS * np.linalg.cond(M)


@pytest.mark.parametrize("bw", [1, 2, 3, 4, 5])
def test_band_cases_have_their_half_bandwidth(bw):
    c = DC.band(65, bw, inverse=False)
    I, f = c["I"], c["f"]
    ff = I[I[:, 0] >= f]
    assert np.abs(ff[:, 0] - ff[:, 1]).max() == bw and np.all(I[:, 1] >= f)
    # the banded long-double solve is the dense one
    B = np.random.default_rng(bw).normal(size=(65, 3))
    X = DC.band_solve(c, B)
    Xd = DC.chol_solve_ld(DC.normal_matrix(c, DC.LD), B)
    assert np.abs(X - Xd).max() < 1e-17 * np.abs(Xd).max()
    M = DC.normal_matrix(c, DC.LD)
    assert np.abs(M @ X - B).max() < 1e-17 * (np.abs(M) @ np.abs(X)).max()


@pytest.mark.parametrize("name", list(CASES))
def test_pair_formula_gives_back_every_entry(name):
    c, ref = case_of(name)
    f, n = c["f"], c["n"]
    P = DC.all_pairs(n)
    var, pv = DC.outputs_from(c["S"], f, P)
    S = np.asarray(c["S"], dtype=np.float64)
    i, j = P[:, 0] - f, P[:, 1] - f
    both = (i >= 0) & (j >= 0)
    rec = (var[P[both, 0]] + var[P[both, 1]] - pv[both]) / 2
    assert np.abs(rec - S[i[both], j[both]]).max() <= 4 * DC.EPS * np.abs(S).max()
    err, zeros = DC.entry_error(c, ref, var, P, pv)
    print("%s: exact answer through the comparison: %.2e of %.2e" % (name, err, ref["tol"]))
    assert zeros and err < ref["tol"]


@pytest.mark.parametrize("name", ["forest-193-f3", "rank_one-256", "band6-193"])
def test_one_wrong_entry_fails_the_comparison(name):
    c, ref = case_of(name)
    f, n = c["f"], c["n"]
    nu = n - f
    Ss = np.abs(c["S"] * ref["sq"][:, None] * ref["sq"][None, :])
    ti, tj = np.arange(nu)[:, None] // 64, np.arange(nu)[None, :] // 64
    Ss[ti == tj] = 0                                  # an entry of a tile off the diagonal
    # The LARGEST such entry: the norm is relative to the largest entry of the scaled inverse, so this shows that an error
    # of 1e-9 of that size is caught anywhere off the diagonal tiles -- not that every entry is held to 1e-9 of its own
    # size: an entry far below smax moved by 1e-9 relative lies within the bound by construction of the norm.
    i, j = np.unravel_index(np.argmax(Ss), Ss.shape)
    assert i // 64 != j // 64 and c["S"][i, j] != 0
    wrong = np.array(c["S"])
    wrong[i, j] = wrong[j, i] = wrong[i, j] * (1 + DC.LD(1e-9))
    for P in (DC.all_pairs(n), np.array([[f + i, f + j]], dtype=np.int32)):   # among all pairs, and on its own
        var, pv = DC.outputs_from(wrong, f, P)
        err, zeros = DC.entry_error(c, ref, var, P, pv)
        print("%s: entry (%d, %d) moved by 1e-9: %.2e against %.2e" % (name, i, j, err, ref["tol"]))
        assert zeros and err > ref["tol"]
    # ... and a marginal moved by as much fails too
    wrong = np.array(c["S"])
    wrong[i, i] *= 1 + DC.LD(1e-9)
    var, pv = DC.outputs_from(wrong, f, np.zeros((0, 2), dtype=np.int32))
    assert DC.entry_error(c, ref, var, np.zeros((0, 2), dtype=np.int32), pv)[0] > ref["tol"]


def test_seam_rows_and_sampled_pairs():
    assert DC.seam_rows(65).tolist() == [0, 31, 32, 63, 64]
    r = DC.seam_rows(2048)
    assert 2047 in r and 0 in r and 1023 in r and 1024 in r and len(r) == 128
    c = DC.forest(1025, 1)
    P = DC.sample_pairs(c, 100)
    s = DC.seam_rows(1025)
    assert len(P) == 100 + len(s) ** 2 and P.min() >= 0 and P.max() < c["n"] and 1024 in s
