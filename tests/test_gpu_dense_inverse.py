"""Entries of the blocked Gauss-Jordan inverse (irotavg_amd/csrc/dense.hip) against exact answers, at every edge of its
blocking. The cases and the comparison are tests/dense_cases.py (checked on the CPU by test_dense_cases_cpu.py).

1. dense_invert_spd through Graph.rotation_variance (marginals.hip's dense route, nu <= 2048): var = S_vv,
   pair_var = S_ii + S_jj - 2 S_ij, so every entry of S = M^-1 is recovered from three outputs. Sizes: one tile and the
   two-launch path (padded size 64), the smallest look-ahead sweep (128), odd and even tile counts, the limit 2048, and
   free-view counts that leave 32-row blocks partly or wholly identity padding. Bound: the error over all marginals and
   recovered entries, on the Jacobi-scaled inverse relative to its largest entry, stays below
   8 x max(e_ref, nu 2^-52), e_ref = the error of numpy's LAPACK inverse of the same scaled fp64 matrix.
2. nu = 2049: the dense route ends, a forest is no view sequence, the handle answers pairs through its PCG and refuses
   marginals (include/irotavg_hip.h).
3. dense_refresh -- the preconditioner's copy of the launch sequence -- and k_band_inverse<1..4>, which replaces it on a
   banded level: single-level handles, where the inverse of the whole operator is the preconditioner, so the solve must
   give S b and the PCG has nothing left to do.

Every test prints its figures before it asserts (run with -s). In part 3 the level's size and half-bandwidth are read back
from the handle (Graph.fingerprint_scalars), so the run with the switch unset is known to be one that dense_refresh hands
to k_band_inverse<bw> (bw <= 4).

Measured on one MI355X. Part 1: ratio = error / max(e_ref, nu 2^-52); the test fails at 8.

    forest    nu     1     2    31    32    33    63    64    65    96   127   128   129   192   193   256
              f=1  0.06  0.21  0.51  1.21  0.81  0.53  1.13  1.40  0.91  1.83  1.13  1.40  0.89  1.11  0.54
              f=3  0.25  0.37  0.71  2.92  0.93  0.35  0.38  0.61  0.47  0.80  0.83  1.22  0.40  1.17  0.39
              nu  1023  1025  2047  2048
              f=1  0.71  1.44  0.45  0.23
              f=3  0.20  1.16  0.58  0.52
    rank_one  nu    33    64    65   128   129   256
              f=1  0.27  0.51  0.52  0.45  0.52  1.03
    band6     nu    63   129   193
              f=2  0.34  0.42  0.36

The largest, 2.92 (forest, 32 free views, 3 fixed: error 4.4e-14 against e_ref 1.5e-14), is a sweep of one 32-row block
next to a block of pure padding; everywhere the sweep's error stays within three times the larger of nu 2^-52 and the
error of LAPACK's pivoted inverse of the same matrix. e_ref itself runs from 0 (nu = 1) over 1e-14 (nu ~ 100) to 2.7e-13 (nu = 2047).
Part 2 (2049 free views, 28 pairs through the PCG): largest |pair_var - exact| = 7e-6 of the bound
pcg_rtol ||u||^2 / lambda_min(M) (1 / lambda_min = 1.07e4); largest relative error 3.7e-13.
Part 3: PCG iterations of the solve, banded kernel / Gauss-Jordan sweep: 2 / 2 in every one of the 30 cases
(nu = 33, 64, 65, 129, 193, 2048 x half-bandwidth 1 ... 5; with half-bandwidth 5 both runs are the sweep). The device's
test at 1e-15 ends the solve at the first poll. |X - S b| / |S b|, largest of the two runs, by half-bandwidth 1 ... 5:

    nu =   33   1.4e-12  5.4e-14  5.8e-14  1.3e-14  8.4e-15
    nu =   64   8.1e-12  3.4e-13  4.7e-13  3.1e-14  2.0e-14
    nu =   65   6.6e-12  2.8e-13  2.1e-13  3.2e-14  9.8e-15
    nu =  129   8.2e-12  6.1e-13  7.6e-13  4.5e-14  4.9e-14
    nu =  193   3.4e-11  3.1e-12  2.3e-13  3.1e-13  9.4e-14
    nu = 2048   6.7e-10  8.2e-11  2.2e-11  4.7e-12  3.4e-12

(bar: 1e-9; the chain of 2048 views, half-bandwidth 1, has cond(M) ~ 1e7 and comes within a factor 1.5 of it).
"""
import numpy as np
import pytest

import dense_cases as DC
from irotavg_amd import capi
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# Reference points of the comparison, from test_dense_cases_cpu.py (fp64, no device): the exact answers give ratios of
# 0.001 ... 0.02, one entry of an off-diagonal tile moved by 1e-9 of the largest entry gives 3000 ... 10000.

FOREST_NU = [1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 192, 193, 256, 1023, 1025, 2047, 2048]
ENTRY_CASES = ([("forest", nu, f) for nu in FOREST_NU for f in (1, 3)] +
               [("rank_one", nu, 1) for nu in (33, 64, 65, 128, 129, 256)] +
               [("band6", nu, 2) for nu in (63, 129, 193)])


def entry_case(family, nu, f):
    c = DC.forest(nu, f) if family == "forest" else DC.rank_one(nu) if family == "rank_one" else DC.band(nu, 6, f)
    assert c["f"] == f and c["n"] == nu + f
    P = DC.all_pairs(c["n"]) if nu <= 256 else DC.sample_pairs(c, 20000)
    return c, DC.scaled_reference(c), P


def handle(c, **opts):
    G = capi.Graph(c["I"], c["QQ"], c["n"], c["f"], **opts)
    G.set_rotations(c["Q0"])
    return G


# ---- 1. entries of the sweep -------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,nu,f", ENTRY_CASES, ids=["%s-%d-f%d" % t for t in ENTRY_CASES])
def test_entries_of_the_inverse(family, nu, f):
    c, ref, P = entry_case(family, nu, f)
    with handle(c) as G:
        G.set_weights(c["d"])
        before = G.stats()["pcg_solves"]
        r = G.rotation_variance(pairs=P, marginals=True)
        r2 = G.rotation_variance(pairs=P, marginals=True)
        after = G.stats()["pcg_solves"]
    err, zeros = DC.entry_error(c, ref, r["var"], P, r["pair_var"])
    print("dense-entries %s nu=%d f=%d pairs=%d: err %.3e, e_ref %.3e, bound %.3e, ratio %.2f"
          % (family, nu, f, len(P), err, ref["e_ref"], ref["tol"], err / (ref["tol"] / DC.FACTOR)))
    assert zeros
    assert err < ref["tol"]
    assert before == after
    np.testing.assert_array_equal(r["var"], r2["var"])
    np.testing.assert_array_equal(r["pair_var"], r2["pair_var"])


# ---- 2. one view past the limit ----------------------------------------------------------------------------------
def test_2049_free_views_leave_the_dense_route():
    c = DC.forest(2049, 1)
    f, S = c["f"], c["S"]
    rows = DC.seam_rows(2049)[-4:]                                    # 2015 ... 2048: the last seams and the row past them
    rng = np.random.default_rng(2049)
    P = np.concatenate([rng.integers(0, c["n"], size=(18, 2)), [[0, 0], [f + 7, f + 7], [0, f + 2048], [f + 2048, 0]],
                        [[f + a, f + b] for a in rows for b in rows if a < b]]).astype(np.int32)
    rtol = capi.default_options().pcg_rtol                            # passed on explicitly: the bound below rests on it
    assert rtol > 0
    with handle(c, pcg_rtol=rtol) as G:
        st = G.stats()
        assert st["band_block"] == 0 and st["levels"] >= 2, st            # neither dense nor a view sequence: PCG
        G.set_weights(c["d"])
        rv = G.rotation_variance(P, marginals=True, allow_rc=(capi.ERR_UNSUPPORTED,))
        assert rv["rc"] == capi.ERR_UNSUPPORTED
        assert np.isnan(rv["var"]).all() and np.isnan(rv["pair_var"]).all() and np.isnan(rv["scale"])
        r = G.rotation_variance(P, marginals=False)
        assert r["var"] is None
        assert G.stats()["pcg_solves"] == 0                            # the pairs ran on a clone of the solver
    _, exact = DC.outputs_from(S, f, P)
    # u'x with M x = u solved to ||r|| <= pcg_rtol ||u||: |u'S r| <= ||S||_2 pcg_rtol ||u||^2
    lam = float(np.linalg.eigvalsh(DC.normal_matrix(c))[0])
    u2 = (P[:, 0] >= f).astype(float) + (P[:, 1] >= f).astype(float)
    bound = rtol * u2 / lam
    err = np.abs(r["pair_var"] - exact)
    live = P[:, 0] != P[:, 1]
    print("dense-limit nu=2049: max |pair_var - exact| / bound = %.3e, largest relative error %.3e, 1 / lambda_min %.3e"
          % ((err[live] / bound[live]).max(), (err[live] / exact[live]).max(), 1 / lam))
    assert np.all(r["pair_var"][~live] == 0)
    assert np.all(err[live] <= bound[live])


# ---- 3. the preconditioner's copy of the sweep, and the banded kernel that replaces it ------------------------------
REFRESH_CASES = [(nu, bw) for nu in (33, 64, 65, 129, 193, 2048) for bw in (1, 2, 3, 4, 5)]


@pytest.mark.parametrize("nu,bw", REFRESH_CASES)
def test_single_level_solve_is_the_exact_inverse_times_b(nu, bw, monkeypatch):
    c = DC.band(nu, bw, inverse=False)
    n, f, I, d = c["n"], c["f"], c["I"], c["d"]
    ro = O.log_map(O.delta_rel(I, c["QQ"], c["Q0"]))[:, :3]
    b = O.make_A(n, f, I).T @ ((d * d)[:, None] * ro)
    Xe = DC.band_solve(c, b)
    iters = {}
    for name, env in (("band", None), ("gj", "1")):
        if env:
            monkeypatch.setenv("IROTAVG_NO_BAND_INVERSE", env)
        else:
            monkeypatch.delenv("IROTAVG_NO_BAND_INVERSE", raising=False)
        with handle(c) as G:                                           # the switch is read when the handle is made
            fs = G.fingerprint_scalars()
            assert (fs["ndense"], fs["ndense_pad"], fs["dense_bw"]) == (nu, (nu + 63) // 64 * 64, bw), fs
            G.edge_residual()
            G.set_weights(d)
            X = G.ls_solve()
            st = G.stats()
        err = float(np.abs(X - Xe).max() / np.abs(Xe).max())
        iters[name] = st["pcg_iters_last"]
        print("dense-refresh nu=%d bw=%d %s: |X - S b| / |S b| = %.3e, pcg iterations %d, inversions %d"
              % (nu, bw, name, err, st["pcg_iters_last"], st["dense_inversions"]))
        assert st["levels"] == 1 and st["dense_inversions"] >= 1 and st["band_block"] == 0, st
        assert st["pcg_solves"] == 1
        assert err < 1e-9
    assert iters["band"] <= iters["gj"] + 1, iters
    # With an exact inverse the first iteration already leaves a residual at rounding level. The solver polls first after
    # two iterations; if the device's own test at 1e-15 has not ended the solve there, the host needs one more iteration to
    # see that the residual no longer halves: 3. Two more are allowed for a residual that still halves by chance at rounding
    # level. A wrong entry in dense_refresh's copy of the sweep makes every iteration contract by that error only.
    assert iters["gj"] <= 5 and iters["band"] <= 5, iters
