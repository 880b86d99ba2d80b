"""The first three iterates of the multigrid-preconditioned CG (solver.hip, cgcg.hip, dense.hip) against the NumPy
reference of tests/pcg_cases.py (checked on the CPU by test_pcg_cases_cpu.py), on every route through the kernels.

Why iterates. Every other test of this solver looks at the converged solution, and a CG iteration with a wrong but roughly
SPD preconditioner, or a wrong beta, still converges to it. x_1 = alpha_0 M^-1 b pins the whole cycle (coarse operators,
restriction, prolongation, smoothing, the dense apply), x_2 pins beta and the kernels' non-`first` variants, x_3 both
parities of the scalar ping-pong.

Which iterate g.X holds. On a fresh handle stats.pcg_iters_last == 0, so with pcg_check_every = pcg_max_iters = k the
first chunk of both host loops is k:
* pcg_solve_classic (solver.hip): update<INIT> sets x = 0 and leaves r = b; each pass of the chunk loop is precondition
  -> p-update (+ SpMV) -> update, and the update kernel does x += alpha p, r -= alpha q and FL_ITERS += 1: after the chunk
  g.X = x_k. The precondition() that follows only tests convergence (FL_DONE stays 0: the residual is ~1e-2); the loop
  reaches `it >= maxit` with it = k and breaks BEFORE iteration_tail: g.X is still x_k, FL_ITERS = k.
* pcg_solve_cg2 (cgcg.hip): k_cg_update<0> sets x = 0, r = b; each pass is apply (u = M^-1 r, w = L u, the partials of
  gamma = r.u and delta = u.w) -> update<1 or 2> (beta = gamma / gamma_old, alpha = gamma / (delta - beta gamma / alpha_old),
  p = u + beta p, s = w + beta s, x += alpha p, r -= alpha s, FL_ITERS += 1). In exact arithmetic delta - beta gamma /
  alpha_old = p.Lp, so these are the textbook iterates: g.X = x_k after the chunk, the trailing apply() changes neither x
  nor r, and `it >= maxit` (k < kCg2GiveUp = 400: no hand-over) breaks before the next update.
Both return IROTAVG_ERR_NOT_CONVERGED. ls_solve()'s retry block then (1) re-inverts only `if (... && !g.dense_fresh)` --
the first assembly of a handle always refreshes, dense_fresh is true -- and (2) calls assemble_values (matrix values and
the right-hand side, not g.X) and dense_direct_solve, which returns false at once unless the handle is ONE dense level
(dense.hip: `g.levels.size() != 1`). Every case here has two to four levels, so g.X is left alone, and
irotavg_graph_ls_solve copies it out whatever the code. Each case asserts the code, pcg_iters_last == k,
pcg_stagnated == 0 and pcg_handed_over == 0, and from fingerprint_scalars() / stats() that it ran the route it is named for.

The comparison is pcg_cases.ratio: (max|X - x_k^ld| / max|x_k^ld|) / max(e_ref(k), nu 2^-52) < 16, the hierarchy's shape
and kc read back from the handle. The second test runs the largest well-conditioned case of every route to pcg_rtol: the
reference PCG's iteration count +- 1, and numpy.linalg.solve to 1e-8.

Two defects these tests found, fixed in the same change.
1. The level cap ends the hierarchy without a dense level and no kernel of the cycle is left to carry the convergence
   prologue (cycle_from, solver.hip). Additive top level over a capped level 1 (mg_levels_max = 2: the cases cap-add2-*):
   the cycle was one device-to-device copy, so nothing tested convergence and nothing wrote the b1.y1 partials; the p-update
   formed r.z from r.z0 alone, alpha and beta were wrong, and the solve ran to pcg_max_iters whatever it reached. Before
   (the reference with r.z = r.z0, pcg_cases mutant "bottom_rz"; not a device run): ratio 1.7e+12 (513 views) and 8.7e+11
   (1025 views) at k = 1. Three capped levels with the level-1 down-sweep inside the update (cap-add3-1025): the iterates
   were right (ratio 0.01) but last_relres stayed 0.0 and the solve could not end before pcg_max_iters either. After
   (k_jacobi_bottom: the copy, with the prologue and the partials where they are missing): the table below, and 47, 117
   and 62 iterations to 1e-10, the reference's counts.
2. The blocked Gauss-Jordan sweep of dense.hip scaled the pivot row as a - ((p - 1) / p) a (gj_invert32_split), which
   loses log10 p digits for a pivot p > 1. The preconditioner's sweep inverts the UNSCALED coarse operator: weights over
   six decades, pivots of 4e6. add2loop-1025-spread before: ratio 1535 / 1732 / 2355 at k = 1 / 2 / 3 (error 3.5e-10,
   constant over each aggregate; 1.0e-13 with weights over two decades, 1.8e-11 over four: it grows with the pivot), and
   the same formula in NumPy gives 3974. After (the row of a pivot above 1 is formed as 0 + a / p): 0.12 / 0.20 / 0.12.
   The exact form is on for the last level of a hierarchy only: a handle that is one dense level keeps the sweep's
   arithmetic to the bit, because the referee tests of that path sit at cond x 2^-52 of that particular rounding
   (test_gpu_referee.py's near-tree case moved from below 2e-8 to 2.5e-8 with the exact form on everywhere). That path
   still has the defect; it is covered by its iterative refinement and the Cholesky fall-back.

A dead row (isolated view) inside a live aggregate is not left at 0: up_row adds kc P y to every row of the aggregate, so
z, p and x carry the aggregate's correction there. Nothing reads it back (the row and column of L are zero); the
reference does the same and the comparison covers it. A dead row that is an aggregate of its own stays exactly 0.

Out of scope: the sharded PCG (dist.hip) and inexact_outer. The stale-inverse policy (dense_scale != 1, the Woodbury
repair, the re-inversion verdicts) has this method applied to it in test_gpu_stale_inverse.py, with the chained
reference of stale_cases.py.

Measured on one MI355X: ratio by case and k (bar 16; the case names carry the route and nu, pcg_cases._cases).

    case                       k=1    k=2    k=3    e_ref at k = 1, 2, 3
    mult2-255                  0.58   0.75   0.74    3.6e-14  3.0e-14  1.8e-14
    mult2-256                  0.12   0.05   0.08    3.7e-15  5.2e-15  4.2e-15
    mult2-257-a16              0.12   0.11   0.09    8.6e-15  2.6e-15  2.5e-15
    mult3-519                  0.05   0.07   0.11    9.0e-15  4.9e-15  7.2e-15
    mult3-1025                 0.08   0.11   0.10    3.0e-14  4.8e-14  5.2e-14
    add2far-1025               0.11   0.10   0.17    5.9e-14  4.0e-14  4.7e-14
    add2far-1537               0.14   0.15   0.13    8.7e-14  7.4e-14  7.5e-14
    add2far-1025-a16           0.12   0.11   0.10    3.1e-14  2.1e-14  1.5e-14
    add2sep-1537               0.14   0.16   0.13    8.7e-14  7.4e-14  7.5e-14
    add2loop-256-a16           0.17   0.13   0.14    5.0e-15  2.5e-15  3.0e-15
    add2loop-505               0.10   0.13   0.11    1.3e-14  8.8e-15  8.3e-15
    add2loop-513               0.08   0.06   0.06    6.5e-15  1.0e-14  7.5e-15
    add2loop-1537              0.05   0.04   0.04    2.5e-14  3.8e-14  3.6e-14
    add2loop-1025-spread       0.12   0.20   0.12    2.2e-14  4.0e-14  5.0e-14
    l1f-520                    0.14   0.14   0.21    1.3e-14  1.8e-14  2.4e-14
    l1f-577                    0.08   0.09   0.16    4.4e-15  1.6e-14  4.8e-15
    l1f-1025                   0.07   0.09   0.04    1.1e-14  1.3e-14  1.4e-14
    l1f-1537-spread            0.57   0.41   0.50    4.2e-13  1.5e-12  1.1e-12
    cg2-520                    0.13   0.18   0.23    1.3e-14  1.8e-14  2.4e-14
    cg2-577                    0.08   0.08   0.08    4.4e-15  1.6e-14  4.8e-15
    cg2-1025                   0.06   0.05   0.03    1.1e-14  1.3e-14  1.4e-14
    cg2-1537-spread            0.51   0.76   0.77    4.2e-13  1.5e-12  1.1e-12
    cg2-1537-4lev              0.02   0.05   0.08    1.6e-14  2.5e-14  6.8e-14
    cap-mult2-519              0.02   0.02   0.03    1.0e-15  5.5e-16  5.7e-16
    cap-add2-513               0.02   0.01   0.02    1.7e-15  1.1e-15  7.9e-16
    cap-add2-1025-far          0.01   0.01   0.01    1.5e-15  9.6e-16  9.5e-16
    cap-add3-1025              0.01   0.01   0.01    1.4e-15  2.4e-15  1.5e-15
    default-1537               0.37   0.44   0.19    2.1e-13  1.3e-13  7.6e-14

The largest, 0.77, is a family with weights over six decades, whose own e_ref (1.5e-12) is above the floor; everywhere
the device stays within the larger of nu 2^-52 and the float64 reference's own error.
Solves to pcg_rtol = 1e-10 (second test):

    mult3-519                  14 iterations (reference   14), relres 3.68e-11, |X - solve| / |solve| = 1.47e-10
    add2far-1537               23 iterations (reference   23), relres 2.90e-11, |X - solve| / |solve| = 1.78e-10
    add2sep-1537               23 iterations (reference   23), relres 2.90e-11, |X - solve| / |solve| = 1.78e-10
    add2loop-1537              25 iterations (reference   25), relres 8.02e-11, |X - solve| / |solve| = 4.94e-10
    l1f-1025                   25 iterations (reference   25), relres 9.97e-11, |X - solve| / |solve| = 1.87e-10
    cg2-1537-4lev              35 iterations (reference   35), relres 9.19e-11, |X - solve| / |solve| = 5.45e-10
    cap-add2-1025-far         117 iterations (reference  117), relres 3.87e-11, |X - solve| / |solve| = 7.19e-11
    default-1537               24 iterations (reference   24), relres 4.21e-11, |X - solve| / |solve| = 1.18e-10
    cap-add2-513               47 iterations (reference   47), relres 2.82e-11, |X - solve| / |solve| = 5.04e-11
    cap-add3-1025              62 iterations (reference   62), relres 7.61e-11, |X - solve| / |solve| = 2.47e-10
"""
import numpy as np
import pytest

import pcg_cases as PC
from irotavg_amd import capi

pytestmark = pytest.mark.gpu

ITERATE_CASES = [(c["name"], k) for c in PC.CASES for k in (1, 2, 3)]          # by case: its reference is computed once


def solve(G):
    """(return code, X) of irotavg_graph_ls_solve."""
    return G.ls_solve(allow_rc=(capi.ERR_NOT_CONVERGED,), return_rc=True)


def sell_len_bound(c):
    """An upper bound of level 0's SELL length: every slice as wide as its longest row (one entry per edge end), + 3."""
    I = c["I"].astype(np.int64) - c["f"]
    both = (I[:, 0] >= 0) & (I[:, 1] >= 0) & (I[:, 0] != I[:, 1])
    deg = np.bincount(I[both].ravel(), minlength=c["nu"])
    pad = np.zeros((c["nu"] + 63) // 64 * 64, dtype=np.int64)
    pad[:c["nu"]] = deg
    return int(64 * (pad.reshape(-1, 64).max(1) + 3).sum())


def check_route(c, fs, st, pair):
    """The handle took the route the case is named for (and the hierarchy the reference was built for)."""
    route, o = c["route"], c["opts"]
    levels = st["level_rows"]
    assert levels == c["levels"], (levels, c["levels"])
    assert st["band_block"] == 0
    assert fs["additive_top"] == (1 if c["additive"] else 0), fs
    assert fs["mg_kc_x1000"] == int(round(c["kc"] * 1000)), fs
    assert fs["ndense"] == (levels[-1] if c["dense"] else 0), fs
    assert (fs["l0_far_entries"] > 0) == c["far"], fs
    if c["dense"]:
        Lc = pair["r64"].L[-1]
        i, j = np.nonzero(Lc)
        assert fs["dense_bw"] == int(np.abs(i - j).max()), fs
        assert fs["ndense_pad"] == (levels[-1] + 63) // 64 * 64
    far, nnz0 = fs["l0_far_entries"], st["level_nnz"][0]
    if route == "mult":
        assert (fs["l1_fused"], fs["cg2"]) == (0, 0) and len(levels) in (2, 3), fs
    elif route in ("add2far", "add2sep", "default"):
        # solver.hip: fused p-update + SpMV iff far * 32 <= sell_len / 64 and no_fused_pspmv != 1 (sell_len >= nnz)
        assert len(levels) == 2 and (fs["l1_fused"], fs["cg2"]) == (0, 0) and far * 32 <= nnz0 // 64, (fs, nnz0)
        assert o.get("no_fused_pspmv", 0) == (1 if route == "add2sep" else 0)
        if route == "default":
            assert fs["mg_dense_max"] == 1100 and not any(k.startswith("mg_") for k in o), (fs, o)
    elif route == "add2loop":
        assert len(levels) == 2 and (fs["l1_fused"], fs["cg2"]) == (0, 0) and far * 32 > sell_len_bound(c) // 64, fs
    elif route == "l1fused":
        assert len(levels) == 3 and (fs["l1_fused"], fs["cg2"]) == (1, 0), fs
    elif route == "cg2":
        assert len(levels) in (3, 4) and (fs["l1_fused"], fs["cg2"]) == (1, 1), fs
    elif route == "cap":
        assert fs["ndense"] == 0 and fs["cg2"] == 0 and len(levels) == o["mg_levels_max"], fs
    else:
        raise AssertionError(route)


def handle(c, **extra):
    assert capi.default_options().mg_omega == PC.OMEGA
    if c["route"] != "default":                                                # (that family passes no mg_* option at all)
        extra = dict(extra, mg_omega=PC.OMEGA)
    G = capi.Graph(c["I"], c["QQ"], c["n"], c["f"], **c["opts"], **extra)
    G.set_rotations(c["Q0"])
    return G


@pytest.mark.parametrize("name,k", ITERATE_CASES, ids=["%s-k%d" % t for t in ITERATE_CASES])
def test_kth_iterate_matches_the_reference(name, k):
    c = PC.CASE[name]
    with handle(c, pcg_check_every=k, pcg_max_iters=k) as G:
        fs, st0 = G.fingerprint_scalars(), G.stats()
        assert st0["pcg_iters_last"] == 0 and st0["pcg_solves"] == 0           # fresh: the first chunk is pcg_check_every
        pair = PC.reference_pair(c, levels=st0["level_rows"], kc=fs["mg_kc_x1000"] / 1000.0,
                                 additive=fs["additive_top"] == 1)
        check_route(c, fs, st0, pair)
        G.edge_residual()
        G.set_weights(c["w"])
        rc, X = solve(G)
        st = G.stats()
    r = PC.ratio(c, pair, k, X)
    print("pcg-iterate %s k=%d: ratio %.2f (e_ref %.2e, floor %.2e), relres %.2e (reference %.2e), levels %s, kc %.1f, "
          "far %d, dense_bw %d" % (name, k, r, pair["e_ref"][k - 1], c["nu"] * PC.EPS, max(st["last_relres"]),
                                   float(pair["res"][k - 1].max()), st["level_rows"], fs["mg_kc_x1000"] / 1000.0,
                                   fs["l0_far_entries"], fs["dense_bw"]))
    assert rc == capi.ERR_NOT_CONVERGED
    assert st["pcg_iters_last"] == k and st["pcg_solves"] == 1
    assert st["pcg_stagnated"] == 0 and st["pcg_handed_over"] == 0
    assert st["dense_inversions"] == (1 if c["dense"] else 0)                  # one fresh inverse, no retry
    assert np.isfinite(X).all()
    # the convergence prologue ran after the k-th update and saw the residual of x_k (1e-3: it only has to be that one)
    assert abs(max(st["last_relres"]) - float(pair["res"][k - 1].max())) <= 1e-3 * float(pair["res"][k - 1].max())
    if c["isolated"] is not None and c["isolated"] == c["nu"] - 1 and c["isolated"] % c["aggs"][0] == 0:
        assert np.all(X[c["isolated"]] == 0)
    assert r < PC.BAR


def _largest(route):
    ok = [c for c in PC.CASES if c["route"] == route and c["isolated"] is None and not c["spread"]]
    return max(ok, key=lambda c: c["nu"])["name"]


SOLVE_CASES = [_largest(r) for r in ("mult", "add2far", "add2sep", "add2loop", "l1fused", "cg2", "cap", "default")]
SOLVE_CASES += ["cap-add2-513", "cap-add3-1025"]          # each capped hierarchy whose bottom carries the prologue itself


@pytest.mark.parametrize("name", SOLVE_CASES)
def test_solve_takes_the_reference_iteration_count(name):
    c = PC.CASE[name]
    rtol = capi.default_options().pcg_rtol
    with handle(c, pcg_rtol=rtol) as G:
        fs, st0 = G.fingerprint_scalars(), G.stats()
        pair = PC.reference_pair(c, levels=st0["level_rows"], kc=fs["mg_kc_x1000"] / 1000.0,
                                 additive=fs["additive_top"] == 1)
        check_route(c, fs, st0, pair)
        G.edge_residual()
        G.set_weights(c["w"])
        rc, X = solve(G)
        st = G.stats()
    ref = pair["r64"]
    Xr, res = ref.pcg(rtol=rtol)
    Xs = np.linalg.solve(ref.L[0], ref.b)
    err = float(np.abs(X - Xs).max() / np.abs(Xs).max())
    print("pcg-solve %s: %d iterations (reference %d), relres %.2e, |X - solve| / |solve| = %.2e"
          % (name, st["pcg_iters_last"], len(Xr), max(st["last_relres"]), err))
    assert rc == capi.OK and st["pcg_stagnated"] == 0 and st["pcg_handed_over"] == 0
    assert abs(st["pcg_iters_last"] - len(Xr)) <= 1
    assert max(st["last_relres"]) <= rtol
    assert err < 1e-8
