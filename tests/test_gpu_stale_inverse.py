"""The first iterates of the multigrid-preconditioned CG on a RE-USED and on a REPAIRED coarse inverse (dense.hip:
dense_is_stale, k_value_ratio, dense_lowrank_repair and its k_wb_* kernels; the dense apply and k_cg_apply of cgcg.hip
that read dense_scale) against the chained NumPy reference of tests/stale_cases.py (checked on the CPU by
test_stale_cases_cpu.py). The method of test_gpu_pcg_iterates.py, applied to what that module leaves out.

Why iterates. A stale inverse costs PCG iterations, never accuracy: a repair with the wrong sign of delta, a wrong c, a
reference operator that is not rewritten, a slice mapped to the wrong rows or a scale from the wrong min / max all leave
a roughly SPD preconditioner, and the converged solution does not move. x_1 = alpha_0 M^-1 b does, by 1e-3 .. 1e-1
(stale_cases.MUTANTS; the bar sits eight orders below).

Which iterate g.X holds. pcg_max_iters = k cannot cut a solve on a non-fresh handle: ERR_NOT_CONVERGED on a re-used
inverse makes ls_solve re-invert and solve again (solver.hip: failed() && !g.dense_fresh). The tolerance cuts it instead:
pcg_check sets FL_DONE at the first iterate whose three column residuals are all <= pcg_rtol ||b||, every kernel enqueued
after that returns at once, pcg_iters_last = FL_ITERS, the code is OK and no retry runs. pcg_rtol is the geometric mean of
the largest column residual of the long-double iterate k and the smallest such value over the earlier iterates, both at
least a factor 1.25 away (asserted on the CPU; the one (case, k) that misses it, k = 3 of the four-level family, is not
used). The earlier solves of the handle run under the same tolerance: they only establish the inverse. The first test
checks the mechanism alone, on a fresh handle and without any reference: the X read this way equals the X of
pcg_check_every = pcg_max_iters = k bit for bit, on one case per kernel family.

Every case asserts, after every solve of its chain, the code OK and dense_inversions / dense_repairs as the chain of
verdicts predicts; for the solve under test pcg_iters_last == k, pcg_stagnated == pcg_handed_over == 0, the hierarchy the
reference was built for, and

    ratio = (max|X - x_k^ld| / max|x_k^ld|) / max(e_ref(k), nu 2^-52) < 16

with x_k^ld from the exact inverse (long double) of the operator the inverse belongs to and e_ref from the float64 chain of
the device's update formula. For an "invert" verdict that operator is the new one: a fresh reference.

Measured on one MI355X: ratio by case, solve and k (bar 16; "-": the (case, k) whose tolerance misses the margin).
The e_ref columns are those of that machine's host: e_ref is the float64 NumPy chain's own error and moves with the
host's LAPACK (repair-769-r3 at k = 1: 1.87e-13 there, 3.75e-13 on another host; scale-add2far-1025: 5.12e-14 and
4.50e-14). Wherever e_ref is below the floor nu 2^-52 -- every row here -- the ratio does not depend on it.

    case                        solve verdict pairs    k=1    k=2    k=3    e_ref at k = 1, 2, 3
    scale-mult2-513                 1 scale      0    0.36   0.38   0.32    2.43e-14 3.33e-14 1.46e-14
    scale-mult2-513                 2 scale      0    0.35   0.39   0.38    1.78e-14 1.74e-14 2.11e-14
    scale-mult3-519                 1 scale      0    0.05   0.05   0.05    7.71e-15 5.42e-15 5.66e-15
    scale-mult3-519                 2 scale      0    0.03   0.03   0.04    1.41e-14 1.31e-14 9.03e-15
    scale-add2far-1025              1 scale      0    0.10   0.09   0.19    5.12e-14 5.01e-14 2.43e-14
    scale-add2far-1025              2 scale      0    0.09   0.17   0.15    4.62e-14 7.43e-14 6.04e-14
    scale-add2loop-513              1 scale      0    0.07   0.06   0.05    1.04e-14 9.29e-15 6.25e-15
    scale-add2loop-513              2 scale      0    0.07   0.06   0.05    7.68e-15 7.63e-15 6.80e-15
    scale-l1f-1025                  1 scale      0    0.04   0.05   0.07    5.95e-15 2.11e-14 2.09e-14
    scale-l1f-1025                  2 scale      0    0.04   0.08   0.06    2.51e-14 1.50e-14 1.77e-14
    scale-cg2-1025                  1 scale      0    0.03   0.03   0.03    5.95e-15 2.11e-14 2.09e-14
    scale-cg2-1025                  2 scale      0    0.03   0.03   0.05    2.51e-14 1.50e-14 1.77e-14
    scale-cg2-1537-4lev             1 scale      0    0.02   0.06      -    1.08e-14 1.62e-14        -
    scale-cg2-1537-4lev             2 scale      0    0.03   0.04      -    2.89e-14 3.92e-14        -
    repair-65-r1                    1 repair     1    0.08   0.09   0.09    3.18e-14 4.06e-14 3.70e-14
    repair-129-r3-shared-row        1 repair     3    0.18   0.23   0.17    5.14e-14 3.04e-14 2.33e-14
    repair-193-r17                  1 repair    17    0.22   0.14   0.20    4.73e-14 6.94e-14 6.72e-14
    repair-193-r64                  1 repair    64    0.17   0.16   0.16    5.70e-14 4.69e-14 4.84e-14
    repair-769-r3                   1 repair     3    0.56   0.62   0.29    1.87e-13 1.54e-13 1.06e-13
    repair-769-r17                  1 repair    17    0.51   0.89   0.49    1.90e-13 2.99e-13 1.75e-13
    repair-129-r2-mild              1 repair     2    0.12   0.21   0.14    4.53e-14 4.97e-14 3.51e-14
    chain-129                       1 scale      0    0.18   0.16   0.12    5.04e-14 3.20e-14 4.42e-14
    chain-129                       2 repair     2    0.18   0.13   0.10    6.46e-14 4.49e-14 3.66e-14
    chain-129                       3 scale      0    0.20   0.13   0.12    7.64e-14 4.56e-14 3.60e-14
    chain-129                       4 repair     2    0.15   0.20   0.14    6.19e-14 4.37e-14 2.35e-14
    cap-129                        12 repair     2    0.27   0.22   0.18    5.45e-14 7.10e-14 4.86e-14
    cap-129                        13 invert     0    0.17   0.16   0.22    3.44e-14 3.95e-14 3.12e-14
    invert-193-65-pairs             1 invert     0    0.10   0.08   0.08    4.55e-14 2.74e-14 2.97e-14
    invert-129-vanished             1 invert     0    0.11   0.13   0.13    4.98e-14 8.23e-14 4.71e-14
    invert-129-x200                 1 invert     0    0.14   0.13   0.10    3.30e-14 2.97e-14 2.31e-14
    invert-129-diagonal-spread      1 invert     0    0.32   0.23   0.21    1.56e-13 8.03e-14 7.24e-14

The largest, 0.89, is the 769-row last level (ndense_pad 832, 13 SELL slices, k_wb_z / k_wb_w / k_wb_apply over four
workgroups in x), whose own e_ref (3.0e-13) is at the floor; the twelfth repair in a row stays at 0.27, the float64
chain of the formula in NumPy at 0.29: no growth at the cap. The mechanism test: the tolerance and the iteration cap
return the same X to the bit (max|difference| 0) at k = 1, 2, 3 on all four kernel families. No defect found: the
candidates from reading -- sell_row_of on a last level whose slices differ in width (repair-193-r17, repair-769-*),
k_wb_ref_diag after a list that the host had to sort (64 pairs; the second repair of chain-129 reads the rewritten
operator), the dense_scale a repair leaves for the next re-use (chain-129, solve 3) -- all compute what the reference does.
"""
import numpy as np
import pytest

import pcg_cases as PC
import stale_cases as SC
from irotavg_amd import capi

pytestmark = pytest.mark.gpu

SOLVES = [(sc["name"], t, k) for sc in SC.CASES for t, ks in sc["tested"].items() for k in ks]   # by case: one reference
MECHANISM = [(name, k) for name in SC.MECHANISM_CASES for k in (1, 2, 3)]


def handle(c, **extra):
    assert capi.default_options().mg_omega == PC.OMEGA
    assert capi.default_options().dense_always_refresh == 0 and capi.default_options().no_lowrank_repair == 0
    if c["route"] != "default":                                                # (that family passes no mg_* option at all)
        extra = dict(extra, mg_omega=PC.OMEGA)
    G = capi.Graph(c["I"], c["QQ"], c["n"], c["f"], **c["opts"], **extra)
    G.set_rotations(c["Q0"])
    return G


def check_hierarchy(c, fs, st, named_for_route):
    levels = c["levels"]
    assert st["level_rows"] == levels, (st["level_rows"], levels)
    assert st["band_block"] == 0
    assert fs["mg_kc_x1000"] == int(round(c["kc"] * 1000)), fs
    assert fs["additive_top"] == (1 if c["additive"] else 0), fs
    assert fs["ndense"] == levels[-1] and fs["ndense_pad"] == (levels[-1] + 63) // 64 * 64, fs
    if c["route"] == "cg2":
        assert (fs["l1_fused"], fs["cg2"]) == (1, 1), fs
    elif c["route"] == "l1fused":
        assert (fs["l1_fused"], fs["cg2"]) == (1, 0), fs
    else:
        assert (fs["l1_fused"], fs["cg2"]) == (0, 0), fs
    if not named_for_route:
        return
    # a scale case is named for the launch that consumes dense_scale. solver.hip: the p-update and the SpMV are one launch
    # iff far * 32 <= sell_len / 64, with nnz <= sell_len <= 64 x (the longest row of every slice + 3)
    far = fs["l0_far_entries"]
    if c["route"] == "add2far":
        assert 0 < far and far * 32 <= st["level_nnz"][0] // 64, (fs, st["level_nnz"])
    elif c["route"] == "add2loop":
        I = c["I"].astype(np.int64) - c["f"]
        both = (I[:, 0] >= 0) & (I[:, 1] >= 0) & (I[:, 0] != I[:, 1])
        deg = np.zeros((c["nu"] + 63) // 64 * 64, dtype=np.int64)
        deg[:c["nu"]] = np.bincount(I[both].ravel(), minlength=c["nu"])
        assert far * 32 > int(64 * (deg.reshape(-1, 64).max(1) + 3).sum()) // 64, fs
    else:
        assert far == 0 and len(levels) == {"scale-mult2-513": 2, "scale-mult3-519": 3, "scale-l1f-1025": 3,
                                            "scale-cg2-1025": 3, "scale-cg2-1537-4lev": 4}[c["name"]], fs


@pytest.mark.parametrize("name,k", MECHANISM, ids=["%s-k%d" % t for t in MECHANISM])
def test_the_tolerance_stops_at_the_iterate_the_iteration_cap_stops_at(name, k):
    c = PC.CASE[name]
    rtol, holds = SC.stopping(PC.reference_pair(c)["res"], k)
    assert holds
    out = []
    for opts in (dict(pcg_check_every=k, pcg_max_iters=k), dict(pcg_rtol=rtol)):
        with handle(c, **opts) as G:
            fs = G.fingerprint_scalars()
            G.edge_residual()
            G.set_weights(c["w"])
            rc, X = G.ls_solve(allow_rc=(capi.ERR_NOT_CONVERGED,), return_rc=True)
            out.append((rc, X, G.stats()))
    (rc_a, Xa, sa), (rc_b, Xb, sb) = out
    print("stale-mechanism %s k=%d: pcg_rtol %.3e, relres %.3e, codes %d / %d, iterations %d / %d, l1_fused %d, cg2 %d, "
          "max|difference| %.1e" % (name, k, rtol, max(sb["last_relres"]), rc_a, rc_b, sa["pcg_iters_last"],
                                    sb["pcg_iters_last"], fs["l1_fused"], fs["cg2"], float(np.abs(Xa - Xb).max())))
    assert rc_a == capi.ERR_NOT_CONVERGED and rc_b == capi.OK
    assert sa["pcg_iters_last"] == k and sb["pcg_iters_last"] == k
    assert sb["pcg_stagnated"] == 0 and sb["pcg_handed_over"] == 0 and sb["dense_inversions"] == 1
    assert np.array_equal(Xa, Xb)


@pytest.mark.parametrize("name,t,k", SOLVES, ids=["%s-solve%d-k%d" % s for s in SOLVES])
def test_kth_iterate_on_a_stale_inverse_matches_the_reference(name, t, k):
    sc = SC.CASE[name]
    c = sc["case"]
    ref = SC.reference(sc)
    chain = ref["chain"]
    rtol, holds = ref["solve"][t]["stop"][k - 1]
    assert holds
    with handle(c, pcg_rtol=rtol) as G:
        fs, st = G.fingerprint_scalars(), G.stats()
        check_hierarchy(c, fs, st, name.startswith("scale-"))
        assert st["dense_inversions"] == 0 and st["dense_repairs"] == 0
        G.edge_residual()
        for s in range(t + 1):
            G.set_weights(sc["weights"][s])
            rc, X = G.ls_solve(allow_rc=(capi.ERR_NOT_CONVERGED,), return_rc=True)
            st = G.stats()
            got = (rc, st["dense_inversions"], st["dense_repairs"], st["pcg_solves"])
            assert got == (capi.OK, chain[s]["inversions"], chain[s]["repairs"], s + 1), (s, chain[s]["verdict"], got)
    r = SC.ratio(sc, ref, t, k, X)
    sol = ref["solve"][t]
    print("stale-iterate %s solve %d (%s, %d pairs) k=%d: ratio %.2f (e_ref %.2e, floor %.2e), relres %.3e (reference "
          "%.3e), pcg_rtol %.3e, iterations %d, inversions %d, repairs %d"
          % (name, t, chain[t]["verdict"], len(chain[t]["pairs"]), k, r, sol["e_ref"][k - 1], c["nu"] * SC.EPS,
             max(st["last_relres"]), float(np.max(sol["res"][k - 1])), rtol, st["pcg_iters_last"], st["dense_inversions"],
             st["dense_repairs"]))
    assert st["pcg_iters_last"] == k
    assert st["pcg_stagnated"] == 0 and st["pcg_handed_over"] == 0
    assert np.isfinite(X).all()
    assert r < SC.BAR
