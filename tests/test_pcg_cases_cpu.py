"""The reference of pcg_cases.py checked on the CPU, and what its bar can see. No GPU.

* the float64 and the long-double reference agree within the bar at every case and k (printed: e_ref next to the floor
  nu 2^-52 of the comparison);
* the reference preconditioner is symmetric positive definite, in both top modes and for kc = 1.0, 1.6, 2.0 (build.cpp:
  "SPD for every kc > 0");
* the reference PCG run to 1e-10 reproduces numpy.linalg.solve(L0, b) within 1e-8 (the tolerance of test_gpu_parity.py,
  for its weights uniform(0.1, 5); the family with weights over six decades is held to ||r|| / lambda_min instead);
* every defect of pcg_cases.MUTANTS, applied to the float64 reference alone, moves the first iterate (the second for the
  two that act from the second iteration on) by at least 100 x the bar on every case it can act on.

One mutant of the list cannot be seen by ANY right-hand side the handle forms: a dead row's inverse diagonal set to 1
instead of 0. A dead row has neither matrix entries nor a right-hand side (b = A' w^2 r has no term for a view without
edges), so its residual is exactly 0 on every level and 1 x 0 = 0 x 0. What the clamp `d > 0 ? 1 / d : 0` protects
against is 1 / 0 = inf and inf x 0 = NaN; that mutant ("dead_idg_unclamped") is the one checked here, and the GPU test
asserts finite iterates, with exact zeros on a dead row that is an aggregate of its own.
"""
import numpy as np
import pytest

import pcg_cases as PC

NAMES = [c["name"] for c in PC.CASES]
LIVE = [c["name"] for c in PC.CASES if c["isolated"] is None]


@pytest.mark.parametrize("name", NAMES)
def test_float64_and_long_double_references_agree(name):
    c = PC.CASE[name]
    pair = PC.reference_pair(c)
    floor = c["nu"] * PC.EPS
    for k in (1, 2, 3):
        r = PC.ratio(c, pair, k, pair["X64"][k - 1])
        print("pcg-ref %s k=%d: e_ref %.2e, floor %.2e, ratio of the fp64 reference %.2f, relres %.2e"
              % (name, k, pair["e_ref"][k - 1], floor, r, float(pair["res"][k - 1].max())))
        assert np.isfinite(pair["X64"][k - 1]).all() and np.isfinite(np.asarray(pair["Xld"][k - 1], dtype=float)).all()
        assert r < PC.BAR
        assert pair["e_ref"][k - 1] < PC.BAR * floor          # the floor is of the order of the reference's own error
    # a dead row that is an aggregate of its own stays at 0; one inside a live aggregate receives that aggregate's
    # prolonged correction in z (up_row adds kc P y to every row), which nothing reads back: its row and column are zero
    for d in pair["r64"].dead_rows:
        alone = d % c["aggs"][0] == 0 and d == c["nu"] - 1
        assert all(np.all(x[d] == 0) == alone for x in pair["X64"])


SPD_CASES = ["mult2-255", "mult3-519", "add2loop-505", "l1f-520", "cap-mult2-519", "cap-add2-513"]


@pytest.mark.parametrize("kc", [1.0, 1.6, 2.0])
@pytest.mark.parametrize("additive", [False, True], ids=["multiplicative", "additive"])
@pytest.mark.parametrize("name", SPD_CASES)
def test_reference_preconditioner_is_spd(name, additive, kc):
    c = PC.CASE[name]
    assert c["nu"] <= 600 and c["isolated"] is None
    M = PC.Reference(c, np.float64, kc=kc, additive=additive).matrix()
    asym = np.abs(M - M.T).max() / np.abs(M).max()
    lam = np.linalg.eigvalsh((M + M.T) / 2)
    print("pcg-spd %s %s kc=%.1f: asymmetry %.2e, eigenvalues %.3e ... %.3e"
          % (name, "additive" if additive else "multiplicative", kc, asym, lam[0], lam[-1]))
    assert asym <= 1e-13
    assert lam[0] > 0


@pytest.mark.parametrize("name", LIVE)
def test_reference_pcg_converges_to_the_solution(name):
    c = PC.CASE[name]
    ref = PC.reference_pair(c)["r64"]
    X, res = ref.pcg(rtol=1e-10)
    Xs = np.linalg.solve(ref.L[0], ref.b)
    err = np.abs(X[-1] - Xs).max() / np.abs(Xs).max()
    print("pcg-solve %s: %d iterations, relres %.2e, |x - solve| / |solve| = %.2e" % (name, len(X), res[-1].max(), err))
    assert res[-1].max() <= 1e-10
    if not c["spread"]:
        assert err < 1e-8
    else:
        # weights over six decades: cond(L0) ~ 1e10 and a residual of 1e-10 ||b|| no longer promises 1e-8 in x; what it
        # promises is ||x - x*|| <= ||r|| / lambda_min, column by column
        lam = np.linalg.eigvalsh(ref.L[0])[0]
        bound = res[-1] * np.linalg.norm(ref.b, axis=0) / lam
        e2 = np.linalg.norm(X[-1] - Xs, axis=0)
        print("pcg-solve %s: lambda_min %.3e, ||x - solve|| / bound = %s" % (name, lam, e2 / bound))
        assert lam > 0 and np.all(e2 <= bound)


def applies(mutant, case, ref):
    """Can this defect change an iterate of this case at all?"""
    last_row_dead = case["isolated"] == case["nu"] - 1
    if mutant == "post_omega":
        return ref.has_post_smoothing()
    if mutant == "short_aggregate":               # (a short aggregate made of the dead row restricts a zero anyway)
        return ref.has_short_aggregate() and not last_row_dead
    if mutant == "coarse_value":                  # the Jacobi sweep of a level-1 bottom reads its diagonal only
        return case["dense"] or len(ref.L) > 2
    if mutant == "dead_idg_unclamped":
        return case["isolated"] is not None
    if mutant == "bottom_rz":                     # the defect test_gpu_pcg_iterates.py found in cycle_from
        return ref.additive and len(ref.L) == 2 and not case["dense"]
    return mutant != "dead_idg_one"


# by case: the reference is cached. The family with the build's own choices has a last level of 769 rows, seconds per
# reference: it gets the two mutants that need none of the case's special shapes
MUTANT_CASES = [(m, n) for n in NAMES for m in (PC.MUTANTS if n != "default-1537" else ("kc", "beta_zero"))]


@pytest.mark.parametrize("mutant,name", MUTANT_CASES)
def test_mutant_of_the_reference_clears_the_bar(mutant, name):
    c = PC.CASE[name]
    pair = PC.reference_pair(c)
    k = 2 if mutant in ("beta_zero", "parity") else 1
    with np.errstate(all="ignore"):
        X, _ = PC.Reference(c, np.float64, mutant=mutant).pcg(k)
    r = PC.ratio(c, pair, k, X[k - 1])
    on = applies(mutant, c, pair["r64"])
    print("pcg-mutant %s %s k=%d: ratio %.3e (%s)" % (mutant, name, k, r, "acts" if on else "cannot act"))
    if mutant == "dead_idg_one":
        assert r < PC.BAR                         # unobservable: see the module docstring
    elif mutant == "dead_idg_unclamped" and on:
        assert not np.isfinite(X[k - 1]).all()
    elif on:
        assert r >= 100 * PC.BAR
    else:
        assert r < PC.BAR                         # ... and where it cannot act the reference is unchanged


def test_every_mutant_acts_on_some_case_of_every_route_it_can_reach():
    acts = {m: set() for m in PC.MUTANTS}
    for c in PC.CASES:
        ref = PC.reference_pair(c)["r64"] if c["name"] != "default-1537" else None
        for m in PC.MUTANTS:
            if ref is not None and applies(m, c, ref):
                acts[m].add(c["route"])
    routes = {c["route"] for c in PC.CASES} - {"default"}
    for m in ("kc", "coarse_excess", "beta_zero", "parity", "short_aggregate"):
        assert acts[m] == routes, (m, routes - acts[m])
    assert acts["post_omega"] == {"mult", "l1fused", "cg2", "cap"}      # two additive levels have no post-smoothing
    assert acts["coarse_value"] == routes
    assert acts["dead_idg_unclamped"] == {"mult", "l1fused", "cg2"}
    assert acts["bottom_rz"] == {"cap"}
