"""The chained reference of stale_cases.py checked on the CPU, and what its bar can see. No GPU.

* every case takes the chain of verdicts it is named for, with the number of deviating pairs it states, and the float64
  and the long-double chain agree on it (stale_cases._reference asserts that);
* the float64 formula chain agrees with the long-double exact chain at every tested solve and k: e_ref, the yardstick
  of the GPU test, stays below BAR x nu 2^-52 (printed next to the floor), as the sibling test_pcg_cases_cpu.py asks;
* the stopping tolerance of every (case, solve, k) the GPU test uses lies a factor 1.25 from both residuals it separates,
  and every solve keeps at least two of k = 1, 2, 3; the same for the fresh-handle cases of the mechanism test;
* every defect of stale_cases.MUTANTS, applied to the float64 chain alone, exceeds the bar by at least 100 x on every
  case it is tried on, at some k (printed: the factor over the bar), with the chain of verdicts unchanged: the defect
  acts inside the repair or the scale (but for the one that keeps the old reference operator, which changes what the
  next step is compared with).
"""
import numpy as np
import pytest

import pcg_cases as PC
import stale_cases as SC

NAMES = [c["name"] for c in SC.CASES]


def test_stale_step_verdicts_on_a_small_operator():
    """The rules one by one, on a 4 x 4 operator."""
    E = np.array([[4.0, -1, 0, -1], [-1, 4, -1, 0], [0, -1, 4, -1], [-1, 0, -1, 4]])
    s = SC.stale_step(E, 3 * E, 0)
    assert s["verdict"] == "scale" and abs(s["factor"] - 1 / 3) < 1e-15 and np.array_equal(s["E_after"], E)
    N = 2 * E
    N[0, 3] = N[3, 0] = -2 * 5.0                               # one pair moved by x5 on top of the common factor 2
    s = SC.stale_step(E, N, 0)
    assert s["verdict"] == "repair" and s["factor"] == 2.0 and s["pairs"] == [(0, 3, -8.0)]
    A = s["E_after"]
    assert A[0, 3] == A[3, 0] == -10.0 and A[0, 0] == A[3, 3] == 16.0 and A[1, 1] == 8.0 and A[0, 1] == -2.0
    assert SC.stale_step(E, N, SC.WB_REPAIRS_MAX)["verdict"] == "invert"                 # the thirteenth in a row
    V = N.copy()
    V[0, 3] = V[3, 0] = 0.0
    assert SC.stale_step(E, V, 0)["verdict"] == "invert"                                  # an entry vanished
    V[0, 3] = V[3, 0] = -2 * 2e4
    assert SC.stale_step(E, V, 0)["verdict"] == "invert"                                  # beyond four decades
    D = 2 * E
    D[0, 0] *= 1.2
    assert SC.stale_step(E, D, 0)["verdict"] == "invert"                                  # the diagonal spreads
    W = SC.woodbury(np.linalg.inv(E), s["factor"], s["pairs"])
    assert np.abs(W @ A - np.eye(4)).max() < 1e-14                                        # the formula inverts E_after


@pytest.mark.parametrize("name", NAMES)
def test_verdicts_chains_and_stopping_tolerances(name):
    sc = SC.CASE[name]
    ref = SC.reference(sc)
    got = [s["verdict"] for s in ref["chain"]]
    print("stale-ref %s: verdicts %s, pairs %s, factors %s" % (name, got, [len(s["pairs"]) for s in ref["chain"]],
                                                               ["%.4g" % float(s["factor"]) for s in ref["chain"]]))
    assert got == sc["verdicts"]
    for s in ref["chain"]:
        if s["verdict"] == "repair":
            assert len(s["pairs"]) == sc["pairs"]
    floor = sc["case"]["nu"] * SC.EPS
    for t, ks in sc["tested"].items():
        s = ref["solve"][t]
        assert len(ks) >= 2
        for k in (1, 2, 3):
            r = SC.ratio(sc, ref, t, k, s["X64"][k - 1])
            rtol, holds = s["stop"][k - 1]
            print("stale-ref %s solve %d (%s) k=%d: e_ref %.2e, floor %.2e, ratio of the fp64 chain %.2f, relres %.3e, "
                  "pcg_rtol %.3e, margin %s%s" % (name, t, sc["verdicts"][t], k, s["e_ref"][k - 1], floor, r,
                                                 float(np.max(s["res"][k - 1])), rtol, "holds" if holds else "MISSED",
                                                 "" if k in ks else " (k not used)"))
            assert np.isfinite(s["X64"][k - 1]).all()
            assert r < SC.BAR
            assert s["e_ref"][k - 1] < SC.BAR * floor         # the yardstick is of the order of the floor
            if k in ks:
                assert holds


@pytest.mark.parametrize("name", SC.MECHANISM_CASES)
def test_stopping_tolerances_of_the_mechanism_cases(name):
    res = PC.reference_pair(PC.CASE[name])["res"]
    for k in (1, 2, 3):
        rtol, holds = SC.stopping(res, k)
        print("stale-mechanism %s k=%d: relres %.3e, pcg_rtol %.3e" % (name, k, float(np.max(res[k - 1])), rtol))
        assert holds


MUTANT_RUNS = [(m, n) for n in NAMES for m in SC.MUTANTS if n in SC.MUTANT_CASES[m]]      # by case: one reference


@pytest.mark.parametrize("mutant,name", MUTANT_RUNS)
def test_mutant_of_the_chain_clears_the_bar(mutant, name):
    sc = SC.CASE[name]
    ref = SC.reference(sc)
    with np.errstate(all="ignore"):
        chain = SC.run_chain(sc, np.float64, False, mutant=mutant)
    if mutant != "ref_kept":
        assert [s["verdict"] for s in chain] == sc["verdicts"]
    worst = 0.0
    for t, ks in sc["tested"].items():
        for k in ks:
            r = SC.ratio(sc, ref, t, k, chain[t]["X"][k - 1])
            print("stale-mutant %s %s solve %d k=%d: ratio %.3e = %.3g x the bar (verdict %s)"
                  % (mutant, name, t, k, r, r / SC.BAR, chain[t]["verdict"]))
            worst = max(worst, r)
    assert worst >= 100 * SC.BAR


def test_every_mutant_is_tried():
    assert set(SC.MUTANT_CASES) == set(SC.MUTANTS)
    assert all(n in SC.CASE for names in SC.MUTANT_CASES.values() for n in names)
