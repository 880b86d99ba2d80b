"""What test_gpu_l1decode.py relies on, shown from the reference alone (the C oracle and its NumPy twin; no device).

The GPU test compares the handle's primal-dual decoder (irotavg_amd/csrc/l1pd.hip) with the oracle at pdmaxiter up to
8 on the cases of l1pd_cases.py. That comparison means something only where the reference itself is pinned: its two
restatements (sparse Cholesky, SuperLU) agree, every iteration accepts its first trial (a second trial is decided by
rounding once the Hessian weights spread over 1e7 and more), and a linear solver that merely meets pcg_rtol moves the
answer by much less than the tolerance the GPU test derives from it. It also states the gap the GPU test closes: with
pdmaxiter <= 2, all the suite ran before, the fu bounds and the unclamped step almost never decide a step.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import l1pd_cases as LC  # noqa: E402
from irotavg_amd import synth  # noqa: E402
from oracle import np_twin as T  # noqa: E402
from oracle import oracle as O  # noqa: E402

RUNS = [(name, c, p) for name in LC.SMALL for c in range(3) for p in LC.PDITERS]
RUNS += [("pcg2600", c, p) for c in range(3) for p in LC.PDITERS_PCG]


@pytest.mark.parametrize("name,coord,pdmaxiter", RUNS, ids=["%s-c%d-p%d" % r for r in RUNS])
def test_reference_is_pinned(name, coord, pdmaxiter):
    rc, xo, stuck = LC.oracle_decode(name, coord, pdmaxiter)
    tw = LC.twin(name, coord, pdmaxiter)
    assert rc == 0 and stuck == 0 and not tw["stuck"]
    d_ref = np.abs(tw["x"] - xo).max() / np.abs(xo).max()
    print("%s c%d pdmaxiter %d: d_ref %.2e, amp %.2e, bounds %s, last spread %.1e"
          % (name, coord, pdmaxiter, d_ref, tw["amp"], [t["bound"] for t in tw["trace"]], tw["trace"][-1]["spread"]))
    assert d_ref <= 1e-10
    assert len(tw["trace"]) == pdmaxiter                     # sdg never fell below PDTOL: every iteration ran
    assert [t["trials"] for t in tw["trace"]] == [1] * pdmaxiter
    assert 0.0 < tw["amp"] and 10 * tw["amp"] <= 1e-6
    assert LC.amp(name, coord, pdmaxiter) == tw["amp"]


def test_trace_and_solve_leave_the_answer_alone():
    """The two optional arguments of np_twin.l1decode_pd: bitwise the same x with and without a trace, and with the
    default solve passed in by hand."""
    import scipy.sparse.linalg as sla
    c = LC.case("odd65")
    A, H = T.make_A(c["n"], c["f"], c["I"]), T._H_builder(c["n"], c["f"], c["I"])
    y = LC.y_of(c, 2)
    x0, s0 = T.l1decode_pd(A, H, y, 8)
    tr = []
    x1, s1 = T.l1decode_pd(A, H, y, 8, trace=tr)
    x2, s2 = T.l1decode_pd(A, H, y, 8, solve=lambda Hm, b: sla.splu(Hm).solve(b))
    assert x0.tobytes() == x1.tobytes() == x2.tobytes() and s0 == s1 == s2
    assert len(tr) == 8 and set(tr[0]) == {"bound", "trials", "sdg", "spread"}
    assert all(t["bound"] in ("l1", "l2", "f1", "f2", "one") for t in tr)
    assert all(a["sdg"] > b["sdg"] > 0 for a, b in zip(tr, tr[1:]))   # the surrogate duality gap falls


def bounds_of(name, upto):
    return [t["bound"] for c in range(3) for t in LC.twin(name, c, 8)["trace"][:upto]]


@pytest.mark.parametrize("name", LC.SMALL)
def test_every_guarded_bound_decides_a_step(name):
    got = bounds_of(name, 8)
    assert len(got) == 24
    print(name, {b: got.count(b) for b in ("l1", "l2", "f1", "f2", "one")})
    assert {"l1", "l2", "f1", "f2"} <= set(got)


def test_the_unclamped_step_is_taken_somewhere():
    assert any("one" in bounds_of(name, 8) for name in LC.SMALL)


def test_two_iterations_almost_never_reach_the_fu_bounds():
    """The gap: at pdmaxiter <= 2 the step is decided by a lamu bound in all but at most 1 step in 12."""
    got = [b for name in LC.SMALL for b in bounds_of(name, 2)]
    late = [b for b in got if b in ("f1", "f2", "one")]
    print("pdmaxiter <= 2: %d of %d steps decided by an fu bound or unclamped" % (len(late), len(got)))
    assert len(got) == 24 and 12 * len(late) <= len(got)


@pytest.mark.parametrize("name", list(LC.TABLE))
def test_rows_of_A(name):
    c = LC.case(name)
    n, m, p_loop, f, scale, rev, seed = LC.TABLE[name]
    assert (c["n"], c["m"], c["f"]) == (n, m, f)
    zero, one = LC.row_counts(c)
    want_zero, want_one = LC.ROWS[name]
    assert zero == want_zero and (want_one is None or one == want_one)
    # the oracle's make_A is the twin's
    np.testing.assert_array_equal(O.make_A(n, f, c["I"]).toarray(), T.make_A(n, f, c["I"]).toarray())
    # a reversed edge is the same measurement: the residual only changes sign
    if rev:
        S = synth.make_graph(n, m, p_loop, seed=seed, p_band_out=0.05)
        r0 = np.asarray(O.log_map(O.delta_rel(S["I"], S["QQ"], c["Q0"])))[:, :3] * scale
        k = np.arange(0, m, rev)
        np.testing.assert_allclose(c["Y"][k], -r0[k], rtol=0, atol=1e-15)
        keep = np.setdiff1d(np.arange(m), k)
        np.testing.assert_array_equal(c["Y"][keep], r0[keep])


def test_shapes_are_the_ones_the_kernels_can_get_wrong():
    assert LC.case("band129")["m"] % 2 == 0 and LC.case("band129")["m"] % 64 != 0
    assert LC.case("odd65")["m"] % 2 == 1 and LC.case("small200f2")["m"] % 2 == 1
    assert int(LC.case("band129")["is_loop"].sum()) == 0 and int(LC.case("loops129f3")["is_loop"].sum()) == 50
    assert LC.case("odd65")["n"] - LC.case("odd65")["f"] == 64                    # one slice of 64 rows exactly
    assert LC.case("pcg2600")["n"] - 1 > 2048                                      # above mg_dense_max
    assert np.abs(LC.case("small200f2")["Y"]).max() < 4e-3                        # small residuals
    p = LC.planar(12)
    assert p["n"] - p["f"] <= 16 and p["m"] <= 64                                  # fits the wave-resident window kernel


@pytest.mark.parametrize("n,m", [(40, 114), (12, 30)])
def test_planar_cases(n, m):
    c = LC.planar(n)
    assert c["m"] == m
    Y = c["Y"]
    assert (Y[:, 0] == 0).all() and (Y[:, 1] == 0).all() and np.abs(Y[:, 2]).max() > 0.01  # (0 on the spanning tree's edges)
    a = O.l1ra(c["QQ"], c["I"], c["Q0"], 1, 5, 1e-3)
    assert a["rc"] == -3 and a["iters"] == 0 and a["Q"].tobytes() == O.fmat(c["Q0"]).tobytes()
    b = O.irls(c["QQ"], c["I"], c["Q0"], 1, 4, LC.SIG, 30, 1e-3)
    assert b["rc"] == 0 and b["iters"] > 0
    # off the plane the case is an ordinary one
    Qp = LC.perturbed(c["Q0"], 1, 0.05, 11)
    assert np.abs(np.asarray(O.log_map(O.delta_rel(c["I"], c["QQ"], Qp)))[:, :3]).max(axis=0).min() > 0.01
    assert O.l1ra(c["QQ"], c["I"], Qp, 1, 3, 1e-3)["rc"] == 0
