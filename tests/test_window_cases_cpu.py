"""The cases of tests/window_cases.py, checked from the reference alone (CPU oracle + its NumPy twin): what the GPU
test of the window kernels (test_gpu_window_limits.py) relies on must hold before a device is involved.

Branches of the 14 robust weights (ral/l1_irls.cpp:617-727) and the planted edge that hits each -- the table
window_cases.BRANCHES, asserted complete in test_planted_edges_hit_every_branch:

    cost  name            branches
    0     L2              keeps_previous
    1     L1              cap (w > 1e4), below_cap
    2     L1.5            cap, below_cap
    3     L0.5            cap, below_cap
    4     Geman-McClure   formula
    5     Huber           inlier_keeps_previous (e < 1), outlier (e >= 1)
    6     pseudo-Huber    formula
    7     Andrews         e_ge_pi (-> 0 -> floor), e_lt_1e-4 (-> 1), floor_below_pi (w < 1e-4), formula
    8     Bisquare        floor (w < 1e-4), formula
    9     Cauchy          formula
    10    Fair            formula
    11    Logistic        e_lt_1e-4 (-> 1), formula
    12    Talwar          inside (1.0001), outside (0)
    13    Welsch          floor (w < 1e-4), formula
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import window_cases as WC  # noqa: E402
from irotavg_amd import capi, synth  # noqa: E402
from oracle import np_twin as T  # noqa: E402
from oracle import oracle as O  # noqa: E402

SIG = WC.SIG
LIMITS = WC.limits()


def test_branch_table_names_every_cost():
    assert sorted(WC.BRANCHES) == list(range(14))
    for cost, names in WC.BRANCHES.items():
        assert len(set(names)) == len(names) >= 1


@pytest.mark.parametrize("cost", range(14))
def test_planted_edges_hit_every_branch(cost):
    c = WC.planted(cost)
    assert c["nv"] - c["f"] <= 16 and len(c["I"]) <= 64 and c["f"] >= 2       # fits the wave kernel as well
    np.testing.assert_array_equal(c["Q0"][:c["f"]], np.tile([0, 0, 0, 1.0], (c["f"], 1)))
    assert (c["I"][c["planted"]] < c["f"]).all()                                # planted = fixed-fixed
    E, w = WC.planted_reference(c, cost)
    e = np.linalg.norm(E, axis=1)                                               # e2 = theta^2
    np.testing.assert_allclose(e[c["direct"]], c["theta"][c["direct"]], rtol=1e-14, atol=0)
    np.testing.assert_allclose(e[~c["direct"]], c["theta"][~c["direct"]], rtol=0, atol=2e-15)   # through the wrap
    assert (~c["direct"]).any() and c["theta"][~c["direct"]].min() >= 0.05
    hit = WC.classify(cost, SIG, E)
    assert set(hit) == set(WC.BRANCHES[cost]), (cost, sorted(set(WC.BRANCHES[cost]) - set(hit)))
    # the classification and np_twin's weights are one statement: constant branches carry their constant
    for b, wk in zip(hit, w):
        if b in WC.CONST_VALUE:
            assert wk == WC.CONST_VALUE[b], (cost, b, wk)
        else:
            assert wk not in (1e4, 1e-4, 1.0001, 0.0), (cost, b, wk)
    if cost == 5:                                                               # an inlier stays exactly 1.0
        assert (w[np.array(hit) == "inlier_keeps_previous"] == 1.0).all()


@pytest.mark.parametrize("cost", range(14))
def test_pairs_land_on_different_sides(cost):
    c = WC.planted(cost)
    E, w = WC.planted_reference(c, cost)
    hit = WC.classify(cost, SIG, E)
    pos = {int(k): n for n, k in enumerate(c["planted"])}
    want_pairs = {1: 1, 2: 1, 3: 1, 5: 1, 7: 2, 8: 1, 11: 1, 12: 1, 13: 1}.get(cost, 0)
    assert len(c["pairs"]) == want_pairs
    for name, (a, b) in c["pairs"].items():
        assert w[pos[a]] != w[pos[b]], (cost, name)
        assert hit[pos[a]] != hit[pos[b]], (cost, name)


@pytest.mark.parametrize("cost", range(14))
def test_oracle_one_pass_gives_the_planted_weights(cost):
    """oracle.irls(max_iters = 1) = np_twin.weights_update(E = -r) on the planted edges: the linear solve has no say."""
    c = WC.planted(cost)
    _, w = WC.planted_reference(c, cost)
    b = O.irls(c["QQ"], c["I"], c["Q0"], c["f"], cost, SIG, 1, 1e-3)
    assert b["rc"] == 0 and b["iters"] == 1
    np.testing.assert_allclose(b["weights"][c["planted"]], w, rtol=1e-13, atol=0)
    tw = T.irls(c["QQ"], c["I"], c["Q0"], c["f"], cost, SIG, 1, 1e-3)
    np.testing.assert_allclose(b["weights"], tw["weights"], rtol=1e-9, atol=0)
    assert synth.angular_distance(b["Q"], tw["Q"]).max() < 1e-12


def test_star_is_the_residual_of_each_edge():
    s = WC.star()
    nu = s["nv"] - s["f"]
    assert nu <= 16 and len(s["I"]) <= 64 and len(s["I"]) == nu
    b = O.irls(s["QQ"], s["I"], s["Q0"], s["f"], 4, SIG, 1, 1e-3)
    assert b["rc"] == 0 and b["iters"] == 1
    r = T.log_map(T.delta_rel(s["I"], s["QQ"], s["Q0"]))[:, :3]
    X = r.copy()
    X[s["rows"]["quirk"] - 1] = 0                                   # its row is dropped: nothing moves the view
    want = T.quat_mult(s["Q0"][1:], T.exp_map(np.concatenate([X, np.zeros((nu, 1))], axis=1)))
    np.testing.assert_allclose(b["Q"][1:], want, rtol=0, atol=1e-15)
    for v in s["unchanged"]:
        np.testing.assert_array_equal(b["Q"][v], s["Q0"][v])
    np.testing.assert_array_equal(b["Q"][0], s["Q0"][0])
    # exactly pi wraps to -pi: r = (+pi, 0, 0), and the sign shows in the output rotation
    k = s["rows"]["exactly_pi"]
    assert r[k - 1, 0] == np.pi and b["Q"][k, 0] == 1.0
    assert (r[s["rows"]["identity"] - 1] == 0).all() and (r[s["rows"]["below_eps"] - 1] == 0).all()
    assert np.abs(r[s["rows"]["tiny_above_eps"] - 1, 0]) > 0


@pytest.mark.parametrize("name,wave,c", LIMITS, ids=[l[0] for l in LIMITS])
def test_limit_case_is_exact_and_well_posed(name, wave, c):
    nu, nv, ne = c["nu"], c["nv"], c["ne"]
    assert name.endswith("%d-%d-%d" % (nu, nv, ne))
    assert (len(c["Q0"]), len(c["Q0"]) - c["f"], len(c["I"]), len(c["QQ"])) == (nv, nu, ne, ne)
    assert c["I"].min() >= 0 and c["I"].max() == nv - 1
    assert wave == (nu <= 16 and ne <= 64)
    deg = WC.informative_degree(c)
    assert deg.min() >= min(3, ne // nu), deg.min()                 # 3 wherever ne allows it
    if ne >= 3 * nu and nu > 1:
        assert deg.min() >= 3
    A = T.make_A(nv, c["f"], c["I"]).toarray()                      # (the oracle's make_A keeps the reference's assert
                                                                    # n - f > 1; its drivers take one free view)
    np.testing.assert_array_equal(np.abs(A).sum(axis=0), deg)
    cond = np.linalg.cond(A.T @ A)
    assert cond <= 1e4, cond
    a = O.l1ra(c["QQ"], c["I"], c["Q0"], c["f"], 100, 1e-3)
    b = O.irls(c["QQ"], c["I"], a["Q"], c["f"], 4, SIG, 100, 1e-3)
    assert (a["rc"], b["rc"]) == (0, 0)
    assert np.isfinite(b["Q"]).all() and np.isfinite(b["weights"]).all()
    assert 0 < a["iters"] < 100 and 0 < b["iters"] < 100            # converged, not capped


def test_limit_cases_are_the_stated_sizes():
    got = [(c["nu"], c["nv"], c["ne"]) for _, _, c in LIMITS]
    assert got == [(64, 320, 640), (64, 65, 640), (64, 320, 64), (1, 320, 640), (1, 2, 1),
                   (16, 320, 64), (16, 17, 64), (1, 320, 64)]
    c = LIMITS[0][2]
    free = (c["I"] >= c["f"])
    assert (~free[:, 0] & ~free[:, 1]).sum() > 50 and (free[:, 0] & ~free[:, 1]).sum() > 50   # both kinds of filler


PAST = WC.past_limits()


@pytest.mark.parametrize("name,kernel,c", PAST, ids=[p[0] for p in PAST])
def test_one_past_each_limit_is_refused_before_any_device(name, kernel, c):
    """ERR_BAD_ARG, not ERR_NO_DEVICE, on a machine without a GPU: the sizes are refused before a device is asked
    for, so no kernel can have been launched; nothing of the caller's is written."""
    rc, Q, before, w, its = WC.raw_window_solve(c, kernel)
    assert rc == capi.ERR_BAD_ARG
    assert Q.tobytes() == before.tobytes()
    assert (w == -7.0).all() and its == (-1, -1)
