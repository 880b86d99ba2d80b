"""The window kernels (irotavg_amd/csrc/window.hip) at their size limits and in every branch of their per-edge math.

The log map (edge_log), the 14 robust weights (robust_weight), the exp map of a step (step_quat) and the edge flags
(edge_flags) are one function each (kernels.hpp, common.hpp), inlined into both window kernels and into the kernels of
the handle: these tests guard the single copy through every path that inlines it. The primal-dual LP and the dense solve
are the window kernels' own. test_gpu_window.py compares whole pipelines on small random graphs, which reach neither the
limits (64 free views, 320 views, 640 edges; 16 / 64 for the wave kernel) nor the branches. The cases come from
tests/window_cases.py; what they rely on is asserted from the reference alone in test_window_cases_cpu.py.

kernel = 1 is the general LDS kernel, 2 the wave-resident kernel, 0 the automatic choice.
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

pytestmark = pytest.mark.gpu
SIG = WC.SIG
LIMITS = WC.limits()
PAST = WC.past_limits()


def one_pass(c, cost, kernel):
    """l1_iters = 0, irls_iters = 1: residual, unit-weight solve, weight update, step."""
    return capi.window_solve(c["I"], c["QQ"], c["Q0"], c["f"], cost, SIG, 0, 1, 1e-3, kernel=kernel)


def check_planted(w, c, cost, what):
    """weights of the planted edges against np_twin: rtol 1e-11 (the bar of test_weight_update_every_cost), the
    constants of the formula bit for bit. Each figure is printed before it is asserted (run with -s).

    The one planted weight that amplifies rounding is Andrews' at e = pi (1 - 1e-6): d ln w / d ln e = e cot(e) / 2 =
    -5e5, so one ulp of the angle (2.2e-16) moves it by 1.1e-10 relative. The reference's own two restatements agree
    there because they share one libm; a device atan2 that differs from it by an ulp at that input would show as
    ~1e-10 here. If that happens the finding is this edge's conditioning, not a wrong constant: a wrong constant moves
    the weight by > 1e-4."""
    E, ref = WC.planted_reference(c, cost)
    hit = WC.classify(cost, SIG, E)
    got = w[c["planted"]]
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    print("%s cost %d: planted max rel diff %.3e (at theta = %.17g)" % (what, cost, rel.max(), c["theta"][rel.argmax()]))
    for k, (b, g, r) in enumerate(zip(hit, got, ref)):
        if b in WC.CONST_VALUE:
            assert g == r == WC.CONST_VALUE[b], (what, cost, b, c["theta"][k], g, r)
    np.testing.assert_allclose(got, ref, rtol=1e-11, atol=0, err_msg="%s cost %d %s" % (what, cost, hit))


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("cost", range(14))
def test_planted_branches(cost, kernel):
    c = WC.planted(cost)
    r = one_pass(c, cost, kernel)
    check_planted(r["weights"], c, cost, "kernel %d" % kernel)
    b = O.irls(c["QQ"], c["I"], c["Q0"], c["f"], cost, SIG, 1, 1e-3)
    assert b["rc"] == 0
    assert (r["l1_iters"], r["irls_iters"]) == (0, b["iters"]) == (0, 1)
    ang = synth.angular_distance(r["Q"], b["Q"]).max()
    print("kernel %d cost %d: max angular diff vs oracle %.3e rad" % (kernel, cost, ang))
    assert ang < 1e-9
    np.testing.assert_allclose(r["weights"], b["weights"], rtol=1e-7)
    np.testing.assert_array_equal(r["Q"][:c["f"]], c["Q0"][:c["f"]])


@pytest.mark.parametrize("cost", range(14))
def test_planted_kernels_agree(cost):
    """Both kernels inline the same edge_log and robust_weight: the same expressions on the same residual."""
    c = WC.planted(cost)
    g, w = one_pass(c, cost, 1), one_pass(c, cost, 2)
    print("planted cost %d, kernel 1 vs kernel 2: max diff of the planted weights %.3e"
          % (cost, np.abs(w["weights"][c["planted"]] - g["weights"][c["planted"]]).max()))
    np.testing.assert_allclose(w["weights"][c["planted"]], g["weights"][c["planted"]], rtol=1e-13, atol=0)


@pytest.mark.parametrize("kernel", [1, 2])
def test_star_log_and_exp_map(kernel):
    s = WC.star()
    r = one_pass(s, 4, kernel)
    b = O.irls(s["QQ"], s["I"], s["Q0"], s["f"], 4, SIG, 1, 1e-3)
    assert b["rc"] == 0 and (r["l1_iters"], r["irls_iters"]) == (0, b["iters"]) == (0, 1)
    print("kernel %d star: max componentwise diff vs oracle %.3e" % (kernel, np.abs(r["Q"] - b["Q"]).max()))
    for name, v in s["rows"].items():
        # componentwise, not the sign-invariant angle: the wrap at pi shows as the sign of the row
        np.testing.assert_allclose(r["Q"][v], b["Q"][v], rtol=0, atol=1e-14, err_msg=name)
    for v in s["unchanged"]:
        assert r["Q"][v].tobytes() == s["Q0"][v].tobytes(), v
    assert r["Q"][:s["f"]].tobytes() == s["Q0"][:s["f"]].tobytes()
    np.testing.assert_allclose(r["weights"], b["weights"], rtol=1e-7)


def test_star_kernels_agree():
    """At unit weights the star's normal matrix is the identity: both kernels apply the same residual (edge_log) through
    the same exp map (step_quat), so the rotations of the planted rows are compared componentwise between them."""
    s = WC.star()
    g, w = one_pass(s, 4, 1), one_pass(s, 4, 2)
    rows = list(s["rows"].values())
    print("star, kernel 1 vs kernel 2: max componentwise diff %.3e" % np.abs(g["Q"][rows] - w["Q"][rows]).max())
    for name, v in s["rows"].items():
        np.testing.assert_allclose(w["Q"][v], g["Q"][v], rtol=1e-13, atol=0, err_msg=name)


def pipeline_vs_oracle(c, kernel, cost=4, l1=100, irls=100, ang_tol=1e-9, w_tol=dict(rtol=1e-7)):
    r = capi.window_solve(c["I"], c["QQ"], c["Q0"], c["f"], cost, SIG, l1, irls, 1e-3, kernel=kernel)
    a = O.l1ra(c["QQ"], c["I"], c["Q0"], c["f"], l1, 1e-3)
    b = O.irls(c["QQ"], c["I"], a["Q"], c["f"], cost, SIG, irls, 1e-3)
    assert (a["rc"], b["rc"]) == (0, 0)
    ang = synth.angular_distance(r["Q"], b["Q"]).max()
    print("kernel %d cost %d (nu %d, nv %d, ne %d): iters %d/%d (oracle %d/%d), max angular diff %.3e rad"
          % (kernel, cost, c["nu"], c["nv"], c["ne"], r["l1_iters"], r["irls_iters"], a["iters"], b["iters"], ang))
    assert (r["l1_iters"], r["irls_iters"]) == (a["iters"], b["iters"])
    assert ang < ang_tol
    np.testing.assert_allclose(r["weights"], b["weights"], **w_tol)
    np.testing.assert_array_equal(r["Q"][:c["f"]], c["Q0"][:c["f"]])
    return r


LIMIT_RUNS = [(name, c, k) for name, wave, c in LIMITS for k in ((1, 2) if wave else (1,))]


@pytest.mark.parametrize("name,c,kernel", LIMIT_RUNS, ids=["%s-k%d" % (n, k) for n, _, k in LIMIT_RUNS])
def test_limits_pipeline_matches_oracle(name, c, kernel):
    """The bars of test_window_pipeline_matches_oracle, at the largest sizes the kernels accept."""
    pipeline_vs_oracle(c, kernel)


WAVE_CASES = [(name, c) for name, wave, c in LIMITS if wave]


@pytest.mark.parametrize("name,c", WAVE_CASES, ids=[n for n, _ in WAVE_CASES])
def test_limits_automatic_choice_is_the_wave_kernel(name, c):
    auto = capi.window_solve(c["I"], c["QQ"], c["Q0"], c["f"], 4, SIG, 100, 100, 1e-3, kernel=0)
    w = capi.window_solve(c["I"], c["QQ"], c["Q0"], c["f"], 4, SIG, 100, 100, 1e-3, kernel=2)
    assert (auto["l1_iters"], auto["irls_iters"]) == (w["l1_iters"], w["irls_iters"])
    assert auto["Q"].tobytes() == w["Q"].tobytes() and auto["weights"].tobytes() == w["weights"].tobytes()


@pytest.mark.parametrize("cost", [13, 1])
def test_limits_floor_and_cap_costs_at_full_size(cost):
    """Welsch (a floor) and L1 (a cap) on the (64, 320, 640) case, at the bars of test_window_every_cost."""
    name, _, c = LIMITS[0]
    assert (c["nu"], c["nv"], c["ne"]) == (64, 320, 640)
    pipeline_vs_oracle(c, 1, cost=cost, l1=3, irls=12, ang_tol=1e-8, w_tol=dict(rtol=1e-6, atol=1e-12))


@pytest.mark.parametrize("name,kernel,c", PAST, ids=[p[0] for p in PAST])
def test_one_past_each_limit_is_refused(name, kernel, c):
    """ERR_BAD_ARG with the caller's Q bitwise unchanged. That no kernel runs on these paths is what the CPU twin of
    this test shows: the same calls are refused on a machine that has no device to launch on."""
    rc, Q, before, w, its = WC.raw_window_solve(c, kernel)
    assert rc == capi.ERR_BAD_ARG
    assert Q.tobytes() == before.tobytes()
    assert (w == -7.0).all() and its == (-1, -1)
    if len(c["I"]) and c["f"] < c["nv"]:
        with pytest.raises(capi.IrotavgError) as e:
            capi.window_solve(c["I"], c["QQ"], c["Q0"], c["f"], kernel=kernel)
        assert e.value.code == capi.ERR_BAD_ARG


def test_largest_accepted_next_to_the_refused():
    """The raw call itself works at the limit: the refusals above are the size checks, not the calling convention."""
    rc, Q, before, w, its = WC.raw_window_solve(LIMITS[0][2], 0)
    assert rc == 0 and its[0] > 0 and its[1] > 0 and (w != -7.0).all()
    assert Q.tobytes() != before.tobytes()


@pytest.mark.parametrize("cost", range(14))
def test_planted_table_through_the_handle(cost):
    """The same planted table through the handle's kernels: the stage entry points, then the fused weight pass of
    irls. One robust_weight (kernels.hpp), reached through three kernels, held to one table."""
    c = WC.planted(cost)
    with capi.Graph(c["I"], c["QQ"], c["nv"], c["f"]) as G:
        G.set_rotations(c["Q0"])
        G.set_weights(np.ones(len(c["I"])))
        G.edge_residual()
        G.ls_solve()
        G.update_weights(cost, SIG)
        check_planted(G.get_weights(), c, cost, "handle stages")
    with capi.Graph(c["I"], c["QQ"], c["nv"], c["f"]) as G:
        G.set_rotations(c["Q0"])
        it = G.irls(cost, SIG, 1, 1e-3)
        assert it["iters"] == 1
        check_planted(G.get_weights(), c, cost, "handle irls")
