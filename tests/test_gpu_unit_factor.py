"""The banded direct solver keeps the factor of the UNIT-WEIGHT operator (bcr.hip, BcrUnit). `irls` starts from weights of
one (ral/l1_irls.cpp:577), so the first linear system of every call has the unweighted Laplacian of the handle's graph as
its operator: only the right-hand side changes from call to call. The first such solve of a handle is the full reduction
with the A-operands of its matrix-core products stored (D_i^-1, P, Q per eliminated block, a private W); every later one
is a pass over the right-hand sides alone -- one column tile of each product, the stored bits as operands, the same K
order, the same subtractions -- and must return, BIT FOR BIT, what the full solve returns.

Protocol: on ONE handle two irls calls from different rotations (the first stores, the second is served from the store),
held against the same two calls on a fresh handle under IROTAVG_BCR_NO_UNIT_FACTOR=1: iteration counts, score traces,
rotations and weights bitwise. `direct_info()` says whether a store exists and how many solves it served; block size and
level count are asserted so that no case passes by silently taking the full path.
"""
import os

import numpy as np
import pytest

from irotavg_amd import capi, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
SIG = 5 * np.pi / 180
SWITCH = "IROTAVG_BCR_NO_UNIT_FACTOR"


def mst_init(I, QQ, Qgt, n, f=1):
    Q = np.zeros((n, 4)); Q[:, 3] = 1; Q[:f] = Qgt[:f]
    rc, Qm = O.init_mst(Q, QQ, I, f)
    assert rc == 0
    return Qm


def second_start(Qa, f, seed=99):
    """Qa times qexp(N(0, 0.05^2)) on the free views: another right-hand side for the same operator"""
    rng = np.random.default_rng(seed)
    Qb = Qa.copy()
    Qb[f:] = synth.qmul(Qa[f:], synth.qexp(0.05 * rng.standard_normal((len(Qa) - f, 3))))
    return Qb


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def play(I, QQ, n, f, steps, off=False, env=()):
    """The steps on one fresh handle; a record per step. ("irls", Q, max_iters) sets the rotations first."""
    if off:
        os.environ[SWITCH] = "1"
    for k in env:
        os.environ[k] = "1"
    try:
        with capi.Graph(I, QQ, n, f, band_direct=1) as G:
            recs = [dict(info=G.direct_info())]
            for s in steps:
                r = dict(op=s[0])
                if s[0] == "irls":
                    G.set_rotations(s[1])
                    b = G.irls(4, SIG, s[2], 1e-3)
                    r.update(iters=b["iters"], scores=np.asarray(b["scores"])[:b["iters"]], Q=G.get_rotations(),
                             w=G.get_weights())
                    if len(s) > 3:
                        r["resid"] = G.direct_residual()
                elif s[0] == "l1ra":
                    a = G.l1ra(1, 1e-3)
                    r.update(iters=a["iters"], scores=np.asarray(a["scores"])[:a["iters"]], Q=G.get_rotations())
                elif s[0] == "time19":
                    G.time_kernel(19, 2)
                elif s[0] == "trim":
                    capi.trim_memory()
                r["info"] = G.direct_info()
                r["stats"] = G.stats()
                recs.append(r)
            return recs
    finally:
        os.environ.pop(SWITCH, None)
        for k in env:
            os.environ.pop(k, None)


def equal_records(ra, rb):
    assert len(ra) == len(rb)
    for a, b in zip(ra, rb):
        for k in ("iters",):
            if k in a:
                assert a[k] == b[k], (a["op"], a[k], b[k])
        for k in ("scores", "Q", "w", "resid"):
            if k in a:
                same_bits(a[k], b[k])
                assert np.isfinite(a[k]).all()


def two_calls(I, QQ, n, f, Qa, block, min_levels=3):
    Qb = second_start(Qa, f)
    steps = [("irls", Qa, 30), ("irls", Qb, 30)]
    on = play(I, QQ, n, f, steps)
    off = play(I, QQ, n, f, steps, off=True)
    for r in (on, off):
        assert r[0]["info"]["block"] == block and len(r[0]["info"]["levels"]) >= min_levels, r[0]["info"]
        assert r[0]["info"]["unit_factor"] == 0 and r[0]["info"]["unit_factor_solves"] == 0
        assert r[1]["iters"] >= 2 and r[2]["iters"] >= 2
        assert r[2]["stats"]["direct_solves"] == r[1]["iters"] + r[2]["iters"] and r[2]["stats"]["pcg_solves"] == 0
    assert on[1]["info"]["unit_factor"] == 1 and on[1]["info"]["unit_factor_solves"] == 0, on[1]["info"]
    assert on[1]["info"]["unit_factor_bytes"] > 0
    assert on[2]["info"]["unit_factor"] == 1 and on[2]["info"]["unit_factor_solves"] == 1, on[2]["info"]
    for r in off[1:]:
        assert r["info"]["unit_factor"] == 0 and r["info"]["unit_factor_solves"] == 0 and r["info"]["unit_factor_bytes"] == 0
    equal_records(on, off)
    assert not np.array_equal(on[1]["Q"], Qa) and not np.array_equal(on[2]["Q"], Qb)
    return on, off


_graphs = {}


def graph(n, m, seed=None):
    key = (n, m)
    if key not in _graphs:
        S = synth.make_graph(n, m, 0.0, seed=n if seed is None else seed, p_band_out=0.02)
        _graphs[key] = (S, mst_init(S["I"], S["QQ"], S["Qgt"], n))
    return _graphs[key]


# blocks of 8: three levels with a partial last chunk and slice; 16: rows no multiple of 128; 24: 209 blocks -> 27 -> 4, the
# instantiation of the headline
@pytest.mark.parametrize("n,m,block", [(4100, 3 * 4100 - 6, 8), (3001, 15 * 3001, 16), (5000, 100000, 24)])
def test_second_call_is_served_from_the_store_bitwise(n, m, block):
    S, Qa = graph(n, m)
    two_calls(S["I"], S["QQ"], n, 1, Qa, block)


def test_mixed_level_one():
    """563 chunks on 512 resident slots: the raw blocks of level 1 take their operands from the store, their right-hand
    sides from the level-0 right-hand side"""
    n, m = 36000, 4 * 36000 - 10
    S, Qa = graph(n, m, seed=12)
    on, _ = two_calls(S["I"], S["QQ"], n, 1, Qa, 8)
    lev = on[0]["info"]["levels"]
    assert lev[1]["reduced"] < lev[1]["blocks"] and 8 * lev[0]["chunks"] < lev[0]["blocks"], lev


def test_fixed_views_and_duplicate_edges():
    n, f = 1500, 3
    S = synth.make_graph(n, 4 * n, 0.0, seed=13, p_band_out=0.02)
    rng = np.random.default_rng(5)
    I, QQ = S["I"].copy(), S["QQ"].copy()
    flip = rng.random(len(I)) < 0.3
    I[flip] = I[flip][:, ::-1]
    QQ[flip] = synth.qconj(QQ[flip])
    I = np.concatenate([I, I[:80]]).astype(np.int32)
    QQ = np.concatenate([QQ, QQ[:80]])
    Qa = mst_init(I, QQ, S["Qgt"], n, f)
    on, _ = two_calls(I, QQ, n, f, Qa, 8)
    np.testing.assert_array_equal(on[2]["Q"][:f], second_start(Qa, f)[:f])


def test_dead_pivot_is_stored_as_a_zero_reciprocal():
    """every edge of one mid-sequence free view removed: its pivot is dead, the stored inverse carries the reciprocal 0 --
    the view keeps its rotation in both calls"""
    n, m = 4100, 3 * 4100 - 6
    S, Qa = graph(n, m)
    v = 2051
    keep = (S["I"][:, 0] != v) & (S["I"][:, 1] != v)
    I, QQ = np.ascontiguousarray(S["I"][keep]), np.ascontiguousarray(S["QQ"][keep])
    on, _ = two_calls(I, QQ, n, 1, Qa, 8)
    Qb = second_start(Qa, 1)
    np.testing.assert_array_equal(on[1]["Q"][v], Qa[v])
    np.testing.assert_array_equal(on[2]["Q"][v], Qb[v])


@pytest.mark.parametrize("n,m,block", [(4100, 3 * 4100 - 6, 8), (5000, 100000, 24)])
def test_call_patterns(n, m, block):
    S, Qa = graph(n, m)
    I, QQ = S["I"], S["QQ"]
    Qb = second_start(Qa, 1)

    def both(steps, env=()):
        on, off = play(I, QQ, n, 1, steps, env=env), play(I, QQ, n, 1, steps, off=True, env=env)
        assert on[0]["info"]["block"] == block and len(on[0]["info"]["levels"]) >= 3
        equal_records(on, off)
        for r in off:
            assert r["info"]["unit_factor"] == 0 and r["info"]["unit_factor_solves"] == 0
        return on, off

    # one iteration as the second call: the solve comes from the store and the residual half is skipped
    on, off = both([("irls", Qa, 30), ("irls", Qb, 1, "resid")])
    assert on[2]["iters"] == 1 and on[2]["info"]["unit_factor_solves"] == 1
    assert on[2]["resid"].max() <= 1e-12, on[2]["resid"]
    # no iteration: nothing runs
    on, _ = both([("irls", Qa, 30), ("irls", Qb, 0), ("irls", Qb, 30)])
    assert on[2]["iters"] == 0 and on[2]["info"]["unit_factor_solves"] == 0 and on[3]["info"]["unit_factor_solves"] == 1
    # other solves on the handle in between: the store survives them
    on, _ = both([("irls", Qa, 30), ("l1ra",), ("time19",), ("irls", Qb, 30)])
    assert [r["info"]["unit_factor"] for r in on[1:]] == [1, 1, 1, 1]
    assert [r["info"]["unit_factor_solves"] for r in on[1:]] == [0, 0, 0, 1]
    # the cache handed back between two calls: the store is rebuilt
    on, _ = both([("irls", Qa, 30), ("trim",), ("irls", Qb, 30), ("irls", Qa, 30)])
    assert [r["info"]["unit_factor"] for r in on[1:]] == [1, 0, 1, 1]
    assert [r["info"]["unit_factor_solves"] for r in on[1:]] == [0, 0, 0, 1]
    # the give-up of the single-launch upper reduction happens on the filling solve: no store, the same bits as unfaked
    steps = [("irls", Qa, 30), ("irls", Qb, 30)]
    plain = play(I, QQ, n, 1, steps)
    on, _ = both(steps, env=("IROTAVG_BCR_FAKE_UP_FAIL",))
    assert on[1]["stats"]["direct_up_fallbacks"] == 1
    assert [r["info"]["unit_factor"] for r in on] == [0, 0, 0] and on[2]["info"]["unit_factor_solves"] == 0
    equal_records(on, plain)


def test_time_kernel_of_the_rhs_only_solve_needs_a_store():
    n, m = 4100, 3 * 4100 - 6
    S, Qa = graph(n, m)
    with capi.Graph(S["I"], S["QQ"], n, 1, band_direct=1) as G:
        G.set_rotations(Qa)
        for which in (17, 18):
            with pytest.raises(capi.IrotavgError):
                G.time_kernel(which, 1)
        G.irls(4, SIG, 30, 1e-3)
        assert G.direct_info()["unit_factor"] == 1
        assert G.time_kernel(17, 2) > 0 and G.time_kernel(18, 2) > 0 and G.time_kernel(19, 2) > 0
        assert G.direct_info()["unit_factor_solves"] == 0


def routes_off(I, QQ, n, Qa, block, levels=None, closures=0):
    Qb = second_start(Qa, 1)
    steps = [("irls", Qa, 30), ("irls", Qb, 30)]
    on, off = play(I, QQ, n, 1, steps), play(I, QQ, n, 1, steps, off=True)
    equal_records(on, off)
    info = on[0]["info"]
    assert info["block"] == block and info["closures"] == closures, info
    if levels is not None:
        assert len(info["levels"]) == levels, info
    for r in on + off:
        assert r["info"]["unit_factor"] == 0 and r["info"]["unit_factor_solves"] == 0 and r["info"]["unit_factor_bytes"] == 0


def test_two_levels_take_the_full_path():
    n = 3001
    S, Qa = graph(n, 21 * n)
    routes_off(S["I"], S["QQ"], n, Qa, 24, levels=2)


def test_blocks_of_twelve_take_the_full_path():
    n = 3000
    S, Qa = graph(n, 33000, seed=3)
    routes_off(S["I"], S["QQ"], n, Qa, 12)


def test_closures_take_the_full_path():
    n = 3000
    S = synth.closure_graph(n, 12000, 5, seed=1)
    Qa = mst_init(S["I"], S["QQ"], S["Qgt"], n)
    routes_off(S["I"], S["QQ"], n, Qa, 8, closures=5)
