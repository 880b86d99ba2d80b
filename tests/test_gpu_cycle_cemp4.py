"""irotavg_cycle_cemp4 / irotavg_cycle_cemp4_dev (irotavg_amd/csrc/cemp4.hip, cemp4.hpp, devapi.hip; torch_api.cycle_cemp4;
docs/cycle_check.md, "Corruption estimates over four-cycles"): message passing over the quadrilaterals of the edges listed.

The reference is written here, independent of cemp4.hpp: an enumeration from neighbour dictionaries, then the definition in
np.longdouble with the global shift, computed once per case and shared (REF). quad_used, summary and the NaN positions
must be equal, s4 within TOL.

Tolerance. The same restatement run in float64 differs from the long-double one by at most 9.45e-16 rad over this file's
cases, measured on the CPU (the ladder of 1030 rungs with every edge listed; beta = 1e6 on the separation graph gives
1.7e-16: its three quadrilaterals per closure leave the shift little to amplify). 100 times the largest is 9.45e-14 rad, below
the floor of 1e-12 rad, so TOL is the floor.

The separation graph with seed 3 draws as the issue's sketch did: the plain mean gives inliers up to 1.585 and outliers down
to 0.593 rad, six iterations give inliers <= 0.027 and outliers >= 0.598 rad."""
import ctypes as C

import numpy as np
import pytest
import torch

from irotavg_amd import capi, torch_api
from test_gpu_cycle_cemp import LD, against, dev, graph, qmul, reference as triangle_reference, t32, t64, unit

pytestmark = pytest.mark.gpu
TOL = max(100 * 9.45e-16, 1e-12)
BETA6 = torch_api.cemp_beta(6)


# ---- the reference ---------------------------------------------------------------------------------------------------------
def quadrilaterals(I, edges):
    """every (t, k, k1, k1 against its stored direction, k2, k2 against, k3, k3 against) of the definition"""
    out, between = {}, {}
    for k, (a, b) in enumerate(I.tolist()):
        if a != b:
            out.setdefault(b, []).append((a, k, True))
            out.setdefault(a, []).append((b, k, False))
            between.setdefault((a, b), []).append((k, False))
            between.setdefault((b, a), []).append((k, True))
    T = [(t, k, k1, g1, k2, g2, k3, g3) for t, k in enumerate(edges) for a, b in [I[k].tolist()] if a != b
         for c, k1, g1 in out[b] if c != a for d, k2, g2 in out[c] if d != a and d != b for k3, g3 in between.get((d, a), ())]
    return np.array(T, dtype=np.int64).reshape(-1, 8)


def reference(I, QQ, s_in, edges, beta, real=LD):
    edges, QQ = np.asarray(edges, dtype=np.int64), QQ.astype(real)
    ne, T = len(edges), quadrilaterals(np.asarray(I, dtype=np.int64), edges.tolist())
    pi = real(np.pi) if real is np.float64 else 4 * np.arctan(LD(1))
    with np.errstate(invalid="ignore"):
        q = qmul(against(QQ[T[:, 2]], T[:, 3] != 0), QQ[T[:, 1]])
        q = qmul(against(QQ[T[:, 6]], T[:, 7] != 0), qmul(against(QQ[T[:, 4]], T[:, 5] != 0), q))
        th = 2 * np.arctan2(np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2 + q[:, 2] ** 2), q[:, 3])
        d = np.abs(np.where(th >= pi, th - 2 * pi, th))
    T, d = T[np.isfinite(d)], d[np.isfinite(d)]
    t, used = T[:, 0], np.bincount(T[:, 0], minlength=ne)

    def per_position(x):
        return np.array([x[t == j].sum() for j in range(ne)], dtype=real)
    with np.errstate(invalid="ignore", divide="ignore"):
        s4, S = per_position(d) / used, np.asarray(s_in).astype(real)
        for b in beta:
            S[edges] = s4
            e = S[T[:, 2]] + S[T[:, 4]] + S[T[:, 6]]
            mu = np.full(ne, np.inf, dtype=real)
            np.fmin.at(mu, t, e)
            w = np.exp(-real(b) * (e - mu[t]))
            keep = ~np.isnan(w)
            s4 = per_position(np.where(keep, w * d, 0)) / per_position(np.where(keep, w, 0))
    s4.setflags(write=False)
    return dict(s=s4, quad_used=used.astype(np.int32), summary=dict(records=int(used.sum()), untested=int((used == 0).sum())))


REF = {}


def ref(g, edges, beta, real=LD):
    key = (g["name"], tuple(edges), tuple(beta), real)
    if key not in REF:
        REF[key] = reference(g["I"], g["QQ"], g["s_in"], edges, beta, real)
    return REF[key]


def run_dev(g, edges, beta, s_in=None, **kw):
    r = torch_api.cycle_cemp4(t32(g["I"]), t64(g["QQ"]), g["n_total"], t64(g["s_in"] if s_in is None else s_in), t32(edges), beta, **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def assert_matches(g, edges, beta, r):
    e = ref(g, edges, beta)
    assert (r["quad_used"] == e["quad_used"]).all() and r["summary"] == e["summary"]
    assert (np.isnan(r["s"]) == np.isnan(e["s"])).all()
    has = ~np.isnan(e["s"])
    diff = float(np.abs(r["s"][has] - e["s"][has]).max()) if has.any() else 0.0
    print("%s, %d listed, %d iterations: %d records, max |s4 - reference| = %.3e" % (g["name"], len(edges), len(beta),
                                                                                   e["summary"]["records"], diff))
    assert diff <= TOL
    return e


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def square(theta):
    g = graph("square%.1f" % theta, [(0, 1), (2, 1), (2, 3), (0, 3)], unit(np.random.default_rng(1), 4), turned=[theta, 0, 0, 0])
    return dict(g, s_in=np.full(4, np.nan))


def ladder(p):
    """tested edge (0, 1) and p rungs 1 - c - d - 0; every third rung has its middle edge doubled and every fifth its edge at
    view 0 doubled the other way round; a self loop; one NaN row, the middle edge of rung 0; s_in with one NaN"""
    I = [(0, 1)]
    for r in range(p):
        c, d = 2 + 2 * r, 3 + 2 * r
        I += [(1, c), (d, c), (d, 0)] + [(c, d)] * (r % 3 == 0) + [(0, d)] * (r % 5 == 0)
    rng = np.random.default_rng(p)
    g = graph("ladder%d" % p, I + [(2, 2)], unit(rng, 2 + 2 * p), turned=rng.uniform(0, 0.3, size=len(I) + 1))
    g["QQ"][2, 1] = np.nan
    g["s_in"] = rng.uniform(0, 0.1, size=len(I) + 1)
    g["s_in"][5] = np.nan
    return g


def band(m):
    """the first m edges of a band of three predecessors per view: no edge is listed twice, every listed edge has quadrilaterals"""
    rng, n = np.random.default_rng(m), m // 3 + 3
    I = [(j - d, j) for j in range(n) for d in (1, 2, 3) if j >= d][:m]
    return dict(graph("band%d" % m, I, unit(rng, n), n_total=n, turned=rng.normal(scale=0.02, size=m)), s_in=rng.uniform(0, 0.05, size=m))


def closures(seed=3, n=64, noise=0.01):
    """the separation graph: every pair at distance <= 4, sixteen closures in four clusters; 0.01 rad noise; 10 % of the band
    edges and closures 1, 6, 8, 9 turned by a further 0.5 .. pi rad about a random axis. The draws follow planted() of
    test_gpu_cycle_cemp.py: poses, band outlier mask, axes, angles. s_in: the float64 of the triangle reference."""
    rng = np.random.default_rng(seed)
    I = [(a, b) for a in range(n) for b in range(a + 1, min(n, a + 5))]
    nb = len(I)
    I += [(a + j, b + j) for a, b in ((2, 30), (10, 50), (20, 58), (36, 60)) for j in range(4)]
    g = graph("closures", I, unit(rng, n))
    out = np.concatenate([rng.random(nb) < 0.1, np.isin(np.arange(16), (1, 6, 8, 9))])
    axis = unit(rng, len(I))[:, :3]
    ang = noise * rng.normal(size=len(I)) + np.where(out, rng.uniform(0.5, np.pi, size=len(I)), 0.0)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    g["QQ"] = qmul(np.concatenate([axis * np.sin(ang / 2)[:, None], np.cos(ang / 2)[:, None]], axis=1), g["QQ"])
    g["s_in"] = triangle_reference(g["I"], g["QQ"], BETA6)["s"].astype(np.float64)
    return dict(g, out=out, listed=np.arange(nb, nb + 16))


CLOSURES = closures()


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 6])
@pytest.mark.parametrize("theta", [0.0, 0.3])
def test_one_square_with_one_edge_turned(theta, iters):
    g, beta = square(theta), torch_api.cemp_beta(iters)
    r = run_dev(g, range(4), beta)
    assert np.abs(r["s"] - theta).max() <= TOL and r["quad_used"].tolist() == [1, 1, 1, 1]
    assert_matches(g, range(4), beta, r)
    r0, r1 = run_dev(g, [0], []), run_dev(g, [0], BETA6[:1])         # one edge listed, the other three NaN in s_in
    assert abs(r0["s"][0] - theta) <= TOL and np.isnan(r1["s"][0])


def test_a_path_and_a_triangle_have_no_estimate():
    g = graph("path", [(0, 1), (1, 2), (2, 3), (3, 4), (5, 6), (6, 7), (7, 5)], unit(np.random.default_rng(2), 8))
    r = run_dev(dict(g, s_in=np.zeros(7)), range(7), torch_api.cemp_beta(2))
    assert np.isnan(r["s"]).all() and not r["quad_used"].any() and r["summary"] == dict(records=0, untested=7)


@pytest.mark.parametrize("p", [1, 7, 8, 9, 17, 65, 1030])
def test_ladder_graphs_across_the_group_width_and_the_slab(p):
    g = ladder(p)
    for beta in ([], torch_api.cemp_beta(3)):
        e = assert_matches(g, range(len(g["I"])), beta, run_dev(g, range(len(g["I"])), beta))
        assert_matches(g, [0], beta, run_dev(g, [0], beta))
    assert e["quad_used"][2] == 0 and e["quad_used"][-1] == 0 and e["quad_used"][0] > p     # the NaN row, the self loop


@pytest.mark.parametrize("ne", [3, 4, 5, 17])
def test_listed_counts_around_a_workgroup_pass(ne):
    g = band(40)
    assert assert_matches(g, range(7, 7 + ne), BETA6[:2], run_dev(g, range(7, 7 + ne), BETA6[:2]))["summary"]["records"] > ne


def test_duplicates_and_the_own_entry_of_a_listed_edge():
    g, edges = CLOSURES, [250, 246, 250, 3, 246]
    r = run_dev(g, edges, BETA6)
    assert_matches(g, edges, BETA6, r)
    assert r["s"][0].tobytes() == r["s"][2].tobytes() and r["s"][1].tobytes() == r["s"][4].tobytes()
    other = g["s_in"].copy()
    other[edges] = 7.0                                                                    # NaN there and 7.0 there
    assert run_dev(g, edges, BETA6, s_in=other)["s"].tobytes() == r["s"].tobytes()


def test_the_planted_closures_are_separated():
    g, out = CLOSURES, CLOSURES["out"][-16:]
    e, e0 = ref(g, g["listed"], BETA6), ref(g, g["listed"], [])
    assert np.isnan(g["s_in"][-16:]).all() and not np.isnan(g["s_in"][:-16]).any() and (e["quad_used"] == 3).all()
    assert e0["s"][~out].max() > e0["s"][out].min()                                      # the plain mean does not separate ...
    assert e["s"][~out].max() < 0.05 and e["s"][out].min() > 0.4                          # ... and the reference does
    assert_matches(g, g["listed"], [], run_dev(g, g["listed"], []))
    s = t64(g["s_in"])
    q = torch_api.cycle_cemp4(t32(g["I"]), t64(g["QQ"]), g["n_total"], s)                 # (the default subset and schedule)
    assert (q["edges"].cpu().numpy() == g["listed"]).all()
    assert_matches(g, g["listed"], BETA6, {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in q.items()})
    s[q["edges"]] = q["s"]
    assert (torch_api.rank_from_cemp(s, 0.2).cpu().numpy() == np.where(g["out"], 2, 0)).all()


def test_a_huge_beta_stays_finite_by_the_shift():
    r = run_dev(CLOSURES, CLOSURES["listed"], [1e6] * 3)
    assert_matches(CLOSURES, CLOSURES["listed"], [1e6] * 3, r)
    assert np.isfinite(r["s"]).all()


# ---- the interface -----------------------------------------------------------------------------------------------------------
def raw(g, I, edges, beta, max_records, s4, used):
    ei, qq, si, ed, h = t32(I), t64(g["QQ"]), t64(g["s_in"]), t32(edges), (C.c_int64 * 2)(-1, -2)
    b, p = np.array(beta, dtype=np.float64), lambda t: C.c_void_p(t.data_ptr())
    rc = capi.lib().irotavg_cycle_cemp4_dev(len(I), g["n_total"], p(ei), p(qq), 4, 1, p(si), len(edges), p(ed), len(b), capi._d(b),
                                            max_records, p(s4), p(used), h, None)
    torch.cuda.synchronize()
    return rc, list(h)


def test_bad_ids_and_the_record_cap_leave_the_outputs_untouched():
    g, beta, edges = CLOSURES, BETA6[:2], CLOSURES["listed"]
    need = ref(g, edges, beta)["summary"]["records"]
    s4, used = torch.full((16,), -9.0, dtype=torch.float64, device=dev()), t32(np.full(16, -7))
    bad_view, bad_edge = g["I"].copy(), edges.copy()
    bad_view[-1, 1], bad_edge[5] = g["n_total"], len(g["I"])
    assert raw(g, bad_view, edges, beta, 0, s4, used) == (capi.ERR_BAD_ARG, [-1, -2])
    assert raw(g, g["I"], bad_edge, beta, 0, s4, used) == (capi.ERR_BAD_ARG, [-1, -2])
    assert raw(g, g["I"], edges, beta, need - 1, s4, used) == (capi.ERR_NOMEM, [need, 0])
    assert (s4 == -9.0).all() and (used == -7).all()
    assert raw(g, g["I"], edges, beta, need, s4, used) == (capi.OK, [need, 0])
    assert_matches(g, edges, beta, dict(s=s4.cpu().numpy(), quad_used=used.cpu().numpy(), summary=ref(g, edges, beta)["summary"]))


@pytest.mark.parametrize("mask", range(8))
def test_null_outputs_strides_int64_ids_and_two_calls(mask):
    g, beta, edges = CLOSURES, BETA6[:2], CLOSURES["listed"]
    want = run_dev(g, edges, beta)
    planes = t64(g["QQ"].T).t()                                                       # column-major: strides (1, m)
    i64 = dict(dtype=torch.int64, device=dev())
    r = torch_api.cycle_cemp4(torch.tensor(g["I"], **i64), planes, g["n_total"], t64(g["s_in"]), torch.tensor(edges, **i64), beta,
                              s4=bool(mask & 1), used=bool(mask & 2), summary=bool(mask & 4))
    for bit, key in ((1, "s"), (2, "quad_used"), (4, "summary")):
        if not mask & bit:
            assert r[key] is None
        elif key == "summary":
            assert r[key] == want[key]
        else:
            assert r[key].cpu().numpy().tobytes() == want[key].tobytes()              # bitwise: two calls, either layout


def test_inputs_in_flight_outputs_consumed_on_a_side_stream_and_the_host_form():
    g, beta, edges = CLOSURES, BETA6[:2], CLOSURES["listed"]
    want = run_dev(g, edges, beta)
    ei, half, si, ed = t32(g["I"]), t64(g["QQ"] * 0.5), t64(g["s_in"]), t32(edges)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r = torch_api.cycle_cemp4(ei, half * 2.0, g["n_total"], si * 1.0, ed, beta)   # exact; produced on the stream
        doubled = r["s"] * 2                                      # consumed right behind the call, no synchronise
    side.synchronize()
    assert r["s"].cpu().numpy().tobytes() == want["s"].tobytes() and (doubled.cpu().numpy() == 2 * want["s"]).all()
    for sub in (edges, None):                                     # the host form stages through the same kernels
        h = capi.cycle_cemp4(g["I"], g["QQ"], g["n_total"], g["s_in"], sub, beta)
        w = want if sub is not None else run_dev(g, range(len(g["I"])), beta)
        assert h["s"].tobytes() == w["s"].tobytes() and (h["quad_used"] == w["quad_used"]).all() and h["summary"] == w["summary"]
