"""irotavg_cycle_cemp / irotavg_cycle_cemp_dev (irotavg_amd/csrc/cemp.hip, cemp.hpp, devapi.hip; torch_api.cycle_cemp;
docs/cycle_check.md, "Corruption estimates"): cycle-edge message passing over the triangles of every edge, on the device.

The reference is written here, independent of cemp.hpp: the triangle enumeration of test_gpu_cycle_check.py restated, then
the definition in np.longdouble with the global shift. It is computed once per (graph, schedule) and shared (REF).

Tolerance. tri_used and summary must be equal. For s: the same restatement run in float64 differs from the long-double one
by at most 7.73e-13 rad on this file's graphs, measured on the CPU: that is the separation graph at beta = 1e6, where a
last-bit difference of e is multiplied by 1e6 in the exponent; every other case stays below 9e-16. 100 times the largest is
TOL = 7.73e-11 rad, above the floor of 1e-12 (the project's TOL_MIN for a triangle error). The factor covers another exp
and another summation order."""
import ctypes as C

import numpy as np
import pytest
import torch

from irotavg_amd import capi, synth, torch_api

pytestmark = pytest.mark.gpu
TOL = max(100 * 7.73e-13, 1e-12)
G = 8                                                            # the group width cemp.hip is compiled with
LD = np.longdouble


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def t64(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev())


def t32(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.int32, device=dev())


# ---- the reference ---------------------------------------------------------------------------------------------------------
def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def against(q, flag):
    q = q.copy()
    q[flag, 3] = -q[flag, 3]
    return q


def triangles(I):
    """every (k, k1, k1 against its stored direction, k2, k2 against) of the definition"""
    out, between = {}, {}
    for k, (a, b) in enumerate(I.tolist()):
        if a != b:
            out.setdefault(b, []).append((a, k, True))
            out.setdefault(a, []).append((b, k, False))
            between.setdefault((a, b), []).append((k, False))
            between.setdefault((b, a), []).append((k, True))
    T = [(k, k1, g1, k2, g2) for k, (a, b) in enumerate(I.tolist()) if a != b for c, k1, g1 in out[b] if c != a
         for k2, g2 in between.get((c, a), ())]
    return np.array(T, dtype=np.int64).reshape(-1, 5)


def reference(I, QQ, beta, real=LD):
    m, T, QQ = len(I), triangles(np.asarray(I, dtype=np.int64)), QQ.astype(real)
    pi = real(np.pi) if real is np.float64 else 4 * np.arctan(LD(1))
    with np.errstate(invalid="ignore"):
        q = qmul(against(QQ[T[:, 3]], T[:, 4] != 0), qmul(against(QQ[T[:, 1]], T[:, 2] != 0), QQ[T[:, 0]]))
        th = 2 * np.arctan2(np.sqrt(q[:, 0] ** 2 + q[:, 1] ** 2 + q[:, 2] ** 2), q[:, 3])
        d = np.abs(np.where(th >= pi, th - 2 * pi, th))
    T, d = T[np.isfinite(d)], d[np.isfinite(d)]
    k, used = T[:, 0], np.bincount(T[:, 0], minlength=m)

    def per_edge(x):
        return np.array([x[k == j].sum() for j in range(m)], dtype=real)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = per_edge(d) / used
        for b in beta:
            e = s[T[:, 1]] + s[T[:, 3]]
            mu = np.full(m, np.inf, dtype=real)
            np.fmin.at(mu, k, e)
            w = np.exp(-real(b) * (e - mu[k]))
            keep = ~np.isnan(w)
            w, wd = np.where(keep, w, 0), np.where(keep, w * d, 0)
            s = per_edge(wd) / per_edge(w)
    r = dict(s=s, tri_used=used.astype(np.int32), summary=dict(records=int(used.sum()), untested=int((used == 0).sum())))
    s.setflags(write=False)
    return r


REF = {}


def ref(g, beta):
    key = (g["name"], tuple(beta))
    if key not in REF:
        REF[key] = reference(g["I"], g["QQ"], beta)
    return REF[key]


def run_dev(g, beta, **kw):
    r = torch_api.cycle_cemp(t32(g["I"]), t64(g["QQ"]), g["n_total"], beta, **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def assert_matches(g, beta, r):
    e = ref(g, beta)
    assert (r["tri_used"] == e["tri_used"]).all() and r["summary"] == e["summary"]
    assert (np.isnan(r["s"]) == np.isnan(e["s"])).all()
    has = ~np.isnan(e["s"])
    diff = float(np.abs(r["s"][has] - e["s"][has]).max()) if has.any() else 0.0
    print("%s, %d iterations: %d edges, %d records, max |s - reference| = %.3e" % (g["name"], len(beta), len(g["I"]),
                                                                                 e["summary"]["records"], diff))
    assert diff <= TOL
    return e


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def turn(angle):
    return np.array([np.sin(angle / 2), 0.0, 0.0, np.cos(angle / 2)])


def graph(name, I, Q, n_total=None, turned=None):
    """measurements Q_b (x) inverse(Q_a), each then turned by turned[k] rad about x"""
    I = np.array(I, dtype=np.int32).reshape(-1, 2)
    QQ = qmul(Q[I[:, 1]], synth.qconj(Q[I[:, 0]]))
    if turned is not None:
        QQ = qmul(np.stack([turn(t) for t in turned]), QQ)
    return dict(name=name, I=I, QQ=np.ascontiguousarray(QQ), n_total=int(I.max()) + 1 if n_total is None else n_total)


def unit(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def book(p):
    """spine (0, 1) and p pages; every third page has its hub-0 edge doubled and every fifth its hub-1 edge doubled the other
    way round (the runs of equals vary across the lanes of a round); a self loop; one NaN row, the hub-1 edge of page 0"""
    I = [(0, 1)]
    for c in range(p):
        I += [(0, 2 + c), (2 + c, 1) if c % 2 else (1, 2 + c)] + [(0, 2 + c)] * (c % 3 == 0)
        I += [(1, 2 + c) if c % 2 else (2 + c, 1)] * (c % 5 == 0)
    rng = np.random.default_rng(p)
    g = graph("book%d" % p, I + [(2, 2)], unit(rng, 2 + p), turned=rng.uniform(0, 0.3, size=len(I) + 1))
    g["QQ"][2, 1] = np.nan
    return g


def planted(seed=3, n=48, bw=6, p_out=0.1, noise=0.01):
    """the separation graph: every pair of views at distance <= bw joined, 0.01 rad noise, 10 % of the edges turned by a
    further 0.5 .. pi rad about a random axis"""
    rng = np.random.default_rng(seed)
    I = np.array([(a, b) for a in range(n) for b in range(a + 1, min(n, a + bw + 1))], dtype=np.int32)
    g = graph("planted", I, unit(rng, n))
    out = rng.random(len(I)) < p_out
    axis = unit(rng, len(I))[:, :3]
    ang = noise * rng.normal(size=len(I)) + np.where(out, rng.uniform(0.5, np.pi, size=len(I)), 0.0)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    g["QQ"] = qmul(np.concatenate([axis * np.sin(ang / 2)[:, None], np.cos(ang / 2)[:, None]], axis=1), g["QQ"])
    g["out"] = out
    return g


PLANTED = planted()


def band(m):
    """the first m edges of a band of three predecessors per view, grouped by the newer view; 0.02 rad noise"""
    rng, n = np.random.default_rng(m), m // 3 + 3
    I = [(j - d, j) for j in range(n) for d in (1, 2, 3) if j >= d][:m]
    return graph("band%d" % m, I, unit(rng, n), n_total=n, turned=rng.normal(scale=0.02, size=m))


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 6])
@pytest.mark.parametrize("theta", [0.0, 0.3])
def test_one_triangle_with_one_edge_turned(theta, iters):
    g = graph("triangle%.1f" % theta, [(0, 1), (2, 1), (2, 0)], unit(np.random.default_rng(1), 3), turned=[theta, 0, 0])
    beta = torch_api.cemp_beta(iters)
    r = run_dev(g, beta)
    assert np.abs(r["s"] - theta).max() <= TOL and r["tri_used"].tolist() == [1, 1, 1]
    assert_matches(g, beta, r)


def test_a_path_has_no_estimate():
    g = graph("path", [(0, 1), (1, 2), (2, 3), (3, 4)], unit(np.random.default_rng(2), 5))
    r = run_dev(g, torch_api.cemp_beta(2))
    assert np.isnan(r["s"]).all() and not r["tri_used"].any() and r["summary"] == dict(records=0, untested=4)


@pytest.mark.parametrize("p", [1, G - 1, G, G + 1, 2 * G + 1, 65])
def test_book_graphs_across_the_group_width(p):
    g = book(p)
    for beta in ([], torch_api.cemp_beta(3)):
        e = assert_matches(g, beta, run_dev(g, beta))
    assert e["tri_used"][2] == 0 and e["tri_used"][-1] == 0                           # the NaN row, the self loop


@pytest.mark.parametrize("m", [31, 32, 33, 129])
def test_edge_counts_around_a_workgroup_pass(m):
    g = band(m)
    assert assert_matches(g, torch_api.cemp_beta(2), run_dev(g, torch_api.cemp_beta(2)))["summary"]["records"] > m


def test_the_planted_outliers_are_separated():
    g, beta, out = PLANTED, torch_api.cemp_beta(6), PLANTED["out"]
    e, e0 = ref(g, beta), ref(g, [])
    assert e["s"][~out].max() < 0.05 and e["s"][out].min() > 0.4                      # the reference separates ...
    assert e0["s"][~out].max() > e0["s"][out].min()                                  # ... and the plain mean does not
    assert_matches(g, [], run_dev(g, []))
    r = torch_api.cycle_cemp(t32(g["I"]), t64(g["QQ"]), g["n_total"])                # (the default schedule)
    assert_matches(g, beta, {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()})
    assert (torch_api.rank_from_cemp(r["s"], 0.2).cpu().numpy() == np.where(out, 2, 0)).all()


def test_a_huge_beta_stays_finite_by_the_shift():
    r = run_dev(PLANTED, [1e6] * 3)
    e = assert_matches(PLANTED, [1e6] * 3, r)
    assert (np.isfinite(r["s"]) == np.isfinite(e["s"].astype(np.float64))).all() and np.isfinite(r["s"]).all()


# ---- the interface -----------------------------------------------------------------------------------------------------------
def raw(g, I, beta, max_records, s, used, stream=None):
    ei, qq, h = t32(I), t64(g["QQ"]), (C.c_int64 * 2)(-1, -2)
    b = np.array(beta, dtype=np.float64)
    rc = capi.lib().irotavg_cycle_cemp_dev(len(I), g["n_total"], C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1,
                                           len(b), capi._d(b), max_records, C.c_void_p(s.data_ptr()), C.c_void_p(used.data_ptr()),
                                           h, stream)
    torch.cuda.synchronize()
    return rc, list(h)


def test_a_bad_id_and_the_record_cap_leave_the_outputs_untouched():
    g, beta = PLANTED, torch_api.cemp_beta(2)
    need = ref(g, beta)["summary"]["records"]
    s, used = torch.full((len(g["I"]),), -9.0, dtype=torch.float64, device=dev()), t32(np.full(len(g["I"]), -7))
    bad = g["I"].copy()
    bad[-1, 1] = g["n_total"]
    assert raw(g, bad, beta, 0, s, used) == (capi.ERR_BAD_ARG, [-1, -2])
    assert raw(g, g["I"], beta, need - 1, s, used) == (capi.ERR_NOMEM, [need, 0])
    assert (s == -9.0).all() and (used == -7).all()
    assert raw(g, g["I"], beta, need, s, used) == (capi.OK, [need, 0])
    assert_matches(g, beta, dict(s=s.cpu().numpy(), tri_used=used.cpu().numpy(), summary=ref(g, beta)["summary"]))
    r = torch_api.cycle_cemp(t32(g["I"]), t64(g["QQ"]), g["n_total"], beta, max_records=1, allow_rc=(capi.ERR_NOMEM,))
    assert r["rc"] == capi.ERR_NOMEM and r["summary"]["records"] == need


@pytest.mark.parametrize("mask", range(8))
def test_null_outputs_strides_int64_ids_and_two_calls(mask):
    g, beta = PLANTED, torch_api.cemp_beta(2)
    want = run_dev(g, beta)
    planes = t64(g["QQ"].T).t()                                                       # column-major: strides (1, m)
    r = torch_api.cycle_cemp(torch.tensor(g["I"], dtype=torch.int64, device=dev()), planes, g["n_total"], beta,
                             s=bool(mask & 1), used=bool(mask & 2), summary=bool(mask & 4))
    for bit, key in ((1, "s"), (2, "tri_used"), (4, "summary")):
        if not mask & bit:
            assert r[key] is None
        elif key == "summary":
            assert r[key] == want[key]
        else:
            assert r[key].cpu().numpy().tobytes() == want[key].tobytes()              # bitwise: two calls, either layout


def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream():
    g, beta = PLANTED, torch_api.cemp_beta(2)
    want = run_dev(g, beta)
    ei, half = t32(g["I"]), t64(g["QQ"] * 0.5)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        qq = half * 2.0                                           # exact: the inputs of the synchronised run, produced on the stream
        r = torch_api.cycle_cemp(ei, qq, g["n_total"], beta)
        doubled = r["s"] * 2                                      # consumed right behind the call, no synchronise
    side.synchronize()
    assert r["s"].cpu().numpy().tobytes() == want["s"].tobytes() and (doubled.cpu().numpy() == 2 * want["s"]).all()
    h = capi.cycle_cemp(g["I"], g["QQ"], g["n_total"], beta)      # the host form stages through the same kernels
    assert h["s"].tobytes() == want["s"].tobytes() and (h["tri_used"] == want["tri_used"]).all() and h["summary"] == want["summary"]
