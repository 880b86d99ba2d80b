"""irotavg_window_cemp_batch_dev (irotavg_amd/csrc/wincemp.hip, wincemp.hpp, devapi.hip; torch_api.window_cemp_batch;
docs/window_cemp_batch.md): cycle-edge message passing on many window-size problems in one launch.

The reference is written here and imports nothing from another test: the triangles of the definition, then the iteration
in np.longdouble with the global shift, per problem, computed once per (graph, schedule) and shared (REF).

Tolerance. tri_used, the counts of `results` and the NaN pattern of s must be equal. For s: the same restatement run in
float64 differs from the long-double one by at most TOL_MEASURED = 7.73e-13 rad on this file's graphs (every graph below at
every schedule a test uses), measured on the CPU; the largest is the planted graph at three iterations of beta = 1e6, where
a last-bit difference of e is multiplied by 1e6 in the exponent, and every other case stays below 9e-16. TOL is 100 times
that, 7.73e-11 rad, above the floor of the project's 1e-12: the factor covers another exp and another summation order."""
import numpy as np
import pytest
import torch

from irotavg_amd import capi, torch_api

pytestmark = pytest.mark.gpu
TOL_MEASURED = 7.73e-13
TOL = max(100 * TOL_MEASURED, 1e-12)
LD, DEV = np.longdouble, "cuda"


# ---- the reference ---------------------------------------------------------------------------------------------------------
def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def against(q, flag):
    return q * np.stack([1 + 0 * flag, 1 + 0 * flag, 1 + 0 * flag, np.where(flag, -1, 1)], axis=1)


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
    s.setflags(write=False)
    return dict(s=s, tri_used=used.astype(np.int32), results=[capi.OK, int(used.sum()), int((used == 0).sum())])


REF = {}


def ref(g, beta):
    key = (g["name"], tuple(beta))
    if key not in REF:
        REF[key] = reference(g["I"], g["QQ"], beta)
    return REF[key]


# ---- graphs: dict(name, I, QQ, n, f), f the fewest fixed views that leave at most 64 free ----------------------------------
def unit(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def graph(name, I, Q, turned=None, n=None):
    """measurements Q_b (x) inverse(Q_a), each then turned by turned[k] rad about x"""
    I = np.array(I, dtype=np.int32).reshape(-1, 2)
    QQ = qmul(Q[I[:, 1]], Q[I[:, 0]] * np.array([-1.0, -1.0, -1.0, 1.0]))
    if turned is not None:
        t = np.asarray(turned, dtype=np.float64)
        QQ = qmul(np.stack([np.sin(t / 2), 0 * t, 0 * t, np.cos(t / 2)], axis=1), QQ)
    n = int(I.max()) + 1 if n is None else n
    return dict(name=name, I=I, QQ=np.ascontiguousarray(QQ), n=n, f=max(1, n - 64))


def triangle(theta):
    return graph("triangle%.1f" % theta, [(0, 1), (2, 1), (2, 0)], unit(np.random.default_rng(1), 3), [theta, 0, 0])


def book(p):
    """spine (0, 1) and p pages; every third page has its hub-0 edge doubled and every fifth its hub-1 edge doubled the other
    way round (the runs of equals vary across the lanes of a round); a self loop; one NaN row, the hub-1 edge of page 0"""
    I = [(0, 1)]
    for c in range(p):
        I += [(0, 2 + c), (2 + c, 1) if c % 2 else (1, 2 + c)] + [(0, 2 + c)] * (c % 3 == 0)
        I += [(1, 2 + c) if c % 2 else (2 + c, 1)] * (c % 5 == 0)
    rng = np.random.default_rng(p)
    g = graph("book%d" % p, I + [(2, 2)], unit(rng, 2 + p), rng.uniform(0, 0.3, size=len(I) + 1))
    g["QQ"][2, 1] = np.nan
    return g


def band(m, n=None):
    """the first m edges of a band of three predecessors per view, grouped by the newer view; 0.02 rad noise"""
    rng, nv = np.random.default_rng(m), m // 3 + 3
    I = [(j - d, j) for j in range(nv) for d in (1, 2, 3) if j >= d][:m]
    return graph("band%d_%s" % (m, n), I, unit(rng, nv), rng.normal(scale=0.02, size=m), n=nv if n is None else n)


def planted(seed=3, n=48, bw=6, p_out=0.1, noise=0.01):
    """docs/cycle_check.md's separation graph: every pair of views at distance <= bw joined, 0.01 rad noise, 10 % of the
    edges turned by a further 0.5 .. pi rad about a random axis"""
    rng = np.random.default_rng(seed)
    I = np.array([(a, b) for a in range(n) for b in range(a + 1, min(n, a + bw + 1))], dtype=np.int32)
    g = graph("planted", I, unit(rng, n))
    out = rng.random(len(I)) < p_out
    axis = unit(rng, len(I))[:, :3]
    ang = noise * rng.normal(size=len(I)) + np.where(out, rng.uniform(0.5, np.pi, size=len(I)), 0.0)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    g["QQ"] = qmul(np.concatenate([axis * np.sin(ang / 2)[:, None], np.cos(ang / 2)[:, None]], axis=1), g["QQ"])
    g["out"], g["f"] = out, 1
    return g


TRI, PLANTED = triangle(0.3), planted()
PATH = graph("path", [(0, 1), (1, 2), (2, 3), (3, 4)], unit(np.random.default_rng(2), 5))


# ---- running and comparing -------------------------------------------------------------------------------------------------
def run(gs, beta, qq=None, ids=torch.int32, **kw):
    """the problems packed into one call -> rc, results, and per problem (s, tri_used) as numpy (None where not asked for)"""
    sizes = np.array([(g["n"], g["f"], len(g["I"])) for g in gs])
    ei = torch.tensor(np.concatenate([g["I"] for g in gs]), dtype=ids, device=DEV)
    if qq is None:
        qq = torch.tensor(np.concatenate([g["QQ"] for g in gs]), dtype=torch.float64, device=DEV)
    r = torch_api.window_cemp_batch(sizes, ei, qq, beta, **kw)
    torch.cuda.synchronize()
    cut = np.cumsum(sizes[:, 2])[:-1]
    parts = [[None] * len(gs) if r[key] is None else np.split(r[key].cpu().numpy(), cut) for key in ("s", "tri_used")]
    return r["rc"], r["results"], list(zip(*parts))


def assert_matches(g, beta, got, results):
    e, (s, used) = ref(g, beta), got
    assert (used == e["tri_used"]).all() and results.tolist() == e["results"]
    assert (np.isnan(s) == np.isnan(e["s"])).all()
    has = ~np.isnan(e["s"])
    diff = float(np.abs(s[has] - e["s"][has]).max()) if has.any() else 0.0
    print("%s, %d iterations: %d edges, %d triangles, max |s - reference| = %.3e" % (g["name"], len(beta), len(g["I"]),
                                                                                   e["results"][1], diff))
    assert diff <= TOL
    return e


def check(g, beta):
    """alone and in the middle of a batch: both match the reference, and each other byte for byte"""
    rc, res, alone = run([g], beta)
    e = assert_matches(g, beta, alone[0], res[0])
    rc3, res3, batch = run([TRI, g, PATH], beta)
    assert rc == rc3 == capi.OK and (res3[1] == res[0]).all() and res3[2].tolist() == [capi.OK, 0, 4]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(alone[0], batch[1]))
    assert_matches(TRI, beta, batch[0], res3[0])
    assert np.isnan(batch[2][0]).all() and not batch[2][1].any()                     # the path: NaN everywhere, nothing used
    return e, alone[0]


# ---- the cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 6])
@pytest.mark.parametrize("theta", [0.0, 0.3])
def test_one_triangle_with_one_edge_turned(theta, iters):
    e, (s, used) = check(triangle(theta), torch_api.cemp_beta(iters))
    assert np.abs(s - theta).max() <= TOL and used.tolist() == [1, 1, 1]


def test_a_path_has_no_estimate():
    rc, res, got = run([PATH], torch_api.cemp_beta(2))
    assert rc == capi.OK and res.tolist() == [[capi.OK, 0, 4]] and np.isnan(got[0][0]).all() and not got[0][1].any()


@pytest.mark.parametrize("p", [1, 7, 8, 9, 17, 65])
def test_book_graphs_across_the_group_width(p):
    for beta in ([], torch_api.cemp_beta(3)):
        e, _ = check(book(p), beta)
    assert e["tri_used"][2] == 0 and e["tri_used"][-1] == 0                          # the NaN row, the self loop


@pytest.mark.parametrize("m", [31, 32, 33, 255, 256, 257, 511, 512, 513, 640])
def test_bands_around_the_group_stride_a_thread_pass_the_sort_length_and_the_edge_limit(m):
    g = band(m)
    assert g["n"] - g["f"] <= 64 and check(g, torch_api.cemp_beta(2))[0]["results"][1] > m


def test_320_views_of_which_the_upper_ones_are_isolated():
    g = band(100, n=320)
    assert (g["n"], g["f"]) == (320, 256) and check(g, torch_api.cemp_beta(2))[0]["results"][1] > 100


def test_the_planted_outliers_are_separated_and_a_huge_beta_stays_finite():
    g, beta, out = PLANTED, torch_api.cemp_beta(6), PLANTED["out"]
    e, e0 = ref(g, beta), ref(g, [])
    assert e["s"][~out].max() < 0.05 and e["s"][out].min() > 0.4                     # the reference separates ...
    assert e0["s"][~out].max() > e0["s"][out].min()                                 # ... and the plain mean does not
    check(g, [])
    _, (s, _) = check(g, beta)
    assert (torch_api.rank_from_cemp(torch.tensor(s), 0.2).numpy() == np.where(out, 2, 0)).all()
    assert np.isfinite(check(g, [1e6] * 3)[1][0]).all()                              # a huge beta stays finite by the shift


# ---- the interface -----------------------------------------------------------------------------------------------------------
def test_a_bad_id_fails_its_problem_alone_and_keeps_its_rows():
    beta, bad = torch_api.cemp_beta(2), dict(book(8), name="bad")
    bad["I"] = bad["I"].copy()
    bad["I"][-2, 1] = bad["n"]
    gs = [TRI, bad, PATH, book(7), band(33)]
    M = sum(len(g["I"]) for g in gs)
    s, used = torch.full((M,), -9.0, dtype=torch.float64, device=DEV), torch.full((M,), -7, dtype=torch.int32, device=DEV)
    rc, res, got = run(gs, beta, s=s, used=used, allow_rc=(capi.ERR_BAD_ARG,))
    assert rc == capi.ERR_BAD_ARG and res[1].tolist() == [capi.ERR_BAD_ARG, 0, 0]
    assert (got[1][0] == -9.0).all() and (got[1][1] == -7).all()
    for j in (0, 2, 3, 4):
        assert_matches(gs[j], beta, got[j], res[j])


def test_the_place_in_a_batch_and_a_second_call_change_no_byte():
    g, beta = PLANTED, torch_api.cemp_beta(6)
    want = run([g], beta)[2][0]
    for gs, j in (([g], 0), ([g, TRI, book(9)], 0), ([book(9), TRI, g], 2)):
        got = run(gs, beta)[2][j]
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("form,ids,s,used", [("rows", torch.int32, True, True), ("planes", torch.int64, False, True),
                                             ("padded rows", torch.int32, True, False),
                                             ("rows behind an 8-byte offset", torch.int64, None, None)])
def test_every_stride_form_of_qq_int64_ids_and_each_output_null(form, ids, s, used):
    gs, beta = [book(9), PLANTED, TRI], torch_api.cemp_beta(2)
    t = torch.tensor(np.concatenate([g["QQ"] for g in gs]), dtype=torch.float64, device=DEV)
    if form == "planes":
        t = t.t().contiguous().t()                                                   # strides (1, M)
    elif form == "padded rows":
        t = torch.cat([t, t[:, :2]], dim=1)[:, :4]                                   # strides (6, 1)
    elif form.endswith("offset"):
        t = torch.cat([t.new_zeros(1), t.flatten()])[1:].view(-1, 4)                 # strides (4, 1), not 16-byte aligned
        assert t.data_ptr() % 16 == 8
    want, got = run(gs, beta), run(gs, beta, qq=t, ids=ids, s=s, used=used)
    assert got[0] == capi.OK and (got[1] == want[1]).all()
    for a, b in zip(got[2], want[2]):
        for x, y, asked in zip(a, b, (s, used)):
            assert x.tobytes() == y.tobytes() if asked else x is None


def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream():
    gs, beta = [PLANTED, book(17)], torch_api.cemp_beta(2)
    want = np.concatenate([p[0] for p in run(gs, beta)[2]])
    half = torch.tensor(np.concatenate([g["QQ"] for g in gs]) * 0.5, dtype=torch.float64, device=DEV)
    ei = torch.tensor(np.concatenate([g["I"] for g in gs]), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        qq = half * 2.0                                           # exact: the inputs of the synchronised run, produced on the stream
        r = torch_api.window_cemp_batch(np.array([(g["n"], g["f"], len(g["I"])) for g in gs]), ei, qq, beta)
        doubled = r["s"] * 2                                      # consumed right behind the call, no synchronise
    side.synchronize()
    assert r["s"].cpu().numpy().tobytes() == want.tobytes()
    assert np.array_equal(doubled.cpu().numpy(), 2 * want, equal_nan=True)
