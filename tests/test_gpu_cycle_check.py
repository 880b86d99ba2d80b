"""irotavg_cycle_check / irotavg_cycle_check_dev (irotavg_amd/csrc/cycles.hip, cycles.hpp, devapi.hip;
torch_api.cycle_check; docs/cycle_check.md): the triangle test of every edge on the device.

The reference is a NumPy restatement of the definition written here (triangles from Python dictionaries, the errors of all
of them in one vectorised pass), independent of cycles.hpp. It is computed once per graph and shared (REF).

Tolerances. Counts must be equal. tri_min must agree within 1e-12 rad: the bound test_k1_edge_residual holds edge_log to; a
product of three unit quaternions and one atan2 err by a few 1e-16. tri_ok must be equal on the condition, asserted, that
no reference error lies within 1e-9 of the threshold: thresholds are chosen in a gap.

The shapes are the smallest at which each part can go wrong: rows across every group width (8, 16, 32, 64) and one past it,
the shorter / longer choice, search misses at both ends of a row, a workgroup with more than one pass, ids at the top of
the int32 range."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from irotavg_amd import capi, graphio, synth, torch_api

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
TOL_MIN = 1e-12
GAP = 1e-9


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
    """q(k, b_k -> a_k): only w negated"""
    q = q.copy()
    q[flag, 3] = -q[flag, 3]
    return q


def triangles(I):
    """every (k, k1, k1 against its stored direction, k2, k2 against) of the definition"""
    out, between = {}, {}
    for k, (a, b) in enumerate(I.tolist()):
        if a == b:
            continue
        out.setdefault(a, []).append((b, k, False))
        out.setdefault(b, []).append((a, k, True))
        between.setdefault((a, b), []).append((k, False))
        between.setdefault((b, a), []).append((k, True))
    T = []
    for k, (a, b) in enumerate(I.tolist()):
        if a == b:
            continue
        for c, k1, g1 in out[b]:                          # b -> c, then every c -> a
            if c != a:
                T.extend((k, k1, g1, k2, g2) for k2, g2 in between.get((c, a), ()))
    return np.array(T, dtype=np.int64).reshape(-1, 5)


def reference(I, QQ, threshold):
    I = np.asarray(I, dtype=np.int64)
    m = len(I)
    T = triangles(I)
    k = T[:, 0]
    with np.errstate(invalid="ignore"):
        d = qmul(against(QQ[T[:, 3]], T[:, 4] != 0), qmul(against(QQ[T[:, 1]], T[:, 2] != 0), QQ[k]))
        s = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + d[:, 2] ** 2)
        th = 2 * np.arctan2(s, d[:, 3])
        th = np.where(th < -np.pi, th + 2 * np.pi, np.where(th >= np.pi, th - 2 * np.pi, th))
        err = np.abs(th)
        ok = err <= threshold
    count = np.bincount(k, minlength=m)
    nok = np.bincount(k[ok], minlength=m)
    mn = np.full(m, INF)
    fin = np.isfinite(err)
    np.minimum.at(mn, k[fin], err[fin])
    summary = dict(triangles=int(count.sum()), supported=int((nok >= 1).sum()),
                   contradicted=int(((count >= 1) & (nok == 0)).sum()), untested=int((count == 0).sum()))
    r = dict(tri_count=count.astype(np.int32), tri_ok=nok.astype(np.int32), tri_min=mn, summary=summary, err=err)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


REF = {}


def ref(g):
    if g["name"] not in REF:
        REF[g["name"]] = reference(g["I"], g["QQ"], g["threshold"])
    return REF[g["name"]]


def run_dev(g, **kw):
    r = torch_api.cycle_check(t32(g["I"]), t64(g["QQ"]), g["n_total"], g["threshold"], **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def assert_matches(g, r, what=""):
    e = ref(g)
    fin = np.isfinite(e["err"])
    assert not (np.abs(e["err"][fin] - g["threshold"]) < GAP).any(), "the threshold is not in a gap"
    assert (r["tri_count"] == e["tri_count"]).all(), what
    assert (r["tri_ok"] == e["tri_ok"]).all(), what
    assert (np.isinf(r["tri_min"]) == np.isinf(e["tri_min"])).all() and not np.isnan(r["tri_min"]).any(), what
    has = np.isfinite(e["tri_min"])
    diff = np.abs(r["tri_min"][has] - e["tri_min"][has]).max() if has.any() else 0.0
    print("%s %s: %d edges, %d triangles, max |tri_min - reference| = %.3e" % (g["name"], what, len(g["I"]),
                                                                              e["summary"]["triangles"], diff))
    assert diff <= TOL_MIN, what
    assert r["summary"] == e["summary"], what
    s = r["summary"]
    assert s["supported"] + s["contradicted"] + s["untested"] == len(g["I"])


# ---- graphs ----------------------------------------------------------------------------------------------------------------
def unit(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def turn(angle):
    return np.array([np.sin(angle / 2), 0.0, 0.0, np.cos(angle / 2)])


def measured(Q, I):
    """Q_b (x) inverse(Q_a) for every edge"""
    return qmul(Q[I[:, 1]], synth.qconj(Q[I[:, 0]]))


def graph(name, I, n_total=None, threshold=0.1, seed=0, noise=0.0, QQ=None):
    I = np.array(I, dtype=np.int32).reshape(-1, 2)
    n_total = int(I.max()) + 1 if n_total is None else n_total
    if QQ is None:
        rng = np.random.default_rng([seed, len(I)])
        ids, inv = np.unique(I, return_inverse=True)       # (rotations for the ids in use: n_total may be 2^31 - 1)
        QQ = measured(unit(rng, len(ids)), inv.reshape(-1, 2))
        if noise:
            QQ = qmul(synth.qexp(rng.normal(scale=noise, size=(len(I), 3))), QQ)
    return dict(name=name, I=I, QQ=np.ascontiguousarray(QQ, dtype=np.float64), n_total=n_total, threshold=threshold)


def book(d, extra):
    """hubs 0 and 1 joined, d common neighbours, `extra` private neighbours of hub 0 on both sides of them in id order"""
    I = [(0, 1)]
    for c in range(d):
        v = 2 + extra // 2 + c
        I += [(0, v), (v, 1) if c % 4 == 0 else (1, v)]       # (both ways round: either end of a spoke may be the hub)
    I += [(0, 2 + p if p < extra // 2 else 2 + d + p) for p in range(extra)]
    return graph("book%d+%d" % (d, extra), I, n_total=2 + d + extra, threshold=1e-6, seed=d)


# exact unit quaternions (the 24-cell): their products are exact, and they do not commute
EXACT = np.array([(.5, .5, .5, .5), (.5, -.5, .5, .5), (0, 1.0, 0, 0)])


# ---- known answers -----------------------------------------------------------------------------------------------------------
def test_a_consistent_triangle():
    I = np.array([(0, 1), (1, 2), (2, 0)], dtype=np.int32)
    g = graph("triangle", I, QQ=measured(EXACT, I))
    r = run_dev(g)
    assert r["tri_count"].tolist() == [1, 1, 1] and r["tri_ok"].tolist() == [1, 1, 1]
    print("tri_min", r["tri_min"])
    assert (r["tri_min"] <= 4e-16).all()
    assert r["summary"] == dict(triangles=3, supported=3, contradicted=0, untested=0)
    assert_matches(g, r)


def test_a_reversed_a_negated_and_a_turned_edge():
    I = np.array([(0, 1), (2, 1), (2, 0)], dtype=np.int32)       # the second edge stored as (b, a)
    QQ = measured(EXACT, I)
    QQ[2] = -QQ[2]
    QQ[0] = qmul(turn(0.3), QQ[0])
    g = graph("triangle-turned", I, QQ=QQ)
    r = run_dev(g)
    print("tri_min - 0.3", r["tri_min"] - 0.3)
    assert r["tri_count"].tolist() == [1, 1, 1] and r["tri_ok"].tolist() == [0, 0, 0]
    assert (np.abs(r["tri_min"] - 0.3) <= 2e-16).all()
    assert r["summary"] == dict(triangles=3, supported=0, contradicted=3, untested=0)
    assert_matches(g, r)


def test_the_golden_fixture_has_no_triangle():
    f = graphio.read_ravg_input(os.path.join(ROOT, "tests", "golden", "ravg_input.txt"))
    d = f["I"][:, 1].astype(np.int64) - f["I"][:, 0]
    assert len(f["I"]) == 3655 and set(np.abs(d).tolist()) == {4, 5}
    g = graph("golden", f["I"], n_total=f["n"], QQ=f["QQ"])
    r = run_dev(g)
    assert (r["tri_count"] == 0).all() and (r["tri_ok"] == 0).all() and np.isposinf(r["tri_min"]).all()
    assert r["summary"] == dict(triangles=0, supported=0, contradicted=0, untested=3655)


@pytest.fixture(scope="module")
def planted():
    S = synth.make_graph(2000, 10000, sigma_n=0, p_out=0, seed=3)
    I, QQ = S["I"], S["QQ"].copy()
    vs = np.arange(40, 1921, 40)
    sel = np.array([np.flatnonzero((I[:, 0] == v - 2) & (I[:, 1] == v))[0] for v in vs])
    assert len(sel) == 48
    QQ[sel] = qmul(turn(0.3), QQ[sel])
    return graph("planted", I, n_total=2000, threshold=0.1, QQ=QQ), sel


def test_planted_outliers_are_exactly_the_contradicted_edges(planted):
    g, sel = planted
    r = run_dev(g)
    assert_matches(g, r)
    assert r["summary"]["triangles"] == 60105 and r["tri_count"].min() == 4 and r["tri_count"].max() == 9
    contradicted = np.flatnonzero((r["tri_count"] >= 1) & (r["tri_ok"] == 0))
    assert sorted(contradicted.tolist()) == sorted(sel.tolist())
    others = np.setdiff1d(np.arange(len(g["I"])), sel)
    print("largest tri_min of an edge that was not turned: %.3e" % r["tri_min"][others].max())
    assert (r["tri_min"][others] < 1e-15).all()
    assert r["summary"]["untested"] == 0 and r["summary"]["contradicted"] == 48


# ---- branches of the definition ------------------------------------------------------------------------------------------------
K4 = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
BRANCHES = [
    (graph("self-loops", [(0, 1), (1, 2), (2, 0), (1, 1), (5, 5), (0, 0)], n_total=7), [1, 1, 1, 0, 0, 0]),
    (graph("parallel", [(0, 1), (1, 2), (2, 0), (0, 1)]), [1, 2, 2, 1]),
    (graph("parallel-reversed", [(0, 1), (1, 2), (2, 0), (1, 0)]), [1, 2, 2, 1]),
    (graph("path", [(0, 1), (1, 2), (2, 3), (3, 4)]), [0, 0, 0, 0]),
    (graph("k4", K4), [2] * 6),
    (graph("unused-id", [(0, 1), (1, 3), (3, 0)], n_total=9), [1, 1, 1]),
    (graph("n-total-3", [(2, 1), (0, 2), (0, 1)], n_total=3), [1, 1, 1]),
]


@pytest.mark.parametrize("g,counts", BRANCHES, ids=[b[0]["name"] for b in BRANCHES])
def test_branches_of_the_definition(g, counts):
    r = run_dev(g)
    assert r["tri_count"].tolist() == counts
    assert_matches(g, r)
    loops = g["I"][:, 0] == g["I"][:, 1]
    assert (r["tri_count"][loops] == 0).all() and (r["tri_ok"][loops] == 0).all() and np.isposinf(r["tri_min"][loops]).all()
    assert (r["tri_ok"] == r["tri_count"]).all()                  # consistent measurements: every triangle is ok


def test_a_nan_row_counts_is_never_ok_and_leaves_the_minimum_alone():
    g = graph("nan-row", [(0, 1), (1, 2), (2, 0), (2, 3), (3, 0)], threshold=INF)
    QQ = g["QQ"].copy()
    QQ[1, 0] = np.nan
    g = dict(g, QQ=QQ)
    r = run_dev(g)
    assert r["tri_count"].tolist() == [1, 1, 2, 1, 1] and r["tri_ok"].tolist() == [0, 0, 1, 1, 1]
    assert np.isposinf(r["tri_min"][:2]).all() and (r["tri_min"][2:] <= TOL_MIN).all()
    assert r["summary"] == dict(triangles=6, supported=3, contradicted=2, untested=0)
    assert_matches(g, r)


# ---- where the kernel can go wrong ---------------------------------------------------------------------------------------------
DS = [7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 2000]


@pytest.fixture(params=[8, 16, 32, 64], ids=lambda w: "G%d" % w)
def every_width(request):
    """the triangle kernel with every group width it is compiled for (no result depends on it)"""
    old = capi.cycle_check_group(request.param)
    yield request.param
    capi.cycle_check_group(old)


@pytest.mark.parametrize("extra", [False, True], ids=["plain", "private"])
def test_book_graphs(every_width, extra):
    for d in DS:
        g = book(d, d if extra else 0)
        r = run_dev(g)
        assert r["tri_count"][0] == d and (r["tri_count"][1:2 * d + 1] == 1).all() and (r["tri_count"][2 * d + 1:] == 0).all()
        assert_matches(g, r, "G%d" % every_width)


def test_a_star_with_rim_edges(every_width):
    n = 5000
    I = [(0, v) if v % 50 else (v, 0) for v in range(1, n + 1)] + [(v, v + 1) for v in range(1, n, 2)]
    g = graph("star", I, threshold=1e-6)
    r = run_dev(g)
    assert (r["tri_count"][:n] == 1).all() and (r["tri_count"][n:] == 1).all()
    assert_matches(g, r, "G%d" % every_width)


def band(m_target, seed, noise=0.0, turned=0.0, shuffle=False, threshold=0.1):
    n = max(m_target // 5, 2)
    S = synth.make_graph(n, m_target, sigma_n=noise, p_out=0, seed=seed) if m_target >= 10 else None
    if S is None:
        return graph("m%d" % m_target, [(0, 1)] * m_target, seed=seed)
    I, QQ = S["I"], S["QQ"].copy()
    rng = np.random.default_rng(seed)
    if turned:
        bad = rng.choice(len(I), size=int(round(turned * len(I))), replace=False)
        axis = unit(rng, len(bad))                               # 0.3 rad about a random axis
        QQ[bad] = qmul(qmul(qmul(axis, turn(0.3)[None, :]), synth.qconj(axis)), QQ[bad])
    if shuffle:
        p = rng.permutation(len(I))
        I, QQ = I[p], QQ[p]
        flip = rng.random(len(I)) < 0.5
        I = np.where(flip[:, None], I[:, ::-1], I)
        QQ = against(QQ, flip)
    return graph("band%d-%d" % (len(I), seed), I, n_total=n, threshold=threshold, QQ=QQ)


@pytest.mark.parametrize("m", [1, 255, 256, 257, 10007])
def test_edge_counts_around_a_workgroup_pass(every_width, m):
    g = band(m, seed=m)
    assert len(g["I"]) == m
    r = run_dev(g)
    assert_matches(g, r, "G%d" % every_width)
    assert m < 10 or r["summary"]["triangles"] > m


def raw_call(ei, qq, n_total, threshold, outs):
    """the C call on tensors that exist already: nothing is allocated on this side of it"""
    s = (C.c_int64 * 4)()
    rc = capi.lib().irotavg_cycle_check_dev(len(ei), n_total, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1,
                                            threshold, *[C.c_void_p(t.data_ptr()) for t in outs], s,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, dict(zip(capi.SUMMARY_FIELDS, (int(v) for v in s)))


def test_ids_at_the_top_of_the_range_cost_no_memory():
    big = [0, 1, 2 ** 30, 2 ** 31 - 3, 2 ** 31 - 2]
    pairs = [(0, 4), (4, 3), (3, 0), (2, 4), (3, 2), (1, 2)]
    g = graph("top-ids", [(big[a], big[b]) for a, b in pairs], n_total=2 ** 31 - 1, threshold=1e-6)
    ei_small, ei, qq = t32(pairs), t32(g["I"]), t64(g["QQ"])
    outs = [torch.zeros(6, dtype=torch.int32, device=dev()), torch.zeros(6, dtype=torch.int32, device=dev()),
            torch.zeros(6, dtype=torch.float64, device=dev())]
    # the same six edges among five views first: the code objects are loaded and the blocks that six edges need are in
    # the pool before the baseline is read. The first call with n_total = 2^31 - 1 comes after it.
    assert raw_call(ei_small, qq, 5, g["threshold"], outs)[0] == capi.OK
    small_counts = outs[0].cpu().numpy().copy()
    free0 = torch.cuda.mem_get_info()[0]
    rc, summary = raw_call(ei, qq, g["n_total"], g["threshold"], outs)
    free1 = torch.cuda.mem_get_info()[0]
    print("device memory taken by the first call with n_total = 2^31 - 1: %d bytes" % (free0 - free1))
    assert rc == capi.OK
    r = dict(tri_count=outs[0].cpu().numpy(), tri_ok=outs[1].cpu().numpy(), tri_min=outs[2].cpu().numpy(), summary=summary)
    assert r["tri_count"].tolist() == [1, 2, 1, 1, 1, 0] and (small_counts == r["tri_count"]).all()
    assert_matches(g, r)
    # Six edges need well under a megabyte (12 keys and values twice, the sort's storage, a few sums); a block the pool
    # does not hold yet comes from the driver in steps of a few MB at the most. One BIT per view would be 256 MiB.
    assert free0 - free1 <= 8 * 2 ** 20
    ids_small = dict(g, n_total=2 ** 31 - 2)                      # the largest id is now one too many
    assert torch_api.cycle_check(t32(ids_small["I"]), t64(ids_small["QQ"]), ids_small["n_total"], 0.1,
                                 allow_rc=(capi.ERR_BAD_ARG,))["rc"] == capi.ERR_BAD_ARG


@pytest.fixture(scope="module")
def noisy():
    # 2 % of the edges turned by 0.3 rad about a random axis, noise of 1e-3 rad: the errors cluster below 1e-2 and around
    # 0.3, the threshold lies between
    return band(10000, seed=11, noise=1e-3, turned=0.02, shuffle=True, threshold=0.1)


def test_a_noisy_shuffled_band_graph(noisy, every_width):
    r = run_dev(noisy)
    assert_matches(noisy, r, "G%d" % every_width)
    assert r["summary"]["contradicted"] > 0 and r["summary"]["supported"] > 9000


# ---- interface ---------------------------------------------------------------------------------------------------------------
def as_bytes(r):
    return (r["tri_count"].tobytes(), r["tri_ok"].tobytes(), r["tri_min"].tobytes(), tuple(sorted(r["summary"].items())))


def test_the_device_form_is_bitwise_the_host_call_and_two_calls_agree(noisy):
    a, b = run_dev(noisy), run_dev(noisy)
    h = capi.cycle_check(noisy["I"], noisy["QQ"], noisy["n_total"], noisy["threshold"])
    assert as_bytes(a) == as_bytes(b) == as_bytes(h)
    assert_matches(noisy, h, "host form")


def strided(QQ, form):
    m = len(QQ)
    if form == "aos":
        return t64(QQ)
    if form == "planes":
        return t64(QQ.T).t()
    if form == "generic":                                          # rows of 6, an odd offset: no 16-byte rows
        return t64(np.zeros(6 * m + 1))[1:].view(m, 6)[:, :4].copy_(t64(QQ))
    if form == "negative":                                         # torch has no negative strides: the C call below takes them
        return t64(QQ[::-1])
    if form == "column-slice":
        return t64(np.zeros((m, 9)))[:, 3:7].copy_(t64(QQ))
    raise ValueError(form)


@pytest.mark.parametrize("form", ["aos", "planes", "generic", "negative", "column-slice"])
def test_every_stride_form_of_qq(noisy, form):
    g = noisy
    m = len(g["I"])
    want = run_dev(g)
    q = strided(g["QQ"], form)
    if form != "negative":
        r = torch_api.cycle_check(t32(g["I"]), q, g["n_total"], g["threshold"])
        got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    else:                                                          # the last row first: rs = -4 from the last row's address
        ei = t32(g["I"])
        outs = [torch.empty(m, dtype=torch.int32, device=dev()), torch.empty(m, dtype=torch.int32, device=dev()),
                torch.empty(m, dtype=torch.float64, device=dev())]
        s = (C.c_int64 * 4)()
        rc = capi.lib().irotavg_cycle_check_dev(m, g["n_total"], C.c_void_p(ei.data_ptr()),
                                                C.c_void_p(q.data_ptr() + 32 * (m - 1)), -4, 1, g["threshold"],
                                                *[C.c_void_p(t.data_ptr()) for t in outs], s,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == capi.OK
        got = dict(tri_count=outs[0].cpu().numpy(), tri_ok=outs[1].cpu().numpy(), tri_min=outs[2].cpu().numpy(),
                   summary=dict(zip(capi.SUMMARY_FIELDS, (int(v) for v in s))))
    assert as_bytes(got) == as_bytes(want)


def test_int64_ids(noisy):
    g = noisy
    r = torch_api.cycle_check(torch.tensor(g["I"], dtype=torch.int64, device=dev()), t64(g["QQ"]), g["n_total"], g["threshold"])
    got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    assert as_bytes(got) == as_bytes(run_dev(g))
    bad = torch.tensor(g["I"], dtype=torch.int64, device=dev())
    bad[5, 1] = 2 ** 32 + 3                                        # a value that would wrap into the range
    assert torch_api.cycle_check(bad, t64(g["QQ"]), g["n_total"], allow_rc=(capi.ERR_BAD_ARG,))["rc"] == capi.ERR_BAD_ARG


@pytest.mark.parametrize("mask", range(16))
def test_every_combination_of_null_outputs(noisy, mask):
    g = noisy
    want = run_dev(g)
    r = run_dev(g, count=bool(mask & 1), ok=bool(mask & 2), min_err=bool(mask & 4), summary=bool(mask & 8))
    assert r["rc"] == capi.OK
    for bit, key in ((1, "tri_count"), (2, "tri_ok"), (4, "tri_min"), (8, "summary")):
        if mask & bit:
            assert (r[key] == want[key]) if key == "summary" else r[key].tobytes() == want[key].tobytes()
        else:
            assert r[key] is None


def test_a_bad_id_in_the_last_edge_leaves_every_output_byte(noisy):
    g = noisy
    m = len(g["I"])
    for bad in (-1, g["n_total"], 2 ** 31 - 1):
        I = g["I"].copy()
        I[-1, 1] = bad
        cnt = torch.full((m,), -7, dtype=torch.int32, device=dev())
        ok = torch.full((m,), -8, dtype=torch.int32, device=dev())
        mn = torch.full((m,), -9.0, dtype=torch.float64, device=dev())
        r = torch_api.cycle_check(t32(I), t64(g["QQ"]), g["n_total"], g["threshold"], count=cnt, ok=ok, min_err=mn,
                                  allow_rc=(capi.ERR_BAD_ARG,))
        torch.cuda.synchronize()
        assert r["rc"] == capi.ERR_BAD_ARG and r["summary"] is None
        assert (cnt == -7).all() and (ok == -8).all() and (mn == -9.0).all()
        s = (C.c_int64 * 4)(-1, -2, -3, -4)
        ei, qq = t32(I), t64(g["QQ"])
        rc = capi.lib().irotavg_cycle_check_dev(m, g["n_total"], C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1,
                                                g["threshold"], None, None, None, s, None)
        assert rc == capi.ERR_BAD_ARG and list(s) == [-1, -2, -3, -4]
        h = capi.cycle_check(I, g["QQ"], g["n_total"], g["threshold"], allow_rc=(capi.ERR_BAD_ARG,))
        assert h["rc"] == capi.ERR_BAD_ARG and (h["tri_count"] == -1).all() and (h["tri_ok"] == -1).all() and \
            np.isnan(h["tri_min"]).all()
    # the id check alone, and a valid call afterwards
    ei, qq = t32(g["I"]), t64(g["QQ"])
    assert capi.lib().irotavg_cycle_check_dev(m, g["n_total"], C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1,
                                              g["threshold"], None, None, None, None, None) == capi.OK
    assert_matches(g, run_dev(g))


def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream(noisy):
    g = noisy
    want = run_dev(g)
    ei, half = t32(g["I"]), t64(g["QQ"] * 0.5)
    big = torch.ones(1 << 25, dtype=torch.float64, device=dev())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = big
        for _ in range(16):                                       # keeps the stream busy while the call is made
            busy = busy * 1.5
        qq = half * 2.0                                           # exact: the inputs of the synchronised run, produced on the stream
        r = torch_api.cycle_check(ei, qq, g["n_total"], g["threshold"])
        doubled = r["tri_count"] * 2                              # consumed right behind the call, no synchronise
    side.synchronize()
    got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    assert as_bytes(got) == as_bytes(want)
    assert (doubled.cpu().numpy() == 2 * want["tri_count"]).all()


def test_the_handle_method_passes_its_own_n_total(noisy):
    g = noisy
    ei, qq = t32(g["I"]), t64(g["QQ"])
    G = torch_api.TorchGraph(ei, qq, g["n_total"], 1)
    try:
        r = G.cycle_check(ei, qq, g["threshold"])
    finally:
        G.close()
    got = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}
    assert as_bytes(got) == as_bytes(run_dev(g))
