"""irotavg_cycle_check4 / irotavg_cycle_check4_dev (irotavg_amd/csrc/cycles4.hip, cycles4.hpp, devapi.hip;
torch_api.cycle_check4; docs/cycle_check.md, "Four-cycles"): the four-cycle test of the edges listed, on the device.

The reference is the definition restated here: quadrilaterals enumerated from Python dictionaries, their errors in
np.longdouble in the definition's association, independent of cycles4.hpp. Counts and the summary must be equal, quad_min
within 1e-12 rad (the triangle test's bound: one more product, still a few eps), quad_ok equal on the asserted condition
that no reference error lies within 1e-9 of the threshold. The shapes are the smallest at which each part can go wrong."""
import numpy as np
import pytest
import torch

from irotavg_amd import capi, synth, torch_api

pytestmark = pytest.mark.gpu
INF, TOL_MIN, GAP = float("inf"), 1e-12, 1e-9
KEYS = ("quad_count", "quad_ok", "quad_min")


def on_dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=torch.device("cuda", torch.cuda.current_device()))


def qmul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def reference(I, QQ, threshold, sub):
    out, between = {}, {}
    for k, (a, b) in enumerate(I.tolist()):
        if a != b:
            out.setdefault(a, []).append((b, k, False))
            out.setdefault(b, []).append((a, k, True))
            between.setdefault((a, b), []).append((k, False))
            between.setdefault((b, a), []).append((k, True))
    T = []                                                            # (entry, k, k1, against, k2, against, k3, against)
    for t, k in enumerate(sub):
        a, b = I[k].tolist()
        T += [(t, k, k1, g1, k2, g2, k3, g3) for c, k1, g1 in out.get(b, ()) if a != b and c != a
              for d, k2, g2 in out[c] if d not in (a, b) for k3, g3 in between.get((d, a), ())]
    T = np.array(T, dtype=np.int64).reshape(-1, 8)
    L = QQ.astype(np.longdouble)
    q = [L[T[:, 1]]] + [np.where((T[:, j + 1] != 0)[:, None], L[T[:, j]] * np.array([1, 1, 1, -1]), L[T[:, j]]) for j in (2, 4, 6)]
    with np.errstate(invalid="ignore"):
        d = qmul(q[3], qmul(q[2], qmul(q[1], q[0])))
        th = 2 * np.arctan2(np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + d[:, 2] ** 2), d[:, 3])
        pi = np.arctan2(np.longdouble(0), np.longdouble(-1))
        err = np.abs(np.where(th >= pi, th - 2 * pi, th)).astype(np.float64)
        assert not (np.abs(err[np.isfinite(err)] - threshold) < GAP).any(), "the threshold is not in a gap"
        ok = err <= threshold
    ne = len(sub)
    count, nok, mn = np.bincount(T[:, 0], minlength=ne), np.bincount(T[ok, 0], minlength=ne), np.full(ne, INF)
    np.minimum.at(mn, T[np.isfinite(err), 0], err[np.isfinite(err)])
    return dict(quad_count=count, quad_ok=nok, quad_min=mn,
                summary=dict(quadrilaterals=int(count.sum()), supported=int((nok >= 1).sum()),
                             contradicted=int(((count >= 1) & (nok == 0)).sum()), untested=int((count == 0).sum())))


def run(g, sub=None, **kw):
    r = torch_api.cycle_check4(on_dev(g["I"], torch.int32), on_dev(g["QQ"], torch.float64), g["n"], g["th"],
                               None if sub is None else on_dev(sub, torch.int32), **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def check(g, sub=None, what=""):
    r, e = run(g, sub), reference(g["I"], g["QQ"], g["th"], range(len(g["I"])) if sub is None else sub)
    has = np.isfinite(e["quad_min"])
    diff = np.abs(r["quad_min"][has] - e["quad_min"][has]).max() if has.any() else 0.0
    print("%s %s: %d quadrilaterals, max |quad_min - reference| = %.3e" % (g["name"], what, e["summary"]["quadrilaterals"], diff))
    assert (r["quad_count"] == e["quad_count"]).all() and (r["quad_ok"] == e["quad_ok"]).all() and r["summary"] == e["summary"], what
    assert (r["quad_min"][~has] == INF).all() and diff <= TOL_MIN, what
    return r


def as_bytes(r):
    return tuple(r[k].tobytes() for k in KEYS) + (tuple(sorted(r["summary"].items())),)


def graph(name, I, th=0.1, n=None, seed=0):
    """consistent measurements Q_b (x) inverse(Q_a) of random rotations of the ids in use"""
    I = np.array(I, dtype=np.int32).reshape(-1, 2)
    ids, inv = np.unique(I, return_inverse=True)
    Q = np.random.default_rng([seed, len(I)]).normal(size=(len(ids), 4))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    inv = inv.reshape(-1, 2)
    return dict(name=name, I=I, QQ=qmul(Q[inv[:, 1]], synth.qconj(Q[inv[:, 0]])), n=int(I.max()) + 1 if n is None else n, th=th)


def turned(g, k, angle=0.3):
    QQ = g["QQ"].copy()
    QQ[k] = qmul(np.array([np.sin(angle / 2), 0, 0, np.cos(angle / 2)]), QQ[k])
    return dict(g, QQ=QQ)


SQUARE, K4 = [(0, 1), (1, 2), (2, 3), (3, 0)], [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
COUNTS = [(graph("square", SQUARE), [1, 1, 1, 1]), (graph("triangle", [(0, 1), (1, 2), (2, 0)]), [0, 0, 0]),
          (graph("diagonal", SQUARE + [(0, 2)]), [1, 1, 1, 1, 0]), (graph("self-loops", SQUARE + [(1, 1), (5, 5)], n=7), [1, 1, 1, 1, 0, 0]),
          (graph("parallel", SQUARE + [(0, 1), (1, 0), (1, 2)]), [2, 3, 6, 6, 2, 2, 3]), (graph("k4", K4), [2] * 6)]


@pytest.mark.parametrize("g,counts", COUNTS, ids=[c[0]["name"] for c in COUNTS])
def test_known_counts(g, counts):
    r = check(g)
    assert r["quad_count"].tolist() == counts and (r["quad_ok"] == r["quad_count"]).all()
    assert (r["quad_min"][r["quad_count"] > 0] <= 1e-15).all()


def test_a_reversed_a_negated_and_a_turned_edge_and_a_nan_row():
    g = turned(graph("square-turned", [(0, 1), (2, 1), (2, 3), (3, 0)]), 0)     # the second edge stored as (b, a)
    g["QQ"][2] = -g["QQ"][2]
    r = check(g)
    assert r["quad_ok"].tolist() == [0] * 4 and (np.abs(r["quad_min"] - 0.3) <= 4e-16).all(), r["quad_min"] - 0.3
    g = graph("k4-nan", K4, th=INF)
    g["QQ"][3, 0] = np.nan                 # edge (1, 2): both quadrilaterals of the opposite edge (0, 3) pass it
    r = check(g)
    assert r["quad_count"].tolist() == [2] * 6 and r["quad_ok"].tolist() == [1, 1, 0, 0, 1, 1] and (r["quad_min"][2:4] == INF).all()


def bipartite(ra, rb, swap=False):
    """edge 0 = (0, 1); ra further neighbours of view 0, rb of view 1, every one of the former joined to every one of the latter"""
    A, B = range(2, 2 + ra), range(2 + ra, 2 + ra + rb)
    return [(1, 0) if swap else (0, 1)] + [(0, i) for i in A] + [(j, 1) for j in B] + [(i, j) for i in A for j in B]


@pytest.mark.parametrize("r", [7, 8, 9, 15, 16, 17, 63, 64, 65])
def test_complete_bipartite_neighbourhoods_at_every_width(r):
    for ra, rb, swap in ((r, r + 1, False), (r + 1, r, False), (r, r + 1, True)):
        g = graph("bipartite%dx%d" % (ra, rb), bipartite(ra, rb, swap), th=1e-6, seed=r)
        sub, got = [0, 1, ra + 1, len(g["I"]) - 1, r], []             # the edge, a spoke of either end, cross edges
        for w in (8, 16, 32, 64):
            old = capi.cycle_check4_group(w)
            try:
                got.append(run(g, sub) if got else check(g, sub, "S%d" % w))     # (one reference per graph)
            finally:
                capi.cycle_check4_group(old)
        assert got[0]["quad_count"].tolist() == [ra * rb] * 5 and all(as_bytes(x) == as_bytes(got[0]) for x in got)


@pytest.mark.parametrize("swap", [False, True], ids=["x=b", "x=a"])
@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_the_staging_boundary(n, swap):
    """view 0 has n neighbours, view 1 has three: 0, p and q, which reach the first, the last and a few other neighbours of 0;
    edge 0 stored as (1, 0) walks row a and searches row b, staged or not"""
    p, q = n + 1, n + 2
    far = [2, 3, n // 2, n - 1, n]
    g = graph("stage%d" % n, [(1, 0) if swap else (0, 1)] + [(0, v) for v in range(2, n + 1)] + [(1, p), (q, 1)] + [(p, v) for v in far] + [(v, q) for v in far[::2]],
              th=1e-6)
    sub = [0, n, n + 1, 1, len(g["I"]) - 1]
    r = check(g, sub)
    assert r["quad_count"][0] == 8
    h = capi.cycle_check4(g["I"], g["QQ"], g["n"], g["th"], sub)
    assert as_bytes(h) == as_bytes(r)


def band_with_closures(n=300):
    I = [(v - s, v) for v in range(1, n) for s in range(1, 5) if v - s >= 0]
    m0 = len(I)
    for a, b in ((3, 150), (30, 200), (60, 250), (90, 280), (110, 230), (10, 120)):
        I += [(a, b), (b + 1, a + 1)]
    return turned(graph("band", I), m0 + 4), m0                       # one closure of the third pair is off by 0.3 rad


@pytest.mark.parametrize("ne", [3, 4, 5, 8, 9])
def test_subsets_around_a_workgroup_pass(ne):
    g, m0 = band_with_closures()
    g = dict(g, I=np.concatenate([g["I"], [(7, 7)]]).astype(np.int32), QQ=np.concatenate([g["QQ"], [[0, 0, 0, 1.0]]]))
    sub = [m0 + 11, m0 + 4, len(g["I"]) - 1, m0 + 4, 17, m0, 500, m0 + 5, 2][:ne]    # out of order, a duplicate, a self loop
    r = check(g, sub)
    assert r["quad_count"][2] == 0 and abs(r["quad_min"][1] - 0.3) < 1e-15 and (ne < 4 or r["quad_min"][3] == r["quad_min"][1])


def test_closures_of_a_band_graph_are_screened_and_the_tree_avoids_the_contradicted():
    g, m0 = band_with_closures()
    ei, qq = on_dev(g["I"], torch.int32), on_dev(g["QQ"], torch.float64)
    t = torch_api.cycle_check(ei, qq, g["n"], g["th"])
    sub = torch.nonzero(t["tri_count"] == 0).flatten()
    assert sub.tolist() == list(range(m0, m0 + 12))
    r = torch_api.cycle_check4(ei, qq, g["n"], g["th"], sub)
    assert r["summary"] == dict(quadrilaterals=12, supported=10, contradicted=2, untested=0)
    assert torch.nonzero(r["quad_ok"] == 0).flatten().tolist() == [4, 5]
    check(g, sub.cpu().numpy())
    count, ok = t["tri_count"].clone(), t["tri_ok"].clone()
    count[sub] += r["quad_count"]
    ok[sub] += r["quad_ok"]
    rank = torch_api.rank_from_cycle_check(count, ok)
    assert rank[m0:].tolist() == [0, 0, 0, 0, 2, 2, 0, 0, 0, 0, 0, 0] and (rank[:m0] == 0).all()
    Q = torch.zeros((g["n"], 4), dtype=torch.float64, device=ei.device)
    Q[:, 3] = 1
    tree = torch_api.init_tree(ei, qq, g["n"], Q, rank=rank, in_tree=True)["in_tree"]
    assert int(tree.sum()) == g["n"] - 1 and int(tree[rank == 2].sum()) == 0


# ---- interface ---------------------------------------------------------------------------------------------------------------
def test_ids_at_the_top_of_the_range_strides_and_a_second_call():
    big = np.array([0, 1, 2 ** 30, 2 ** 31 - 3, 2 ** 31 - 2])
    g = graph("top-ids", big[np.array(K4 + [(4, 0), (2, 4)])], th=1e-6, n=2 ** 31 - 1)
    want = check(g)
    assert want["quad_count"].tolist() == [3, 2, 3, 3, 2, 3, 2, 2] and as_bytes(run(g)) == as_bytes(want)
    assert as_bytes(capi.cycle_check4(g["I"], g["QQ"], g["n"], g["th"])) == as_bytes(want)
    ei, m = on_dev(g["I"], torch.int64), len(g["I"])
    planes = on_dev(g["QQ"].T, torch.float64).t()
    wide = on_dev(np.zeros((m, 9)), torch.float64)[:, 3:7].copy_(planes)
    for qq in (planes, wide):
        r = torch_api.cycle_check4(ei, qq, g["n"], g["th"], torch.arange(m, device=ei.device))
        assert as_bytes({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}) == as_bytes(want)
    assert run(dict(g, n=2 ** 31 - 2), allow_rc=(capi.ERR_BAD_ARG,))["rc"] == capi.ERR_BAD_ARG


def test_bad_ids_leave_every_output_byte_and_null_outputs_are_the_id_check():
    g, m0 = band_with_closures()
    sub = np.arange(m0, m0 + 12)
    bad_view = g["I"].copy()
    bad_view[-1, 1] = g["n"]
    for I, s in ((bad_view, sub), (g["I"], np.append(sub, len(g["I"]))), (g["I"], np.append(-1, sub)), (g["I"], sub)):
        outs = [on_dev(np.full(len(s), -7), torch.int32), on_dev(np.full(len(s), -8), torch.int32), on_dev(np.full(len(s), -9.0), torch.float64)]
        ok = s is sub and I is g["I"]
        for kw in (dict(count=outs[0], ok=outs[1], min_err=outs[2]), dict(count=None, ok=None, min_err=None, summary=False)):
            r = torch_api.cycle_check4(on_dev(I, torch.int32), on_dev(g["QQ"], torch.float64), g["n"], g["th"], on_dev(s, torch.int32),
                                       allow_rc=(capi.ERR_BAD_ARG,), **kw)
            assert r["rc"] == (capi.OK if ok else capi.ERR_BAD_ARG) and (ok and kw["count"] is not None) == (r["summary"] is not None)
        assert ok or ((outs[0] == -7).all() and (outs[1] == -8).all() and (outs[2] == -9.0).all())
        h = capi.cycle_check4(I, g["QQ"], g["n"], g["th"], s, allow_rc=(capi.ERR_BAD_ARG,))
        assert ok or (h["rc"] == capi.ERR_BAD_ARG and (h["quad_count"] == -1).all() and np.isnan(h["quad_min"]).all())


def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream():
    g, m0 = band_with_closures()
    want = run(g, np.arange(m0, m0 + 12))
    ei, half, sub = on_dev(g["I"], torch.int32), on_dev(g["QQ"] * 0.5, torch.float64), on_dev(np.arange(m0, m0 + 12), torch.int32)
    busy = torch.ones(1 << 24, dtype=torch.float64, device=ei.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(8):                                            # keeps the stream busy while the call is made
            busy = busy * 1.5
        r = torch_api.cycle_check4(ei, half * 2.0, g["n"], g["th"], sub)    # exact: the inputs of the synchronised run
        doubled = r["quad_count"] * 2                                 # consumed right behind the call, no synchronise
    side.synchronize()
    assert as_bytes({k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}) == as_bytes(want)
    assert (doubled.cpu().numpy() == 2 * want["quad_count"]).all()
