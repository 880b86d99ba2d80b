"""irotavg_init_tree / irotavg_init_tree_dev (irotavg_amd/csrc/treeinit.hip, treeinit.hpp, devapi.hip;
torch_api.init_tree, TorchGraph.init_tree, rank_from_cycle_check; docs/init_tree.md): the order-free spanning-tree
initialiser on the device.

The reference is written here, independent of treeinit.hpp: Kruskal on the keys (rank, k) with a union-find for the tree,
and a breadth-first propagation from view 0 along it in np.longdouble for the rows. Every shape checks four things
(check): (a) in_tree equals Kruskal's set exactly; (b) every free row is within TOL(n_total) of the reference's by the
angular distance 2 acos |<q, q'>|; (c) the rows below f are byte-identical to the input; (d) a second call gives the same
bytes and the host form is bitwise the device form.

Tolerance, derived and not measured: a row is a product of at most 2 (n_total - 1) factors (the path to the final
representative and back to view 0), each product perturbs the angle by a few eps: 64 n_total 2.2e-16 rad, which is 2.8e-11
or less at n_total <= 2000. The angular distance is evaluated as the angle of q (x) q'^-1, 2 atan2(|v|, |w|) in
np.longdouble: the same angle as 2 acos |<q, q'>|, but acos cannot resolve anything below 1e-8 rad next to 1
(synth.angular_distance says the same of its chord form).

The ruler path: the issue that asked for this test expected 9 rounds for 300 views. Components at least halve per round --
an odd one out has an edge that leaves it and joins in the same round -- so 300 -> 150 -> 75 -> 37 -> 18 -> 9 -> 4 -> 2 -> 1
and eight rounds are the most 300 views can take; the test asserts 8, the sequence the reference's own round count gives."""
import ctypes as C

import numpy as np
import pytest
import torch

from irotavg_amd import capi, ral, synth, torch_api

pytestmark = pytest.mark.gpu
LD = np.longdouble


def TOL(n_total):
    return 64 * n_total * 2.2e-16


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


def angle(p, q):
    """the angular distance of quaternion rows, in long double: the angle of p (x) q^-1"""
    p, q = np.asarray(p, dtype=LD), np.asarray(q, dtype=LD)
    d = qmul(p, q * np.array([-1, -1, -1, 1], dtype=LD))
    return (2 * np.arctan2(np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2 + d[..., 2] ** 2), np.abs(d[..., 3]))).astype(np.float64)


def kruskal(I, rank, n_total):
    """(in_tree, components left, tree edges with rank > 0, largest rank in the tree, Boruvka rounds) under (rank, k)"""
    m = len(I)
    rank = np.zeros(m, dtype=np.int64) if rank is None else np.asarray(rank, dtype=np.int64)
    usable = (rank >= 0) & (I[:, 0] != I[:, 1])
    order = [k for k in np.lexsort((np.arange(m), rank)).tolist() if usable[k]]
    parent = list(range(n_total))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    E = I.tolist()
    in_tree = np.zeros(m, dtype=np.int32)
    comps = n_total
    for k in order:
        ra, rb = find(E[k][0]), find(E[k][1])
        if ra != rb:
            parent[ra] = rb
            in_tree[k] = 1
            comps -= 1
    picked = rank[in_tree == 1]
    # the rounds, on labels of their own: every component picks its smallest key to another one, all picks join
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    a, b = I[:, 0].astype(np.int64), I[:, 1].astype(np.int64)
    key = (rank.astype(np.uint64) << np.uint64(32)) | np.arange(m, dtype=np.uint64)
    none = np.uint64(2 ** 64 - 1)
    lab = np.arange(n_total)
    rounds = 0
    while True:
        la, lb = lab[a], lab[b]
        act = usable & (la != lb)
        if not act.any():
            break
        best = np.full(n_total, none, dtype=np.uint64)
        np.minimum.at(best, la[act], key[act])
        np.minimum.at(best, lb[act], key[act])
        ks = np.unique((best[best != none] & np.uint64(0xffffffff)).astype(np.int64))
        _, new = connected_components(coo_matrix((np.ones(len(ks)), (la[ks], lb[ks])), shape=(n_total, n_total)), directed=False)
        lab = new[lab]
        rounds += 1
    return in_tree, comps, int((picked > 0).sum()), int(picked.max()) if len(picked) else 0, rounds


def propagate(I, QQ, in_tree, q0, n_total):
    """T(0) = q0, T(b) = QQ_k (x) T(a) walked from a, T(a) = QQ_k* (x) T(b) walked from b; breadth first, long double"""
    adj = [[] for _ in range(n_total)]
    for k in np.flatnonzero(in_tree).tolist():
        adj[int(I[k, 0])].append(k)
        adj[int(I[k, 1])].append(k)
    T = np.zeros((n_total, 4), dtype=LD)
    T[0] = np.asarray(q0, dtype=LD)
    seen = np.zeros(n_total, dtype=bool)
    seen[0] = True
    frontier = [0]
    QL = np.asarray(QQ, dtype=LD)
    while frontier:                                               # one vectorised product per level
        us, ks, vs, inv = [], [], [], []
        for u in frontier:
            for k in adj[u]:
                a, b = int(I[k, 0]), int(I[k, 1])
                v = b if a == u else a
                if not seen[v]:
                    seen[v] = True
                    us.append(u), ks.append(k), vs.append(v), inv.append(v == a)
        if vs:
            e = QL[ks].copy()
            e[np.array(inv), 3] *= -1
            T[vs] = qmul(e, T[us])
        frontier = vs
    assert seen.all()
    return T


def reference(g):
    if "ref" not in g:
        in_tree, comps, npos, rmax, rounds = kruskal(g["I"], g["rank"], g["n_total"])
        r = dict(in_tree=in_tree, info=dict(rounds=rounds, components=comps, ranked_edges=npos, max_rank=rmax),
                 rc=capi.OK if comps == 1 else capi.ERR_NOT_SPANNING)
        if comps == 1:
            r["T"] = propagate(g["I"], g["QQ"], in_tree, g["Q"][0], g["n_total"])
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        g["ref"] = r
    return g["ref"]


# ---- graphs ------------------------------------------------------------------------------------------------------------------
def unit(rng, n):
    q = rng.standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def graph(I, n_total, f=1, rank=None, seed=0):
    """relative rotations that are random unit quaternions (no pose explains them: every tree gives other rows), Q with a
    random unit row 0, rows 1 .. f-1 arbitrary numbers that nothing may read or write, the free rows NaN"""
    rng = np.random.default_rng(seed)
    I = np.asarray(I, dtype=np.int32).reshape(-1, 2)
    Q = np.full((n_total, 4), np.nan)
    Q[:f] = rng.standard_normal((f, 4)) * 7.0
    Q[0] = unit(rng, 1)[0]
    return dict(I=I, QQ=unit(rng, len(I)), n_total=n_total, f=f, Q=Q,
                rank=None if rank is None else np.asarray(rank, dtype=np.int32))


def path(n):
    return [(i, i + 1) for i in range(n - 1)]


def ruler(n):
    """the edges (i, i + 1) listed by the ruler function of i + 1 (how often 2 divides it), then by i"""
    return sorted(path(n), key=lambda e: (((e[0] + 1) & -(e[0] + 1)).bit_length(), e[0]))


def band(n, w, rng, shuffle=False):
    I = np.array([(v - j, v) for v in range(1, n) for j in range(1, w + 1) if v - j >= 0], dtype=np.int32)
    return I[rng.permutation(len(I))] if shuffle else I


# ---- the calls ---------------------------------------------------------------------------------------------------------------
def run_dev(g, in_tree=True, **kw):
    Q = t64(g["Q"])
    r = torch_api.init_tree(t32(g["I"]), t64(g["QQ"]), g["n_total"], Q, g["f"], None if g["rank"] is None else t32(g["rank"]),
                            in_tree=torch.full((len(g["I"]),), -7, dtype=torch.int32, device=dev()) if in_tree else False,
                            allow_rc=(capi.ERR_NOT_SPANNING,), **kw)
    torch.cuda.synchronize()
    return dict(rc=r["rc"], Q=Q.cpu().numpy(), in_tree=None if r["in_tree"] is None else r["in_tree"].cpu().numpy(), info=r["info"])


def run_host(g):
    Q = g["Q"].copy()
    r = capi.init_tree(g["I"], g["QQ"], g["n_total"], Q, g["f"], g["rank"], allow_rc=(capi.ERR_NOT_SPANNING,))
    return dict(rc=r["rc"], Q=Q, in_tree=r["in_tree"], info=r["info"])


def same_bytes(a, b):
    return a["rc"] == b["rc"] and a["Q"].tobytes() == b["Q"].tobytes() and a["info"] == b["info"] and \
        (a["in_tree"] is None or b["in_tree"] is None or (a["in_tree"] == b["in_tree"]).all())


WORST = [0.0]


def check(g, host=True):
    """(a) - (d) of the module docstring; a graph that does not span: the status, info, and every output byte kept"""
    e, r = reference(g), run_dev(g)
    assert r["rc"] == e["rc"] and r["info"] == e["info"], (r["rc"], r["info"], e["info"])
    f = g["f"]
    if e["rc"] == capi.OK:
        assert (r["in_tree"] == e["in_tree"]).all()                                   # (a)
        assert np.isfinite(r["Q"][f:]).all()
        worst = float(angle(r["Q"][f:], e["T"][f:]).max()) if f < g["n_total"] else 0.0
        WORST[0] = max(WORST[0], worst)
        print("n_total %d: largest deviation %.3g rad (bound %.3g), largest so far %.3g" % (g["n_total"], worst,
                                                                                          TOL(g["n_total"]), WORST[0]))
        assert worst <= TOL(g["n_total"])                                             # (b)
        assert r["Q"][:f].tobytes() == g["Q"][:f].tobytes()                           # (c)
    else:
        assert r["Q"].tobytes() == g["Q"].tobytes() and (r["in_tree"] == -7).all()
    assert same_bytes(run_dev(g), r)                                                  # (d)
    if host:
        h = run_host(g)
        if e["rc"] != capi.OK:
            h["in_tree"] = None                                                       # (preset to -1 there, -7 here)
        assert same_bytes(h, r)
    return r


# ---- the named shapes --------------------------------------------------------------------------------------------------------
def test_two_views_one_edge_forward_and_backward():
    a, b = graph([(0, 1)], 2, seed=1), graph([(1, 0)], 2, seed=1)
    ra, rb = check(a), check(b)
    assert ra["info"]["rounds"] == 1 and rb["info"]["rounds"] == 1               # the mutual pick at n_total = 2
    assert angle(ra["Q"][1], rb["Q"][1]) > 1e-3                                    # the direction matters


def test_a_chain_listed_in_order_and_reversed_gives_the_same_rows():
    a = graph(path(5), 5, seed=2)
    b = dict(a, I=a["I"][::-1].copy(), QQ=a["QQ"][::-1].copy())
    ra, rb = check(a), check(b)
    assert (ra["in_tree"] == 1).all() and (rb["in_tree"] == 1).all()
    assert angle(ra["Q"][1:], rb["Q"][1:]).max() <= TOL(5)


def test_the_mutual_pick_inside_a_path_and_a_final_representative_that_is_not_view_0():
    r = check(graph([(1, 2), (0, 1), (2, 3)], 4, seed=3))                          # 1 and 2 choose edge 0; 1 stays
    assert r["info"]["rounds"] == 1
    check(graph([(1, 2), (0, 1)], 3, seed=4))                                      # view 0 hooks under view 1
    check(graph([(0, 1), (1, 2)], 3, seed=4))                                      # view 0 stays to the end


def test_a_path_of_300_in_one_round_and_by_the_ruler_function():
    r = check(graph(path(300), 300, seed=5))
    launches, jumps = capi.init_tree_counters()                                    # (of the host form, the last call)
    assert r["info"]["rounds"] == 1 and jumps <= 9, (r["info"], jumps)            # a hook chain of 299
    r = check(graph(ruler(300), 300, seed=6))
    assert r["info"]["rounds"] == 8                                                # components pair up (docstring)


def test_rank_avoids_an_edge_uses_it_as_a_bridge_and_never_uses_a_negative_one():
    r = check(graph([(0, 1), (1, 2), (2, 0)], 3, rank=[2, 0, 0], seed=7))
    assert r["in_tree"].tolist() == [0, 1, 1] and r["info"]["ranked_edges"] == 0 and r["info"]["max_rank"] == 0
    bridge = [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (2, 3)]
    r = check(graph(bridge, 6, rank=[0, 0, 0, 0, 0, 0, 2], seed=8))
    assert r["in_tree"][6] == 1 and r["info"]["ranked_edges"] == 1 and r["info"]["max_rank"] == 2
    r = check(graph(bridge, 6, rank=[0, 0, 0, 0, 0, 0, -1], seed=8))
    assert r["rc"] == capi.ERR_NOT_SPANNING and r["info"]["components"] == 2


def test_edge_kinds():
    I = [(1, 1), (0, 1), (0, 1), (1, 0), (1, 2), (2, 3), (3, 2), (0, 2)]          # a self loop, parallel and reversed edges,
    r = check(graph(I, 4, f=3, seed=9))                                            # edges between fixed views, view 3 behind 2
    assert r["in_tree"].tolist() == [0, 1, 0, 0, 1, 1, 0, 0]
    r = check(graph(I + [(4, 4)], 5, f=3, seed=9))                                 # view 4: a self loop alone
    assert r["rc"] == capi.ERR_NOT_SPANNING and r["info"]["components"] == 2
    r = check(graph(I, 4, f=4, seed=9))                                            # nothing free: nothing written
    assert r["rc"] == capi.OK


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025])
def test_counts_around_one_workgroup_pass(n):
    rng = np.random.default_rng(n)
    tree = [(int(rng.integers(0, v)), v) for v in range(1, n)]
    check(graph(tree + [(int(rng.integers(0, n)), int(rng.integers(0, n)))], n, seed=n))          # m == n_total
    I = band(n, 4, rng, shuffle=True)
    for m in (255, 256, 257, 1023, 1024, 1025):
        if 0 <= m - (n - 1) <= len(I):                                             # a spanning path and m - n + 1 chords
            J = np.concatenate([np.array(path(n), dtype=np.int32), I[:m - (n - 1)]])
            check(graph(J[rng.permutation(len(J))], n, seed=n + m), host=False)


def test_random_multigraphs_and_their_statuses():
    rng = np.random.default_rng(2024)
    spanning = 0
    for t in range(200):
        m = int(rng.integers(1, 1501))
        n = int(rng.integers(2, 2 + min(299, max(1, m // 5))))
        cut, half = rng.integers(0, 5) == 0, int(rng.integers(1, n))              # about a fifth: two sides no edge joins
        I = rng.integers(0, n, (m, 2))
        if cut:
            low = rng.integers(0, 2, m) == 0
            I = np.where(low[:, None], rng.integers(0, half, (m, 2)), rng.integers(half, n, (m, 2)))
        kind = rng.integers(0, 16, m)
        for k in range(1, m):
            if kind[k] == 0:
                I[k] = I[k - 1]                                                    # a duplicate
            elif kind[k] == 1:
                I[k] = I[k - 1][::-1]                                              # a reversed duplicate
            elif kind[k] == 2:
                I[k, 1] = I[k, 0]                                                  # a self loop
        g = graph(I, n, f=1 + int(rng.integers(0, 3)) % n, rank=None if t % 7 == 0 else rng.integers(-1, 4, m), seed=t)
        spanning += check(g, host=t % 10 == 0)["rc"] == capi.OK
    assert 120 <= spanning <= 185                                                  # about a fifth do not span


def test_a_shuffled_band_graph_of_20000_views():
    rng = np.random.default_rng(77)
    n = 20000
    I = band(n, 16, rng, shuffle=True)[:300000]                                   # 300 000 of the 319 864 edges of a band of 16
    rank = np.zeros(len(I), dtype=np.int32)
    rank[rng.choice(len(I), 64, replace=False)] = 1
    g = graph(I, n, rank=rank, seed=10)
    # rows that are products of honest rotations: the deviation is then an error of the products alone
    gt = unit(np.random.default_rng(11), n)
    g["QQ"] = synth.qmul(gt[I[:, 1]], synth.qconj(gt[I[:, 0]]))
    r = check(g)
    assert r["info"]["rounds"] > 1 and r["info"]["ranked_edges"] == 0


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def test_ids_at_the_top_of_the_range_are_refused_with_outputs_untouched():
    base = graph([(0, 1), (1, 2), (2, 3)], 4, seed=12)
    for bad in (-1, 4, 2 ** 31 - 1, -2 ** 31):
        for where in ((0, 0), (2, 1)):
            I = base["I"].copy()
            I[where] = bad
            Q, tree = t64(base["Q"]), torch.full((3,), -7, dtype=torch.int32, device=dev())
            r = torch_api.init_tree(t32(I), t64(base["QQ"]), 4, Q, in_tree=tree, allow_rc=(capi.ERR_BAD_ARG,))
            torch.cuda.synchronize()
            assert r["rc"] == capi.ERR_BAD_ARG and r["info"] is None
            assert Q.cpu().numpy().tobytes() == base["Q"].tobytes() and (tree == -7).all()
            assert capi.init_tree(I, base["QQ"], 4, base["Q"].copy(), allow_rc=(capi.ERR_BAD_ARG,))["rc"] == capi.ERR_BAD_ARG


def test_int64_ids_are_narrowed():
    g = graph(band(40, 3, np.random.default_rng(0)), 40, seed=13)
    want = check(g)
    Q = t64(g["Q"])
    r = torch_api.init_tree(t32(g["I"]).long(), t64(g["QQ"]), 40, Q, in_tree=True)
    assert Q.cpu().numpy().tobytes() == want["Q"].tobytes() and (r["in_tree"].cpu().numpy() == want["in_tree"]).all()
    I = t32(g["I"]).long()
    I[5, 0] = 2 ** 32                                                              # (0 if its low 32 bits were taken)
    r = torch_api.init_tree(I, t64(g["QQ"]), 40, t64(g["Q"]), allow_rc=(capi.ERR_BAD_ARG,))
    assert r["rc"] == capi.ERR_BAD_ARG


def layouts(a):
    """the same matrix as 16-byte rows, as planes, as rows with a gap, and as rows of four at an odd multiple of 8 bytes"""
    n = len(a)
    aos = t64(a)
    planes = t64(a.T.copy()).t()
    padded = torch.zeros((n, 6), dtype=torch.float64, device=dev())[:, 1:5]
    padded.copy_(aos)
    odd = torch.zeros(4 * n + 1, dtype=torch.float64, device=dev())[1:].view(n, 4)
    odd.copy_(aos)
    return dict(aos=aos, planes=planes, padded=padded, odd=odd)


def test_every_stride_form_of_QQ_and_Q():
    g = graph(band(300, 4, np.random.default_rng(1), shuffle=True), 300, f=2, seed=14)
    want = check(g)
    ei = t32(g["I"])
    for qq_name, qq in layouts(g["QQ"]).items():
        for q_name, Q in layouts(g["Q"]).items():
            assert (qq.stride(0) == 4) == (qq_name in ("aos", "odd")) and (Q.stride(1) == 1) == (q_name != "planes")
            r = torch_api.init_tree(ei, qq, 300, Q, 2)
            assert r["rc"] == capi.OK and Q.cpu().numpy().tobytes() == want["Q"].tobytes(), (qq_name, q_name)


def test_in_tree_and_info_may_be_null():
    g = graph(band(50, 2, np.random.default_rng(2)), 50, seed=15)
    want = check(g)
    ei, qq, Q = t32(g["I"]), t64(g["QQ"]), t64(g["Q"])
    rc = capi.lib().irotavg_init_tree_dev(len(g["I"]), 50, 1, C.c_void_p(ei.data_ptr()), C.c_void_p(qq.data_ptr()), 4, 1, None,
                                          C.c_void_p(Q.data_ptr()), 4, 1, None, None, None)
    torch.cuda.synchronize()
    assert rc == capi.OK and Q.cpu().numpy().tobytes() == want["Q"].tobytes()
    assert run_dev(g, in_tree=False)["in_tree"] is None
    Qh = capi.fmat(g["Q"])
    rc = capi.lib().irotavg_init_tree(len(g["I"]), 50, 1, capi._i(g["I"]), capi._d(capi.fmat(g["QQ"])), len(g["I"]), None,
                                      capi._d(Qh), 50, None, None)
    assert rc == capi.OK and np.ascontiguousarray(Qh).tobytes() == want["Q"].tobytes()


def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream():
    g = graph(band(3000, 5, np.random.default_rng(3), shuffle=True), 3000, seed=16)
    want = run_dev(g)
    ei, half, Q = t32(g["I"]), t64(g["QQ"] * 0.5), t64(g["Q"])
    big = torch.ones(1 << 25, dtype=torch.float64, device=dev())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = big
        for _ in range(16):                                       # keeps the stream busy while the call is made
            busy = busy * 1.5
        qq = half * 2.0                                           # exact: the inputs of the synchronised run, produced on the stream
        r = torch_api.init_tree(ei, qq, 3000, Q, in_tree=True)
        doubled = r["in_tree"] * 2                                # consumed right behind the call, no synchronise
    side.synchronize()
    assert Q.cpu().numpy().tobytes() == want["Q"].tobytes() and r["info"] == want["info"]
    assert (doubled.cpu().numpy() == 2 * want["in_tree"]).all()


# ---- end to end: cycle_check -> rank_from_cycle_check -> init_tree -> l1ra -> irls ----------------------------------------------
E2E_SEED = 0


def planted_band(seed):
    """400 views, 6 predecessors each in generation order, 0.01 rad of noise, 5 % of the edges replaced by random rotations"""
    rng = np.random.default_rng(seed)
    n = 400
    I = band(n, 6, rng)
    gt = unit(rng, n)
    gt[0] = [0, 0, 0, 1.0]
    QQ = synth.qmul(synth.qmul(gt[I[:, 1]], synth.qconj(gt[I[:, 0]])), synth.qexp(0.01 * rng.standard_normal((len(I), 3))))
    planted = np.zeros(len(I), dtype=bool)
    planted[rng.choice(len(I), len(I) // 20, replace=False)] = True
    QQ[planted] = unit(rng, int(planted.sum()))
    return dict(I=I, QQ=QQ, gt=gt, planted=planted, n_total=n)


def sweep_tree(I, n_total):
    """the edges over which irotavg_init_mst's sweep reaches a view first (f = 1)"""
    seen = np.zeros(n_total, dtype=bool)
    seen[0] = True
    used = np.zeros(len(I), dtype=bool)
    while not seen.all():
        grew = False
        for k, (a, b) in enumerate(I.tolist()):
            if seen[a] != seen[b]:
                seen[a] = seen[b] = used[k] = grew = True
        assert grew
    return used


def test_end_to_end_the_cycle_check_steers_the_tree_away_from_planted_edges():
    g = planted_band(E2E_SEED)
    n, I = g["n_total"], g["I"]
    swept = sweep_tree(I, n)
    assert (swept & g["planted"]).any()                                            # the sweep crosses a planted edge
    Q0 = np.tile([0, 0, 0, 1.0], (n, 1))
    Qs = ral.init_mst(Q0.copy(), g["QQ"], I, 1)
    ei, qq = t32(I), t64(g["QQ"])
    c = torch_api.cycle_check(ei, qq, n)
    rank = torch_api.rank_from_cycle_check(c["tri_count"], c["tri_ok"])
    Qt = t64(Q0)
    r = torch_api.init_tree(ei, qq, n, Qt, rank=rank, in_tree=True)
    tree = r["in_tree"].cpu().numpy() == 1
    assert r["info"]["max_rank"] <= 1 and not (tree & g["planted"]).any()          # no contradicted and no planted edge
    err_tree = synth.angular_distance(Qt.cpu().numpy(), g["gt"]).max()
    err_sweep = synth.angular_distance(Qs, g["gt"]).max()
    print("largest error against the ground truth: tree %.4g rad, sweep %.4g rad" % (err_tree, err_sweep))
    assert err_tree < err_sweep
    # both chains to convergence: the same minimum within the project's 1e-9 rad
    G = torch_api.TorchGraph(ei, qq, n, 1)
    out = G.init_tree(ei, qq, rank)
    assert out["rc"] == capi.OK and out["Q"].cpu().numpy().tobytes() == Qt.cpu().numpy().tobytes()
    a1, a2 = G.l1ra(5), G.irls(4, max_iters=200, change_th=1e-13)
    Qa = G.rotations().cpu().numpy()
    H = capi.Graph(I, g["QQ"], n, 1)
    H.set_rotations(Qs)
    b1, b2 = H.l1ra(5), H.irls(4, max_iters=200, change_th=1e-13)
    Qb = np.ascontiguousarray(H.get_rotations())
    d = synth.angular_distance(Qa, Qb).max()
    print("iterations l1ra / irls: tree %d / %d, sweep %d / %d; largest distance of the results %.3g rad"
          % (a1["iters"], a2["iters"], b1["iters"], b2["iters"], d))
    assert d < 1e-9
