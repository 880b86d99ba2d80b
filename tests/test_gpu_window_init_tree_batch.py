"""irotavg_window_init_tree_batch_dev (irotavg_amd/csrc/wintree.hip, wintree.hpp, devapi.hip;
torch_api.window_init_tree_batch; docs/window_init_tree_batch.md): the minimum spanning forest under the keys (rank[k], k),
grown from the fixed views, and the free views' rotations along it, one workgroup per problem, one launch.

The reference is restated here (ref): Kruskal on the contracted graph, then the path products from the fixed rows in
np.longdouble. in_tree and the integers of `results` are compared exactly, the fixed rows byte for byte, every free
rotation by the angle of q (x) q'^-1 in long double. Free rows are NaN on entry in every case: they are never read.
TOL follows the project's rule (docs/local_sweeps.md): 100 x the largest angle between the float64 and the long-double
restatement on this file's graphs, measured on the CPU when the module loads (1.03e-15 rad), with a floor of 1e-12 rad."""
import ctypes as C

import numpy as np
import pytest
import torch

from irotavg_amd import capi, synth, torch_api

pytestmark = pytest.mark.gpu
LD = np.longdouble


def tt(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def angle(p, q):
    d = synth.qmul(np.asarray(p, dtype=LD), np.asarray(q, dtype=LD) * np.array([-1, -1, -1, 1], dtype=LD))
    return (2 * np.arctan2(np.sqrt((d[..., :3] ** 2).sum(-1)), np.abs(d[..., 3]))).astype(np.float64)


def case(name, nv, f, I, rank=None, seed=0, noise=0.01):
    """edges -> a problem around a ground truth: unit measurements with `noise` rad of error, fixed rows at the truth"""
    I = np.array(I, dtype=np.int32).reshape(-1, 2)
    rng = np.random.default_rng([seed, nv, f, len(I)])
    gt = rng.normal(size=(nv, 4))
    gt /= np.linalg.norm(gt, axis=1, keepdims=True)
    QQ = synth.qmul(synth.qexp(rng.normal(scale=noise, size=(len(I), 3))), synth.qmul(gt[I[:, 1]], synth.qconj(gt[I[:, 0]])))
    Q0 = np.where(np.arange(nv)[:, None] < f, gt, np.nan)
    return dict(name=name, nv=nv, f=f, ne=len(I), I=I, QQ=QQ, Q0=Q0, gt=gt,
                rank=np.zeros(len(I), dtype=np.int32) if rank is None else np.array(rank, dtype=np.int32))


def ref(c, dtype=LD, rank=None):
    """(in_tree, free views left, tree edges with rank > 0, largest rank, rows) by the definition"""
    rank, f = c["rank"] if rank is None else rank, c["f"]
    node = lambda v: 0 if v < f else v - f + 1
    parent = list(range(c["nv"] - f + 1))

    def find(v):
        while parent[v] != v:
            v = parent[v]
        return v
    E, in_tree, adj = c["I"].tolist(), np.zeros(c["ne"], dtype=np.int32), {}
    for r, k in sorted((int(rank[k]), k) for k in range(c["ne"]) if rank[k] >= 0 and node(E[k][0]) != node(E[k][1])):
        ra, rb = find(node(E[k][0])), find(node(E[k][1]))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            in_tree[k] = 1
            for u, v in (E[k], E[k][::-1]):
                adj.setdefault(u, []).append((k, v))
    T, queue = {u: c["Q0"][u].astype(dtype) for u in range(f)}, list(range(f))
    for u in queue:
        for k, v in adj.get(u, []):
            if v not in T:
                T[v] = synth.qmul(c["QQ"][k].astype(dtype) * np.array([1, 1, 1, 1 if v == E[k][1] else -1], dtype=dtype), T[u])
                queue.append(v)
    picked = rank[in_tree == 1]
    left = sum(find(v) != 0 for v in range(1, len(parent)))
    rows = None if left else np.stack([T[v] for v in range(c["nv"])])
    return in_tree, left, (0 if left else int((picked > 0).sum())), (0 if left else int(picked.max())), rows


def rand_case(name, nv, f, m, seed):
    """a spanning backbone of rank >= 0 at the END; in front duplicates, reversed ones, self loops, random pairs, ranks -1 .. 2"""
    rng = np.random.default_rng([seed, nv, f, m])
    B = [(int(rng.integers(0, v)), v) for v in range(f, nv)]
    pad = [(a, a) if kind == 0 else B[a % len(B)][::-1] if kind == 1 else B[b % len(B)] if kind == 2 else (a, b)
           for kind, a, b in zip(rng.integers(0, 6, m - len(B)), rng.integers(0, nv, m - len(B)), rng.integers(0, nv, m - len(B)))]
    return case(name, nv, f, pad + B, np.concatenate([rng.integers(-1, 3, len(pad)), rng.integers(0, 3, len(B))]), seed)


CYCLES = rand_case("f1-cycles", 20, 1, 60, 1)
CUT = case("cut", 5, 2, [(0, 2), (2, 3), (3, 4)], [0, 0, -1])
SHAPES = [case("forward", 2, 1, [(0, 1)]), case("backward", 2, 1, [(1, 0)]), CYCLES,
          case("one-free", 6, 5, [(0, 5), (5, 1), (2, 5), (5, 3), (4, 5)], [2, 1, 1, 0, 0]),
          case("chain64-backwards", 65, 1, [(v - 1, v) for v in range(64, 0, -1)]),
          case("star64", 65, 1, [(v, 0) for v in range(1, 65)]),
          case("own-fixed-view-64", 320, 256, [(256 + v, 4 * v) for v in range(64)], seed=2),
          case("equal-ranks", 20, 3, rand_case("", 20, 3, 70, 3)["I"], [5] * 70),
          case("duplicates", 4, 1, [(0, 1), (1, 0), (0, 1), (1, 2), (2, 1), (2, 3), (3, 2)], [2, 1, 1, 1, 0, 0, 0], noise=0.3),
          case("big-rank", 3, 1, [(0, 1), (0, 1), (1, 2)], [0x7fffffff, 0, 0x7fffffff], noise=0.3),
          case("negative-forces-next", 3, 1, [(0, 1), (0, 1), (1, 2)], [-1, 3, 0], noise=0.3), CUT,
          case("loops-and-fixed-fixed", 5, 2, [(0, 1), (2, 2), (1, 0), (0, 2), (2, 3), (3, 3), (4, 3)], [0, 0, 0, 1, 1, 0, 1]),
          case("isolated-fixed-view", 5, 3, [(2, 4), (0, 3)])] + \
         [rand_case("m%d" % m, 72, 8, m, 4) for m in (255, 256, 257, 512, 513, 640)] + [rand_case("limit", 320, 256, 640, 5)]
REF = {c["name"]: ref(c) for c in SHAPES}
OK = [c for c in SHAPES if REF[c["name"]][1] == 0]
TOL = max(1e-12, 100 * max(angle(ref(c, np.float64)[4], REF[c["name"]][4])[c["f"]:].max() for c in OK))


def pack(cases):
    return (np.array([(c["nv"], c["f"], c["ne"]) for c in cases], dtype=np.int32), np.concatenate([c["I"] for c in cases]),
            np.concatenate([c["QQ"] for c in cases]), np.concatenate([c["Q0"] for c in cases]),
            np.concatenate([c["rank"] for c in cases]))


def run(cases, rank=True, in_tree=True, ids=torch.int32, rdt=torch.int32, allow_rc=(), I=None):
    sizes, I0, QQ, Q, rk = pack(cases)
    q, tree = tt(Q), (torch.full((len(rk),), -7, dtype=torch.int32, device="cuda") if in_tree else False)
    r = torch_api.window_init_tree_batch(sizes, tt(I0 if I is None else I, ids), tt(QQ), q, tt(rk, rdt) if rank else None, tree,
                                         allow_rc=allow_rc)
    torch.cuda.synchronize()
    return dict(r, Qh=q.cpu().numpy(), tree=tree.cpu().numpy() if in_tree else None)


def check(cases, r, want=None, only=None):
    """every problem of the batch against the reference (want: {name: ref(...)} where it is not REF's)"""
    eo, vo = np.cumsum([0] + [c["ne"] for c in cases]), np.cumsum([0] + [c["nv"] for c in cases])
    for b, c in enumerate(cases):
        if only is not None and b not in only:
            continue
        in_tree, left, rank_pos, rank_max, rows = (want or REF)[c["name"]]
        got, tree = r["Qh"][vo[b]:vo[b + 1]], None if r["tree"] is None else r["tree"][eo[b]:eo[b + 1]]
        assert list(r["results"][b]) == [capi.ERR_NOT_SPANNING if left else 0, left, rank_pos, rank_max], c["name"]
        assert got[:c["f"]].tobytes() == c["Q0"][:c["f"]].tobytes(), c["name"]
        if left:
            assert got.tobytes() == c["Q0"].tobytes() and (tree is None or (tree == -7).all()), c["name"]
            continue
        assert tree is None or ((tree == in_tree).all() and tree.sum() == c["nv"] - c["f"]), c["name"]
        worst = angle(got[c["f"]:], rows[c["f"]:]).max()
        print("%s: worst angle %.3g rad (TOL %.3g)" % (c["name"], worst, TOL))
        assert worst <= TOL, c["name"]


@pytest.mark.parametrize("c", SHAPES, ids=[c["name"] for c in SHAPES])
def test_shape_alone(c):
    r = run([c], allow_rc=(capi.ERR_NOT_SPANNING,) if c is CUT else ())
    check([c], r)
    assert r["rc"] == r["results"][0, 0] and (c is not CUT or list(r["results"][0]) == [capi.ERR_NOT_SPANNING, 1, 0, 0])


def test_f1_is_init_tree_s_tree():
    c = CYCLES
    q = tt(np.where(np.isnan(c["Q0"]), 0.0, c["Q0"]))
    t = torch_api.init_tree(tt(c["I"], torch.int32), tt(c["QQ"]), c["nv"], q, 1, tt(c["rank"], torch.int32), in_tree=True)
    r = run([c])
    assert (t["in_tree"].cpu().numpy() == r["tree"]).all() and angle(q.cpu().numpy()[1:], r["Qh"][1:]).max() <= TOL


def test_rank_none_and_no_in_tree():
    cases = [SHAPES[2], SHAPES[3], SHAPES[8], SHAPES[14]]
    want = {c["name"]: ref(c, rank=np.zeros(c["ne"], dtype=np.int32)) for c in cases}
    check(cases, run(cases, rank=False), want)
    r = run(cases, in_tree=False)
    check(cases, r)
    assert run(cases, rdt=torch.int64)["Qh"].tobytes() == r["Qh"].tobytes()
    c = SHAPES[9]
    with pytest.raises(ValueError, match="int32 range"):
        torch_api.window_init_tree_batch(np.array([(3, 1, 3)]), tt(c["I"], torch.int32), tt(c["QQ"]), tt(c["Q0"]),
                                         tt([2 ** 31, 0, 0], torch.int64))


def test_one_batch_alone_or_in_the_middle_twice_and_with_a_bad_id():
    alone = {c["name"]: run([c], allow_rc=(capi.ERR_NOT_SPANNING,)) for c in SHAPES}
    r = run(SHAPES, allow_rc=(capi.ERR_NOT_SPANNING,))
    check(SHAPES, r)
    assert r["rc"] == capi.ERR_NOT_SPANNING and r["Qh"].tobytes() == b"".join(alone[c["name"]]["Qh"].tobytes() for c in SHAPES)       # alone == inside the batch
    assert r["tree"].tobytes() == b"".join(alone[c["name"]]["tree"].tobytes() for c in SHAPES)
    assert all(run(SHAPES, allow_rc=(capi.ERR_NOT_SPANNING,))[k].tobytes() == r[k].tobytes() for k in ("Qh", "tree"))   # a second call
    five = [SHAPES[14], SHAPES[2], SHAPES[15], CUT, SHAPES[3]]
    I = np.concatenate([c["I"] for c in five]).astype(np.int64)
    for bad, ids in ((20, torch.int32), (2 ** 32 + 3, torch.int64)):          # an id equal to n_total; one that only truncation makes valid
        I[five[0]["ne"] + 7, 1] = bad
        r = run(five, I=I, ids=ids, allow_rc=(capi.ERR_BAD_ARG, capi.ERR_NOT_SPANNING))
        assert r["rc"] == capi.ERR_BAD_ARG and list(r["results"][1]) == [capi.ERR_BAD_ARG, 0, 0, 0]
        assert r["Qh"][five[0]["nv"]:][:20].tobytes() == five[1]["Q0"].tobytes() and (r["tree"][five[0]["ne"]:][:60] == -7).all()
        check(five, r, only=[0, 2, 3, 4])
    check(five, run(five, ids=torch.int64, allow_rc=(capi.ERR_NOT_SPANNING,)))


FORMS = {"planes": lambda n: (0, 1, n + 5), "offset8": lambda n: (1, 4, 1), "padded": lambda n: (2, 7, 1),
         "negative-rows": lambda n: (4 * (n - 1) + 1, -4, 1), "negative-both": lambda n: (4 * n + 2, -4, -1)}


@pytest.mark.parametrize("form", list(FORMS))
def test_stride_forms_through_the_c_call(form):
    cases = [SHAPES[14], SHAPES[3], SHAPES[12], SHAPES[4]]
    sizes, I, QQ, Q, rk = pack(cases)
    want = run(cases)

    def place(A):
        base, rs, cs = FORMS[form](len(A))
        idx = base + np.arange(len(A))[:, None] * rs + np.arange(4)[None] * cs
        flat = np.full(idx.max() + 3, 9.75)
        flat[idx] = A
        return tt(flat), idx, base, rs, cs
    (qq, _, qb, qrs, qcs), (q, idx, b, rs, cs) = place(QQ), place(Q)
    ei, rank, tree, res = tt(I, torch.int32), tt(rk, torch.int32), tt(np.zeros(len(rk)), torch.int32), np.zeros(4 * len(cases), dtype=np.int32)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + 8 * off)
    rc = capi.lib().irotavg_window_init_tree_batch_dev(
        len(cases), sizes.ctypes.data_as(C.POINTER(C.c_int32)), p(ei), p(qq, qb), qrs, qcs, p(rank), p(q, b), rs, cs, p(tree),
        res.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    flat = q.cpu().numpy()
    assert rc == 0 and flat[idx].tobytes() == want["Qh"].tobytes() and (tree.cpu().numpy() == want["tree"]).all()
    assert (res.reshape(-1, 4) == want["results"]).all() and (np.delete(flat, idx.ravel()) == 9.75).all()


def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream():
    cases = [SHAPES[14], SHAPES[3], SHAPES[4]]
    sizes, I, QQ, Q, rk = pack(cases)
    want = run(cases)
    ei, rank, qq_half, q_half = tt(I, torch.int32), tt(rk, torch.int32), tt(QQ * 0.5), tt(Q * 0.5)
    big = torch.ones(1 << 25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = big
        for _ in range(16):                                       # keeps the stream busy while the call is made
            busy = busy * 1.5
        qq_t, q_t = qq_half * 2.0, q_half * 2.0                   # exact: the inputs of the synchronised run, produced on the stream
        r = torch_api.window_init_tree_batch(sizes, ei, qq_t, q_t, rank, True)
        doubled, tree = q_t * 2.0, r["in_tree"] + 0               # consumed right behind the call, no synchronise
    side.synchronize()
    assert busy[-1] == 1.5 ** 16 and (doubled.cpu().numpy() * 0.5).tobytes() == want["Qh"].tobytes()
    assert (tree.cpu().numpy() == want["tree"]).all() and (r["results"] == want["results"]).all()


def test_the_rank_from_cemp_keeps_planted_edges_out_of_the_start():
    """12 views, 2 fixed, every view linked to its 4 predecessors; three measurements off by about 1 rad are listed first,
    where the sweep of window_init_mst_batch takes them: (0, 2) reaches 2, (2, 5) reaches 5, (5, 8) reaches 8"""
    rng = np.random.default_rng(11)
    planted = [(0, 2), (2, 5), (5, 8)]
    rest = [(v - d, v) for d in range(1, 5) for v in range(d, 12) if (v - d, v) not in planted]
    c = case("window", 12, 2, planted + [rest[i] for i in rng.permutation(len(rest))], seed=11)
    axis = rng.normal(size=(3, 3))
    c["QQ"][:3] = synth.qmul(synth.qexp(axis / np.linalg.norm(axis, axis=1, keepdims=True)), c["QQ"][:3])
    seen, sweep = {0}, []                                          # the sweep of init_mst, restated
    while len(seen) < 12:
        for k, (a, b) in enumerate(c["I"].tolist()):
            if (a in seen) != (b in seen):
                seen |= {a, b}
                sweep.append(k)
    assert set(sweep) >= {0, 1, 2}                                 # the planted edges are in the sweep's tree
    assert ref(c, rank=np.array([2] * 3 + [0] * 35))[0][:3].sum() == 0    # the reference alone: no planted edge in its tree
    sizes, I, QQ, Q, _ = pack([c])
    ei, qq, q_tree, q_mst = tt(I, torch.int32), tt(QQ), tt(Q), tt(Q)
    s = torch_api.window_cemp_batch(sizes, ei, qq)["s"]
    r = torch_api.window_init_tree_batch(sizes, ei, qq, q_tree, torch_api.rank_from_cemp(s, 0.1), in_tree=True)
    torch_api.window_init_mst_batch(sizes, ei, qq, q_mst)
    tree_mean, mst_mean = (angle(q.cpu().numpy()[2:], c["gt"][2:]).mean() for q in (q_tree, q_mst))
    print("mean angle to the ground truth: rank-aware %.4f rad, sweep %.4f rad" % (tree_mean, mst_mean))
    assert r["in_tree"].cpu().numpy()[:3].sum() == 0 and r["in_tree"].sum() == 10
    assert tree_mean < mst_mean
