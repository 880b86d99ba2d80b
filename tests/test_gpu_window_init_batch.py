"""irotavg_window_init_mst_batch_dev (irotavg_amd/csrc/winmst.hip, winmst.hpp, devapi.hip; torch_api.window_init_mst_batch;
docs/window_init_batch.md): irotavg_init_mst on many window-size problems on packed device arrays, one workgroup per
problem, one launch.

The reference everywhere is the library's host irotavg_init_mst on each problem alone, and the comparison is == on the
bytes: the kernel finds the sweep's own tree (a parallel relaxation to the sweep's arrival times) and multiplies the same
factors in the same order without contraction. No tolerance. The host results are computed once per case and shared (HOST).

The named cases are the smallest shapes at which each part can go wrong; free rows of Q go in as a marker that no product
can give, fixed rows and measurements are random unit quaternions."""
import ctypes as C

import numpy as np
import pytest
import torch

from irotavg_amd import capi, synth, torch_api

pytestmark = pytest.mark.gpu
MARK = -7.25       # free rows on input
SIG = 5 * np.pi / 180


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def t64(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev())


def unit(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def case(name, nv, f, I, seed=0):
    """edges -> a problem: a random unit measurement per edge (duplicates differ), random fixed rows, marked free rows"""
    I = np.array(I, dtype=np.int32).reshape(-1, 2)
    rng = np.random.default_rng([seed, nv, f, len(I)])
    Q0 = np.full((nv, 4), MARK)
    Q0[:f] = unit(rng, f)
    return dict(name=name, nv=nv, f=f, ne=len(I), I=I, QQ=unit(rng, len(I)), Q0=Q0)


HOST = {}


def host(c):
    """irotavg_init_mst on the problem alone -> (rc, Q); computed once, never modified"""
    if c["name"] not in HOST:
        Qf, QQf, I = capi.fmat(c["Q0"]), capi.fmat(c["QQ"]), np.ascontiguousarray(c["I"], dtype=np.int32)
        rc = capi.lib().irotavg_init_mst(c["nv"], c["ne"], capi._d(Qf), c["nv"], capi._d(QQf), c["ne"], capi._i(I), c["f"])
        Q = np.ascontiguousarray(Qf)
        Q.setflags(write=False)
        HOST[c["name"]] = (rc, Q)
    return HOST[c["name"]]


def pack(cases):
    sizes = np.array([(c["nv"], c["f"], c["ne"]) for c in cases], dtype=np.int32)
    return (sizes, np.concatenate([c["I"] for c in cases]).astype(np.int32),
            np.concatenate([c["QQ"] for c in cases]).astype(np.float64),
            np.concatenate([c["Q0"] for c in cases]).astype(np.float64))


def slices(cases):
    return (np.concatenate([[0], np.cumsum([c["ne"] for c in cases])]),
            np.concatenate([[0], np.cumsum([c["nv"] for c in cases])]))


def run(cases, QQ_t=None, Q_t=None, allow_rc=(), I=None, int64=False):
    sizes, I0, QQ, Q = pack(cases)
    ei = torch.tensor(I0 if I is None else I, dtype=torch.int64 if int64 else torch.int32, device=dev())
    QQ_t = t64(QQ) if QQ_t is None else QQ_t
    Q_t = t64(Q) if Q_t is None else Q_t
    r = torch_api.window_init_mst_batch(sizes, ei, QQ_t, Q_t, allow_rc=allow_rc)
    torch.cuda.synchronize()
    r["Qh"] = Q_t.cpu().numpy()
    return r


def assert_bitwise(cases, r, only=None):
    """every problem of the batch against the host call on it alone; fixed rows byte-identical to the input"""
    _, vo = slices(cases)
    for b, c in enumerate(cases):
        if only is not None and b not in only:
            continue
        rc, Q = host(c)
        assert rc == 0, (c["name"], rc)
        assert r["status"][b] == 0, (c["name"], r["status"][b])
        got = r["Qh"][vo[b]:vo[b + 1]]
        assert not np.isnan(got).any() and not (got[c["f"]:] == MARK).all(axis=1).any(), c["name"]
        assert got.tobytes() == Q.tobytes(), (c["name"], np.flatnonzero((got != Q).any(axis=1))[:8])
        assert got[:c["f"]].tobytes() == np.ascontiguousarray(c["Q0"][:c["f"]]).tobytes(), c["name"]


# ---- the shapes ----------------------------------------------------------------------------------------------------------
def chain_edges(nv, reverse, m=0):
    """0 - 1 - ... - (nv - 1), listed from the far end (one view per sweep) or from view 0 (one sweep), padded to m edges
    with duplicates of its farthest edge in front: of use in the last sweep alone, where the first of them wins"""
    T = [(v, v + 1) for v in range(nv - 1)]
    if reverse:
        T = T[::-1]
    pad = [((nv - 2, nv - 1) if k % 2 == 0 else (nv - 1, nv - 2)) for k in range(max(0, m - (nv - 1)))]
    return pad + T


def tree_case(name, nv, f, m, seed):
    """a random spanning tree over all nv views, its edges in random order, directions and labels; padded to m edges
    with duplicates of tree edges (other measurements), self-loops and random pairs placed in front of the tree edges"""
    rng = np.random.default_rng([seed, nv, f, m])
    label = np.concatenate([[0], 1 + rng.permutation(nv - 1)])
    T = [(int(label[rng.integers(0, v)]), int(label[v])) for v in range(1, nv)]
    T = [T[i] for i in rng.permutation(nv - 1)]
    pad = []
    for k in range(m - (nv - 1)):
        kind = rng.integers(0, 8)
        if kind == 0:
            v = int(rng.integers(0, nv))
            pad.append((v, v))
        elif kind == 1:
            pad.append((int(rng.integers(0, nv)), int(rng.integers(0, nv))))
        else:
            pad.append(T[int(rng.integers(0, nv - 1))])
    E = [(b, a) if rng.random() < 0.5 else (a, b) for a, b in pad + T]
    return case(name, nv, f, E, seed)


TWO = [case("forward", 2, 1, [(0, 1)]), case("backward", 2, 1, [(1, 0)])]
CHAINS = [case("chain6-reversed", 6, 1, chain_edges(6, True)), case("chain6-forward", 6, 1, chain_edges(6, False))]
TRAP = case("trap", 4, 1, [(2, 3), (0, 1), (1, 2), (2, 3)])
INERT = case("inert", 5, 2, [(1, 1), (1, 0), (0, 1), (2, 1), (1, 2), (3, 3), (3, 2), (3, 4), (4, 3)])
F3 = case("f3", 5, 3, [(2, 4), (1, 2), (0, 1), (3, 0)])
F3_ISOLATED = case("f3-isolated", 5, 3, [(2, 4), (0, 2), (3, 0)])
STRIDES = [tree_case("tree-%d-%d" % (n, m), n, max(1, n - 64), m, 5)
           for m in (63, 64, 65, 255, 256, 257, 640) for n in (64, 65, 320) if m >= n - 1]
LIMIT = case("limit-chain", 320, 256, chain_edges(320, True, 640))
NAMED = TWO + CHAINS + [TRAP, INERT, F3]


def random_cases():
    rng = np.random.default_rng(2024)
    out = []
    ends = [(2, 1, 1), (320, 256, 640), (320, 319, 319), (65, 1, 640)]   # the ends of every range, whatever the draw
    for b in range(200):
        nv = int(rng.integers(2, 321))
        f = int(rng.integers(max(1, nv - 64), nv))
        m = int(rng.integers(nv - 1, 641))
        if b < len(ends):
            nv, f, m = ends[b]
        out.append(tree_case("random-%d" % b, nv, f, m, 1000 + b))
    return out


RANDOM = random_cases()


# ---- 1 .. 5: the named cases, each alone and all in one batch ---------------------------------------------------------------
@pytest.mark.parametrize("c", NAMED, ids=[c["name"] for c in NAMED])
def test_named_case_alone(c):
    assert_bitwise([c], run([c]))


def test_named_cases_in_one_batch():
    r = run(NAMED)
    assert r["rc"] == 0
    assert_bitwise(NAMED, r)


def test_the_chains_take_five_sweeps_and_one():
    """what the two chains are for: the reversed one reaches one view per sweep, so its labels cross four sweep boundaries
    (the host reference agrees with the product along the chain whatever the order)"""
    qm = lambda a, b: synth.qmul(a[None], b[None])[0]
    for c in CHAINS:
        by_view = {int(max(e)): k for k, e in enumerate(c["I"])}
        q = c["Q0"][0]
        for v in range(1, 6):
            q = qm(c["QQ"][by_view[v]], q)
        np.testing.assert_allclose(host(c)[1][5], q, rtol=0, atol=1e-14)


def test_the_trap_takes_the_later_duplicate():
    """view 3 is reached by edge 3 in sweep 0, not by edge 0 in sweep 1: the two carry different measurements"""
    c = TRAP
    r = run([c])
    qm = lambda a, b: synth.qmul(a[None], b[None])[0]
    q2 = host(c)[1][2]
    np.testing.assert_allclose(r["Qh"][3], qm(c["QQ"][3], q2), rtol=0, atol=1e-14)
    assert np.abs(r["Qh"][3] - qm(c["QQ"][0], q2)).max() > 1e-3
    assert_bitwise([c], r)


def test_a_free_view_behind_a_fixed_view_uses_the_caller_s_row():
    c = F3
    r = run([c])
    qm = lambda a, b: synth.qmul(a[None], b[None])[0]
    np.testing.assert_allclose(r["Qh"][4], qm(c["QQ"][0], c["Q0"][2]), rtol=0, atol=1e-14)   # (2, 4) forward, in sweep 2
    np.testing.assert_allclose(r["Qh"][3], qm(c["QQ"][3] * [1, 1, 1, -1], c["Q0"][0]), rtol=0, atol=1e-14)  # (3, 0) backward
    assert_bitwise([c], r)


def test_an_isolated_fixed_view_is_not_spanning():
    c = F3_ISOLATED
    assert host(c)[0] == capi.ERR_NOT_SPANNING
    r = run([c], allow_rc=(capi.ERR_NOT_SPANNING,))
    assert r["rc"] == capi.ERR_NOT_SPANNING and list(r["status"]) == [capi.ERR_NOT_SPANNING]
    assert r["Qh"].tobytes() == c["Q0"].tobytes()
    with pytest.raises(capi.IrotavgError):
        run([c])


# ---- 6. free rows are never read ---------------------------------------------------------------------------------------------
def test_nan_in_the_free_rows_is_never_read():
    cases = NAMED + STRIDES[:3]
    sizes, I, QQ, Q = pack(cases)
    _, vo = slices(cases)
    for b, c in enumerate(cases):
        Q[vo[b] + c["f"]:vo[b + 1]] = np.nan
    r = run(cases, Q_t=t64(Q))
    assert not np.isnan(r["Qh"]).any()
    assert_bitwise(cases, r)


# ---- 7. the loop strides of a 256-thread group, 8. the limits ------------------------------------------------------------------
@pytest.mark.parametrize("c", STRIDES + [LIMIT], ids=[c["name"] for c in STRIDES + [LIMIT]])
def test_loop_strides_and_limits(c):
    assert_bitwise([c], run([c]))


def test_the_limit_chain_takes_319_sweeps():
    """one view per sweep: the last one arrives in sweep 318 by the first duplicate in front, the largest label there is"""
    c = LIMIT
    assert (c["nv"], c["f"], c["ne"]) == (320, 256, 640) and tuple(c["I"][0]) == (318, 319) and tuple(c["I"][-1]) == (0, 1)
    qm = lambda a, b: synth.qmul(a[None], b[None])[0]
    Q = host(c)[1]
    np.testing.assert_allclose(Q[319], qm(c["QQ"][0], Q[318]), rtol=0, atol=1e-14)
    np.testing.assert_allclose(Q[256], qm(c["QQ"][640 - 256], c["Q0"][255]), rtol=0, atol=1e-14)


# ---- 9. one mixed batch of 200 random problems, three ways ----------------------------------------------------------------------
def test_random_batch_sizes_cover_the_ranges():
    s = np.array([(c["nv"], c["f"], c["ne"]) for c in RANDOM])
    assert len(s) == 200 and s[:, 0].min() == 2 and s[:, 0].max() == 320 and s[:, 2].min() == 1 and s[:, 2].max() == 640
    assert ((s[:, 1] >= 1) & (s[:, 1] < s[:, 0]) & (s[:, 0] - s[:, 1] <= 64)).all() and (s[:, 0] - s[:, 1]).max() == 64
    assert all(host(c)[0] == 0 for c in RANDOM)                  # the reference succeeds on all 200: none is dropped


def test_random_batch_in_caller_order():
    assert_bitwise(RANDOM, run(RANDOM))


def test_random_batch_reversed():
    rev = RANDOM[::-1]
    assert_bitwise(rev, run(rev))


def test_random_batch_oversubscribed():
    cases = [RANDOM[b % 200] for b in range(2000)]
    assert 2000 > 4 * torch.cuda.get_device_properties(dev()).multi_processor_count
    r = run(cases)
    assert r["rc"] == 0 and (r["status"] == 0).all()
    want = np.concatenate([host(c)[1] for c in RANDOM])
    assert (r["Qh"].reshape(10, -1).view(np.uint64) == want.reshape(1, -1).view(np.uint64)).all()


# ---- 10. failure isolation ---------------------------------------------------------------------------------------------------
def test_failures_stay_with_their_problems():
    good = [STRIDES[0], INERT, CHAINS[0]]
    bad_id = dict(tree_case("bad-id", 40, 3, 100, 9))
    bad_id["I"] = bad_id["I"].copy()
    bad_id["I"][57, 1] = 40                                       # an id equal to n_total
    cases = [good[0], bad_id, good[1], F3_ISOLATED, good[2]]
    r = run(cases, allow_rc=(capi.ERR_BAD_ARG, capi.ERR_NOT_SPANNING))
    assert list(r["status"]) == [0, capi.ERR_BAD_ARG, 0, capi.ERR_NOT_SPANNING, 0]
    assert r["rc"] == capi.ERR_BAD_ARG                            # the first non-zero status in problem order
    _, vo = slices(cases)
    for b in (1, 3):
        assert r["Qh"][vo[b]:vo[b + 1]].tobytes() == cases[b]["Q0"].tobytes()
    assert_bitwise(cases, r, only=[0, 2, 4])
    r = run(cases[::-1], allow_rc=(capi.ERR_BAD_ARG, capi.ERR_NOT_SPANNING))
    assert r["rc"] == capi.ERR_NOT_SPANNING
    r = run([bad_id], I=np.where(bad_id["I"] == 40, -1, bad_id["I"]), allow_rc=(capi.ERR_BAD_ARG,))
    assert r["rc"] == capi.ERR_BAD_ARG and r["Qh"].tobytes() == bad_id["Q0"].tobytes()
    assert_bitwise(good, run(good))                               # a valid call afterwards


# ---- 11. strides and streams ---------------------------------------------------------------------------------------------------
FOUR = [STRIDES[3], INERT, RANDOM[7], CHAINS[0]]


@pytest.fixture(scope="module")
def four_contiguous():
    r = run(FOUR)
    assert_bitwise(FOUR, r)
    return r


def test_column_major_planes(four_contiguous):
    _, _, QQ, Q = pack(FOUR)
    N, M = len(Q), len(QQ)
    qplanes = torch.full((4, N + 5), 321.25, dtype=torch.float64, device=dev())
    qplanes[:, :N] = t64(Q).t()
    qqplanes = t64(QQ).t().contiguous()
    r = run(FOUR, QQ_t=qqplanes.t(), Q_t=qplanes[:, :N].t())
    assert torch_api.matrix_strides(qplanes[:, :N].t()) == (1, N + 5) and torch_api.matrix_strides(qqplanes.t()) == (1, M)
    assert r["Qh"].tobytes() == four_contiguous["Qh"].tobytes()
    assert (qplanes[:, N:] == 321.25).all()


def test_contiguous_rows_behind_an_8_byte_aligned_pointer(four_contiguous):
    _, _, QQ, Q = pack(FOUR)
    flat = torch.full((4 * len(Q) + 2,), 9.75, dtype=torch.float64, device=dev())
    view = flat[1:1 + 4 * len(Q)].view(len(Q), 4)
    view.copy_(t64(Q))
    assert view.data_ptr() % 16 == 8 and torch_api.matrix_strides(view) == (4, 1)
    r = run(FOUR, Q_t=view)
    assert r["Qh"].tobytes() == four_contiguous["Qh"].tobytes()
    assert flat[0] == 9.75 and flat[-1] == 9.75


def test_padded_views(four_contiguous):
    _, _, QQ, Q = pack(FOUR)
    wq = torch.full((len(Q), 7), 55.5, dtype=torch.float64, device=dev())
    wqq = torch.full((len(QQ), 6), 123.5, dtype=torch.float64, device=dev())
    wq[:, 2:6] = t64(Q)
    wqq[:, 1:5] = t64(QQ)
    r = run(FOUR, QQ_t=wqq[:, 1:5], Q_t=wq[:, 2:6])
    assert r["Qh"].tobytes() == four_contiguous["Qh"].tobytes()
    assert (wq[:, :2] == 55.5).all() and (wq[:, 6] == 55.5).all() and (wqq[:, 0] == 123.5).all() and (wqq[:, 5] == 123.5).all()


def raw_call(sizes, I, QQ, qq_strides, Q, q_strides, res=True):
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    p = lambda t: C.c_void_p(t if isinstance(t, int) else t.data_ptr())
    status = np.full(len(sizes), -99, dtype=np.int32)
    rc = capi.lib().irotavg_window_init_mst_batch_dev(
        len(sizes), sizes.ctypes.data_as(C.POINTER(C.c_int32)), p(I), p(QQ), qq_strides[0], qq_strides[1], p(Q), q_strides[0],
        q_strides[1], status.ctypes.data_as(C.POINTER(C.c_int32)) if res else None,
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, status


def test_negative_strides(four_contiguous):
    """torch has no negative strides: reversed buffers go through the raw call, the pointer at their last row"""
    sizes, I, QQ, Q = pack(FOUR)
    N, M = len(Q), len(QQ)
    buf = torch.full((N + 2, 4), 55.5, dtype=torch.float64, device=dev())
    buf[1:N + 1] = t64(Q[::-1])
    qq = t64(QQ[::-1, ::-1])                                      # rows and columns reversed
    ei = torch.tensor(I, dtype=torch.int32, device=dev())
    rc, status = raw_call(sizes, ei, qq.data_ptr() + 8 * (4 * M - 1), (-4, -1), buf.data_ptr() + 32 * N, (-4, 1))
    assert rc == 0 and (status == 0).all()
    got = buf.cpu().numpy()
    assert got[1:N + 1][::-1].tobytes() == four_contiguous["Qh"].tobytes()
    assert (got[0] == 55.5).all() and (got[N + 1] == 55.5).all()


def test_without_results_and_with_int64_ids(four_contiguous):
    sizes, I, QQ, Q = pack(FOUR)
    Q_t = t64(Q)
    rc, status = raw_call(sizes, torch.tensor(I, dtype=torch.int32, device=dev()), t64(QQ), (4, 1), Q_t, (4, 1), res=False)
    assert rc == 0 and (status == -99).all() and Q_t.cpu().numpy().tobytes() == four_contiguous["Qh"].tobytes()
    assert run(FOUR, int64=True)["Qh"].tobytes() == four_contiguous["Qh"].tobytes()
    big = I.astype(np.int64)
    big[3, 0] += 2 ** 32                                          # would alias a valid id if it were merely truncated
    r = run(FOUR, I=big, int64=True, allow_rc=(capi.ERR_BAD_ARG,))
    assert list(r["status"]) == [capi.ERR_BAD_ARG, 0, 0, 0]


def test_refusals_with_a_device_leave_q_alone():
    sizes, I, QQ, Q = pack(FOUR)
    ei, qq, q = torch.tensor(I, dtype=torch.int32, device=dev()), t64(QQ), t64(Q)
    host_q = np.zeros((len(Q), 4))
    f0 = sizes.copy()
    f0[2, 1] = 0
    for what, args in [("f = 0", (f0, ei, qq, (4, 1), q, (4, 1))),
                       ("host Q", (sizes, ei, qq, (4, 1), host_q.ctypes.data, (4, 1))),
                       ("aliasing Q strides", (sizes, ei, qq, (4, 1), q, (2, 1))),
                       ("Q too short for its strides", (sizes, ei, qq, (4, 1), q, (2 ** 31, 1))),
                       ("misaligned I", (sizes, ei.data_ptr() + 4, qq, (4, 1), q, (4, 1)))]:
        rc, status = raw_call(*args)
        assert rc == capi.ERR_BAD_ARG and (status == -99).all(), what
        assert q.cpu().numpy().tobytes() == Q.tobytes(), what


def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream(four_contiguous):
    sizes, I, QQ, Q = pack(FOUR)
    ei = torch.tensor(I, dtype=torch.int32, device=dev())
    qq_half, q_half = t64(QQ * 0.5), t64(Q * 0.5)
    big = torch.ones(1 << 25, dtype=torch.float64, device=dev())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = big
        for _ in range(16):                                       # keeps the stream busy while the call is made
            busy = busy * 1.5
        qq_t, q_t = qq_half * 2.0, q_half * 2.0                   # exact: the inputs of the synchronised run, produced on the stream
        r = torch_api.window_init_mst_batch(sizes, ei, qq_t, q_t)
        doubled = q_t * 2.0                                       # consumed right behind the call, no synchronise
    side.synchronize()
    assert busy[0] == 1.5 ** 16 and busy[-1] == 1.5 ** 16
    assert (doubled.cpu().numpy() * 0.5).tobytes() == four_contiguous["Qh"].tobytes()
    assert (r["status"] == 0).all()


# ---- 12. the chain: init -> solve ----------------------------------------------------------------------------------------------
def solvable(name, nv, f, m, seed):
    """tree_case with measurements that agree with a ground truth up to 0.01 rad of noise, fixed rows at the truth"""
    c = tree_case(name, nv, f, m, seed)
    rng = np.random.default_rng([seed, 77])
    gt = unit(rng, nv)
    loop = c["I"][:, 0] == c["I"][:, 1]                           # the solvers take no self-loops: the next view instead
    c["I"][loop, 1] = (c["I"][loop, 0] + 1) % nv
    c["I"] = np.sort(c["I"], axis=1)                              # second end the higher id: an edge into a fixed view has no row
    a, b = c["I"][:, 0], c["I"][:, 1]
    c["QQ"] = synth.qmul(synth.qexp(rng.normal(scale=0.01, size=(m, 3))), synth.qmul(gt[b], synth.qconj(gt[a])))
    c["Q0"][:f] = gt[:f]
    return c


SOLVE = [solvable("solve-12", 12, 1, 40, 1), solvable("solve-30", 30, 3, 120, 2), solvable("solve-70", 70, 6, 300, 3),
         solvable("solve-4", 4, 1, 8, 4)]


def test_init_then_solve_is_bitwise_the_host_chain():
    sizes, I, QQ, Q = pack(SOLVE)
    ei, qq, q = torch.tensor(I, dtype=torch.int32, device=dev()), t64(QQ), t64(Q)
    r0 = torch_api.window_init_mst_batch(sizes, ei, qq, q)
    r = torch_api.window_solve_batch(sizes, ei, qq, r0["Q"], 4, SIG, 100, 100, 1e-3)   # the tensor the first call returned
    torch.cuda.synchronize()
    Qh, wh = q.cpu().numpy(), r["weights"].cpu().numpy()
    eo, vo = slices(SOLVE)
    assert (r0["status"] == 0).all() and (r["status"] == 0).all() and set(r["kernel"]) == {1, 2}
    for b, c in enumerate(SOLVE):
        rc, Qi = host(c)
        assert rc == 0
        a = capi.window_solve(c["I"], c["QQ"], Qi, c["f"], 4, SIG, 100, 100, 1e-3, kernel=int(r["kernel"][b]))
        assert (r["l1_iters"][b], r["irls_iters"][b]) == (a["l1_iters"], a["irls_iters"]), c["name"]
        assert a["irls_iters"] >= 1
        assert Qh[vo[b]:vo[b + 1]].tobytes() == np.ascontiguousarray(a["Q"]).tobytes(), c["name"]
        assert wh[eo[b]:eo[b + 1]].tobytes() == a["weights"].tobytes(), c["name"]
