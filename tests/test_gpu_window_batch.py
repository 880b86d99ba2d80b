"""irotavg_window_solve_batch_dev (irotavg_amd/csrc/window.hip, devapi.hip; torch_api.window_solve_batch; docs/window_batch.md):
many window-size problems on packed device arrays, one workgroup per problem.

The reference is the single-problem call. Workgroup b runs the body the single-problem kernels run, on the same
numbers, so for every problem of every batch Q, the weights and both iteration counts are BITWISE those of
capi.window_solve(..., kernel=k) on that problem alone, k being the kernel the batch reports for it. No tolerance.
The single-problem results are computed once per (case, kernel, cost, iteration limits) and shared (ALONE).

kernel = 1 is the general LDS kernel, 2 the wave-resident kernel, 0 the choice per problem.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import window_cases as WC  # noqa: E402
from irotavg_amd import capi, synth, torch_api  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
SIG = WC.SIG
W_MARK, R_MARK = -7.0, -99


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def t64(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev())


def named(name, c):
    c = dict(c)
    c["name"] = name
    c["ne"] = len(c["I"])
    c["nu"] = c["nv"] - c["f"]
    return c


LIMITS = [(named("limit-" + n, c), wave) for n, wave, c in WC.limits()]
SMALL = [named("small-%d-%d-%d" % s, WC.size_case(*s, seed=7)) for s in ((3, 5, 7), (20, 25, 90), (7, 8, 70))]
MIXED = [named("planted4", WC.planted(4)), named("star", WC.star())] + [c for c, _ in LIMITS] + SMALL
WAVE_TRIO = [named("w-%d-%d-%d" % s, WC.size_case(*s, seed=11)) for s in ((10, 12, 40), (16, 18, 64), (2, 4, 5))]
GENERAL_TRIO = [named("g-%d-%d-%d" % s, WC.size_case(*s, seed=12)) for s in ((17, 20, 80), (20, 30, 100), (24, 25, 65))]


def fits_wave(c):
    return c["nu"] <= 16 and c["ne"] <= 64


ALONE = {}


def alone(c, k, cost=4, l1=100, irls=100):
    """capi.window_solve on the problem alone; computed once, never modified"""
    key = (c["name"], k, cost, l1, irls)
    if key not in ALONE:
        r = capi.window_solve(c["I"], c["QQ"], c["Q0"], c["f"], cost, SIG, l1, irls, 1e-3, kernel=k)
        r["Q"] = np.ascontiguousarray(r["Q"])
        for a in (r["Q"], r["weights"]):
            a.setflags(write=False)
        ALONE[key] = r
    return ALONE[key]


def pack(cases):
    sizes = np.array([(c["nv"], c["f"], c["ne"]) for c in cases], dtype=np.int32)
    I = np.concatenate([c["I"] for c in cases]).astype(np.int32)
    QQ = np.concatenate([c["QQ"] for c in cases]).astype(np.float64)
    Q = np.concatenate([c["Q0"] for c in cases]).astype(np.float64)
    return sizes, I, QQ, Q


def run(cases, kernel=0, cost=4, l1=100, irls=100, QQ_t=None, Q_t=None, allow_rc=(), I=None):
    sizes, I0, QQ, Q = pack(cases)
    ei = torch.tensor(I0 if I is None else I, dtype=torch.int32, device=dev())
    QQ_t = t64(QQ) if QQ_t is None else QQ_t
    Q_t = t64(Q) if Q_t is None else Q_t
    w = torch.full((len(I0),), W_MARK, dtype=torch.float64, device=dev())
    r = torch_api.window_solve_batch(sizes, ei, QQ_t, Q_t, cost, SIG, l1, irls, 1e-3, kernel=kernel, weights=w,
                                     allow_rc=allow_rc)
    torch.cuda.synchronize()
    r["Qh"] = Q_t.cpu().numpy()
    r["wh"] = w.cpu().numpy()
    return r


def slices(cases):
    eo = np.concatenate([[0], np.cumsum([c["ne"] for c in cases])])
    vo = np.concatenate([[0], np.cumsum([c["nv"] for c in cases])])
    return eo, vo


def assert_bitwise(cases, r, cost=4, l1=100, irls=100, only=None):
    """every problem of the batch against the single-problem call with the kernel the batch reports"""
    eo, vo = slices(cases)
    for b, c in enumerate(cases):
        if only is not None and b not in only:
            continue
        k = int(r["kernel"][b])
        assert k in (1, 2), (c["name"], k)
        a = alone(c, k, cost, l1, irls)
        assert r["status"][b] == 0, (c["name"], r["status"][b])
        assert (r["l1_iters"][b], r["irls_iters"][b]) == (a["l1_iters"], a["irls_iters"]), c["name"]
        assert r["Qh"][vo[b]:vo[b + 1]].tobytes() == a["Q"].tobytes(), c["name"]
        assert r["wh"][eo[b]:eo[b + 1]].tobytes() == a["weights"].tobytes(), c["name"]
        assert r["Qh"][vo[b]:vo[b] + c["f"]].tobytes() == np.ascontiguousarray(c["Q0"][:c["f"]]).tobytes(), c["name"]


# ---- 0. the pinned block grows and is reused (first in the file: the block is process-wide and never shrinks) -----------------
GROW = [named("grow-%d" % b, WC.size_case(2, 3, 3, seed=100 + b)) for b in range(40)]  # 3 views, 1 fixed, 3 edges, 0.01 rad


def test_a_block_that_grew_is_reused():
    """1 problem, then 40, then the 1 again: the second call replaces the block of result records and descriptors by a
    larger one (40 need 5120 bytes, the first call reserved 192), the third finds it larger than it needs."""
    first, many, third = run(GROW[:1]), run(GROW), run(GROW[:1])
    assert (first["rc"], many["rc"], third["rc"]) == (0, 0, 0)
    for k in ("Qh", "wh", "status", "l1_iters", "irls_iters", "kernel"):
        assert np.asarray(first[k]).tobytes() == np.asarray(third[k]).tobytes(), k
    assert_bitwise(GROW[:1], first)
    assert_bitwise(GROW, many)


# ---- 1. mixed batch ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    return run(MIXED)


def test_mixed_batch_is_bitwise_the_single_problem_calls(mixed):
    assert mixed["rc"] == 0
    sizes = [(c["nu"], c["nv"], c["ne"]) for c in MIXED]
    assert (1, 2, 1) in sizes and (64, 320, 640) in sizes
    assert_bitwise(MIXED, mixed)


def test_mixed_batch_kernel_choice(mixed):
    flagged = {c["name"]: wave for c, wave in LIMITS}
    for b, c in enumerate(MIXED):
        want = flagged.get(c["name"], fits_wave(c))
        assert (mixed["kernel"][b] == 2) == want, (c["name"], mixed["kernel"][b])
    assert set(mixed["kernel"]) == {1, 2}


@pytest.mark.parametrize("c", [c for c, _ in LIMITS], ids=[c["name"] for c, _ in LIMITS])
def test_mixed_batch_limit_cases_match_the_oracle(mixed, c):
    """the bars of pipeline_vs_oracle (tests/test_gpu_window_limits.py)"""
    b = [x["name"] for x in MIXED].index(c["name"])
    eo, vo = slices(MIXED)
    a = O.l1ra(c["QQ"], c["I"], c["Q0"], c["f"], 100, 1e-3)
    o = O.irls(c["QQ"], c["I"], a["Q"], c["f"], 4, SIG, 100, 1e-3)
    assert (a["rc"], o["rc"]) == (0, 0)
    ang = synth.angular_distance(mixed["Qh"][vo[b]:vo[b + 1]], o["Q"]).max()
    print("%s: iters %d/%d (oracle %d/%d), max angular diff %.3e rad"
          % (c["name"], mixed["l1_iters"][b], mixed["irls_iters"][b], a["iters"], o["iters"], ang))
    assert (mixed["l1_iters"][b], mixed["irls_iters"][b]) == (a["iters"], o["iters"])
    assert ang < 1e-9
    np.testing.assert_allclose(mixed["wh"][eo[b]:eo[b + 1]], o["weights"], rtol=1e-7)


# ---- 2. order and occupancy ----------------------------------------------------------------------------------------------
def test_reversed_batch_gives_the_same_bits():
    rev = MIXED[::-1]
    assert_bitwise(rev, run(rev))


@pytest.mark.parametrize("trio,k", [(WAVE_TRIO, 2), (GENERAL_TRIO, 1)], ids=["wave", "general"])
def test_more_workgroups_than_compute_units(trio, k):
    cases = [trio[b % 3] for b in range(300)]
    assert 300 > torch.cuda.get_device_properties(dev()).multi_processor_count
    r = run(cases)
    assert (r["kernel"] == k).all()
    assert_bitwise(cases, r)


# ---- 3. forced kernels ---------------------------------------------------------------------------------------------------
def test_forced_general_kernel_on_the_mixed_batch():
    r = run(MIXED, kernel=1)
    assert (r["kernel"] == 1).all()
    assert_bitwise(MIXED, r)


def test_forced_wave_kernel_on_the_wave_fitting_subset():
    sub = [c for c in MIXED if fits_wave(c)]
    assert len(sub) >= 6
    r = run(sub, kernel=2)
    assert (r["kernel"] == 2).all()
    assert_bitwise(sub, r)


# ---- raw calls with every output preset to a marker ----------------------------------------------------------------------
class Raw:
    def __init__(self, cases, I=None):
        self.cases = cases
        self.sizes, I0, QQ, Q = pack(cases)
        self.I = torch.tensor(I0 if I is None else I, dtype=torch.int32, device=dev())
        self.QQ, self.Q = t64(QQ), t64(Q)
        self.Q_before = Q.copy()
        self.w = torch.full((max(len(I0), 1),), W_MARK, dtype=torch.float64, device=dev())
        self.res = np.full((len(cases), 4), R_MARK, dtype=np.int32)

    def call(self, nb=None, sizes=None, I=None, QQ=None, qq_strides=(4, 1), Q=None, q_strides=(4, 1), w="own", res="own",
             kernel=0, cost=4, l1=100, irls=100):
        sizes = self.sizes if sizes is None else sizes
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        p = lambda t: C.c_void_p(t if isinstance(t, int) else t.data_ptr())
        wp = p(self.w) if isinstance(w, str) else (None if w is None else p(w))
        rp = self.res.ctypes.data_as(C.POINTER(C.c_int32)) if isinstance(res, str) else None
        rc = capi.lib().irotavg_window_solve_batch_dev(
            len(sizes) if nb is None else nb, sizes.ctypes.data_as(C.POINTER(C.c_int32)), p(self.I if I is None else I),
            p(self.QQ if QQ is None else QQ), qq_strides[0], qq_strides[1], p(self.Q if Q is None else Q), q_strides[0],
            q_strides[1], cost, SIG, l1, irls, 1e-3, wp, rp, kernel,
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        assert self.Q.cpu().numpy().tobytes() == self.Q_before.tobytes()
        assert (self.w.cpu().numpy() == W_MARK).all()
        assert (self.res == R_MARK).all()


def test_forced_wave_kernel_refuses_a_problem_of_17_free_views():
    wave = [c for c in MIXED if fits_wave(c)][:3]
    R = Raw(wave + [named("nu17", WC.size_case(17, 18, 40, seed=3))])
    assert R.call(kernel=2) == capi.ERR_BAD_ARG
    R.untouched()
    assert R.call(kernel=0) == 0                       # the same batch is fine when every problem gets its kernel


# ---- 4. index guard ------------------------------------------------------------------------------------------------------
FOUR = [WAVE_TRIO[0], GENERAL_TRIO[0], WAVE_TRIO[2], GENERAL_TRIO[2]]


@pytest.mark.parametrize("bad_problem", [0, 1], ids=["wave-size", "general-size"])
@pytest.mark.parametrize("value", ["nv", -1])
def test_an_endpoint_outside_the_problem_is_refused_by_its_workgroup_alone(bad_problem, value):
    """the precedent: test_edge_index_out_of_range_is_a_bad_argument (tests/test_gpu_device_api.py)"""
    eo, vo = slices(FOUR)
    sizes, I, QQ, Q0 = pack(FOUR)
    c = FOUR[bad_problem]
    I = I.copy()
    I[eo[bad_problem] + c["ne"] // 2, 1] = c["nv"] if value == "nv" else -1
    r = run(FOUR, I=I, allow_rc=(capi.ERR_BAD_ARG,))
    assert r["rc"] == capi.ERR_BAD_ARG
    b = bad_problem
    assert (r["status"][b], r["l1_iters"][b], r["irls_iters"][b]) == (capi.ERR_BAD_ARG, 0, 0)
    assert r["Qh"][vo[b]:vo[b + 1]].tobytes() == Q0[vo[b]:vo[b + 1]].tobytes()
    assert (r["wh"][eo[b]:eo[b + 1]] == W_MARK).all()
    assert_bitwise(FOUR, r, only=[x for x in range(4) if x != b])
    assert_bitwise(FOUR, run(FOUR))                    # a valid call afterwards


# ---- 5. all 14 costs -----------------------------------------------------------------------------------------------------
PLANTED = [named("planted%d" % cost, WC.planted(cost)) for cost in range(14)]


@pytest.mark.parametrize("kernel", [1, 2])
def test_every_cost_one_pass(kernel):
    """cost is per call: 14 calls on the batch of all 14 planted problems, problem `cost` is read from call `cost`"""
    eo, vo = slices(PLANTED)
    for cost, c in enumerate(PLANTED):
        r = run(PLANTED, kernel=kernel, cost=cost, l1=0, irls=1)
        assert (r["kernel"] == kernel).all()
        assert_bitwise(PLANTED, r, cost=cost, l1=0, irls=1, only=[cost])
        w = r["wh"][eo[cost]:eo[cost + 1]]
        E, ref = WC.planted_reference(c, cost)
        got = w[c["planted"]]
        rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
        print("kernel %d cost %d: planted max rel diff %.3e" % (kernel, cost, rel.max()))
        for name, g, x in zip(WC.classify(cost, SIG, E), got, ref):
            if name in WC.CONST_VALUE:
                assert g == x == WC.CONST_VALUE[name], (cost, name, g, x)
        np.testing.assert_allclose(got, ref, rtol=1e-11, atol=0)


# ---- 6. strides ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def four_contiguous():
    r = run(FOUR)
    assert_bitwise(FOUR, r)
    return r


def test_qq_as_columns_of_a_wider_tensor(four_contiguous):
    _, _, QQ, _ = pack(FOUR)
    wide = torch.full((len(QQ), 6), 123.5, dtype=torch.float64, device=dev())
    wide[:, 1:5] = t64(QQ)
    r = run(FOUR, QQ_t=wide[:, 1:5])
    assert r["Qh"].tobytes() == four_contiguous["Qh"].tobytes() and r["wh"].tobytes() == four_contiguous["wh"].tobytes()
    assert (wide[:, 0] == 123.5).all() and (wide[:, 5] == 123.5).all()


def test_q_as_four_planes_with_rows_beyond_the_batch(four_contiguous):
    _, _, _, Q = pack(FOUR)
    N = len(Q)
    planes = torch.full((4, N + 5), 321.25, dtype=torch.float64, device=dev())
    planes[:, :N] = t64(Q).t()
    r = run(FOUR, Q_t=planes[:, :N].t())
    assert r["Qh"].tobytes() == four_contiguous["Qh"].tobytes() and r["wh"].tobytes() == four_contiguous["wh"].tobytes()
    assert (planes[:, N:] == 321.25).all()


def test_q_with_a_negative_row_stride(four_contiguous):
    """torch has no negative strides: the reversed buffer goes through the raw call, Q_dev = its last row, rs = -4"""
    R = Raw(FOUR)
    N = len(R.Q_before)
    buf = torch.full((N + 2, 4), 55.5, dtype=torch.float64, device=dev())
    buf[1:N + 1] = t64(R.Q_before[::-1])
    assert R.call(Q=buf.data_ptr() + 32 * N, q_strides=(-4, 1)) == 0
    got = buf.cpu().numpy()
    assert got[1:N + 1][::-1].tobytes() == four_contiguous["Qh"].tobytes()
    assert R.w.cpu().numpy().tobytes() == four_contiguous["wh"].tobytes()
    assert (got[0] == 55.5).all() and (got[N + 1] == 55.5).all()


def test_qq_behind_a_pointer_that_is_8_but_not_16_byte_aligned(four_contiguous):
    _, _, QQ, _ = pack(FOUR)
    flat = torch.full((4 * len(QQ) + 2,), 9.75, dtype=torch.float64, device=dev())
    view = flat[1:1 + 4 * len(QQ)].view(len(QQ), 4)
    view.copy_(t64(QQ))
    assert view.data_ptr() % 16 == 8 and torch_api.matrix_strides(view) == (4, 1)
    r = run(FOUR, QQ_t=view)
    assert r["Qh"].tobytes() == four_contiguous["Qh"].tobytes() and r["wh"].tobytes() == four_contiguous["wh"].tobytes()
    assert flat[0] == 9.75 and flat[-1] == 9.75


# ---- 7. stream ordering --------------------------------------------------------------------------------------------------
def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream(four_contiguous):
    sizes, I, QQ, Q = pack(FOUR)
    ei = torch.tensor(I, dtype=torch.int32, device=dev())
    qq_half, q_half = t64(QQ * 0.5), t64(Q * 0.5)
    big = torch.ones(1 << 25, dtype=torch.float64, device=dev())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = big
        for _ in range(16):                            # keeps the stream busy while the call is made
            busy = busy * 1.5
        qq_t, q_t = qq_half * 2.0, q_half * 2.0        # exact: the inputs of the synchronised run, produced on the stream
        r = torch_api.window_solve_batch(sizes, ei, qq_t, q_t, 4, SIG, 100, 100, 1e-3)
        doubled = q_t * 2.0                            # consumed right behind the call, no synchronise
    side.synchronize()
    assert busy[0] == 1.5 ** 16 and busy[-1] == 1.5 ** 16
    assert (doubled.cpu().numpy() * 0.5).tobytes() == four_contiguous["Qh"].tobytes()
    assert r["weights"].cpu().numpy().tobytes() == four_contiguous["wh"].tobytes()
    assert (r["status"] == 0).all() and (r["kernel"] == four_contiguous["kernel"]).all()


# ---- 8. refusals before any device work ----------------------------------------------------------------------------------
PAST = WC.past_limits()


@pytest.mark.parametrize("name,kernel,c", PAST, ids=[p[0] for p in PAST])
def test_one_problem_past_a_limit_refuses_the_batch(name, kernel, c):
    R = Raw([FOUR[0], named(name, c), FOUR[1]] if kernel != 2 else [FOUR[0], named(name, c), FOUR[2]])
    assert R.call(kernel=kernel) == capi.ERR_BAD_ARG
    R.untouched()


def test_refusals_leave_every_marker():
    R = Raw(FOUR)
    N, M = len(R.Q_before), len(R.I)
    host_q, host_qq = np.zeros((N, 4)), np.zeros((M, 4))
    host_i = np.zeros((M, 2), dtype=np.int32)
    host_w = torch.zeros(M, dtype=torch.float64)
    calls = [
        ("nb = 0", dict(nb=0)),
        ("nb < 0", dict(nb=-4)),
        ("kernel 3", dict(kernel=3)),
        ("host I", dict(I=host_i.ctypes.data)),
        ("host QQ", dict(QQ=host_qq.ctypes.data)),
        ("host Q", dict(Q=host_q.ctypes.data)),
        ("host weights", dict(w=host_w)),
        ("aliasing QQ strides", dict(qq_strides=(2, 1))),
        ("aliasing Q strides", dict(q_strides=(2, 1))),
        ("zero stride", dict(q_strides=(4, 0))),
        ("Q too short for its strides", dict(q_strides=(2 ** 31, 1))),
        ("QQ too short for its strides", dict(qq_strides=(1, 2 ** 31))),
        ("misaligned I", dict(I=R.I.data_ptr() + 4)),
        ("misaligned Q", dict(Q=R.Q.data_ptr() + 4)),
    ]
    for what, kw in calls:
        assert R.call(**kw) == capi.ERR_BAD_ARG, what
        R.untouched()
    for cost in (-1, 14):
        assert R.call(cost=cost) == capi.ERR_UNKNOWN_COST
        R.untouched()
    assert R.call() == 0                               # the same arguments without the fault
    assert (R.res[:, 0] == 0).all()


def test_sixty_five_thousand_problems():
    """the documented cap is above 65 536: that many one-edge problems (nu 1, nv 2) in one call, l1 0 / irls 1"""
    c = named("tiny", WC.size_case(1, 2, 1))
    nb = 65536
    sizes = np.tile(np.array([[2, 1, 1]], dtype=np.int32), (nb, 1))
    ei = torch.tensor(c["I"], dtype=torch.int32, device=dev()).repeat(nb, 1)
    QQ, Q = t64(c["QQ"]).repeat(nb, 1), t64(c["Q0"]).repeat(nb, 1)
    r = torch_api.window_solve_batch(sizes, ei, QQ, Q, 4, SIG, 0, 1, 1e-3)
    a = alone(c, 2, 4, 0, 1)
    assert (r["status"] == 0).all() and (r["kernel"] == 2).all() and (r["irls_iters"] == a["irls_iters"]).all()
    Qh = Q.cpu().numpy().reshape(nb, -1)
    assert (Qh.view(np.uint64) == a["Q"].reshape(1, -1).view(np.uint64)).all()
    assert (r["weights"].cpu().numpy().view(np.uint64) == a["weights"].view(np.uint64)[0]).all()


# ---- 9. optional outputs -------------------------------------------------------------------------------------------------
def test_without_weights_and_results(four_contiguous):
    R = Raw(FOUR)
    assert R.call(w=None, res=None) == 0
    assert R.Q.cpu().numpy().tobytes() == four_contiguous["Qh"].tobytes()
    assert (R.w.cpu().numpy() == W_MARK).all() and (R.res == R_MARK).all()


def test_int64_edge_index_is_narrowed_on_the_device(four_contiguous):
    sizes, I, QQ, Q = pack(FOUR)
    Q_t = t64(Q)
    r = torch_api.window_solve_batch(sizes, torch.tensor(I, dtype=torch.int64, device=dev()), t64(QQ), Q_t)
    assert Q_t.cpu().numpy().tobytes() == four_contiguous["Qh"].tobytes()
    assert r["weights"].cpu().numpy().tobytes() == four_contiguous["wh"].tobytes()
