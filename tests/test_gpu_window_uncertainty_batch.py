"""irotavg_window_uncertainty and irotavg_window_uncertainty_batch_dev on the device (irotavg_amd/csrc/wincov.hip, devapi.hip,
capi.cpp; capi.window_uncertainty, torch_api.window_uncertainty_batch; docs/window_uncertainty_batch.md).

Two yardsticks. The single-problem call is held against the NumPy reference of test_window_uncertainty_cpu.py: relative
1e-9 where the reference is finite and non-zero, NaN / +inf / 0 positions exact (assert_same of
test_gpu_viewgraph_uncertainty.py). The batched call is held against the single-problem call, BITWISE: workgroup b runs
the body the single-problem kernel runs, on the same numbers. Both weight definitions everywhere: "supplied" (the weights
window_solve returned, at the rotations it returned) and "poses" (weights = None: 1 / (|r|^2 + sigma^2) at Q0).

The single-problem results are computed once per (case, mode, sigma, pairs) and shared (ALONE); so are the solves (SOLVED).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import window_cases as WC  # noqa: E402
from irotavg_amd import capi, torch_api  # noqa: E402
from test_window_uncertainty_cpu import (CASES, SIG, SMALL3, SUPPLIED_ONLY, consistency, named, pose_weights, reference,  # noqa: E402
                                         some_pairs)

pytestmark = pytest.mark.gpu
MARK = -7.0
KEYS = ("var", "pair_var", "edge_var", "leverage", "chi2")
MODES = ("supplied", "poses")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def t64(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev())


def assert_same(got, ref, what, rtol=1e-9):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    for cls in (np.isnan, np.isposinf, lambda x: x == 0):
        np.testing.assert_array_equal(cls(got), cls(ref), err_msg=what)
    fin = np.isfinite(ref) & (ref != 0)
    err = np.abs(got[fin] - ref[fin]) / np.abs(ref[fin])
    worst = float(err.max()) if err.size else 0.0
    print("%s: max relative error over %d entries: %.3e" % (what, int(fin.sum()), worst))
    assert worst < rtol, what


# ---- the state a query is made at ----------------------------------------------------------------------------------------------
SOLVED, ALONE = {}, {}


def state(c, mode):
    """(Q, weights or None) of problem c in a mode; computed once, never modified. A case with planted bridges keeps Q0
    (the bridges' residuals are part of the case) and gets d = 2 on them (see bridge_case)."""
    if mode == "poses":
        return c["Q0"], None
    if c["name"] not in SOLVED:
        r = capi.window_solve(c["I"], c["QQ"], c["Q0"], c["f"], 4, SIG, 100, 100, 1e-3)
        Q, w = np.ascontiguousarray(r["Q"]), r["weights"].copy()
        if "bridges" in c:
            Q = np.ascontiguousarray(c["Q0"], dtype=np.float64)
            w[c["bridges"]] = 2.0
        for a in (Q, w):
            a.setflags(write=False)
        SOLVED[c["name"]] = (Q, w)
    return SOLVED[c["name"]]


def alone(c, mode, pairs=None, sigma=SIG):
    """capi.window_uncertainty on the problem alone, all outputs; computed once, never modified"""
    P = some_pairs(c) if pairs is None else pairs
    key = (c["name"], mode, sigma, P.tobytes())
    if key not in ALONE:
        Q, w = state(c, mode)
        r = capi.window_uncertainty(c["I"], c["QQ"], Q, c["f"], weights=w, sigma=sigma, pairs=P if len(P) else None)
        assert r["rc"] == 0
        for k in KEYS:
            r[k].setflags(write=False)
        ALONE[key] = r
    return ALONE[key]


# ---- 1. the single-problem call against the references --------------------------------------------------------------------------
SINGLE = [(c, m) for c in CASES for m in MODES] + [(c, "supplied") for c in SUPPLIED_ONLY]


@pytest.mark.parametrize("c,mode", SINGLE, ids=["%s-%s" % (c["name"], m) for c, m in SINGLE])
def test_single_problem_against_the_references(c, mode):
    Q, w = state(c, mode)
    d = pose_weights(c) if w is None else w
    assert consistency(c, d) < 1e-9                        # the reference is trustworthy at these weights
    P = some_pairs(c)
    ref = reference(c, d, P, Q)
    got = alone(c, mode, sigma=c["sigma"])
    for k in KEYS:
        assert_same(got[k], ref[k], "%s %s %s" % (c["name"], mode, k))
    print("scale %r, reference %r" % (got["scale"], ref["scale"]))
    assert got["scale"] == pytest.approx(ref["scale"], rel=1e-9, nan_ok=True)
    assert abs(got["leverage"].sum() - c["nu"]) <= 1e-9 * c["nu"]
    assert (got["var"][:c["f"]] == 0).all() and got["pair_var"][0] == 0 and got["pair_var"][1] == 0   # i == j
    for k in c.get("bridges", []):
        assert got["leverage"][k] == 1.0 and not np.isfinite(got["chi2"][k])
    if (c["nu"], c["ne"]) == (1, 1):
        assert np.isnan(got["scale"]) and np.isnan(got["chi2"]).all() and np.isfinite(got["var"]).all()
    again = capi.window_uncertainty(c["I"], c["QQ"], Q, c["f"], weights=w, sigma=c["sigma"], pairs=P)
    for k in KEYS:                                         # two identical calls: bitwise equal
        assert again[k].tobytes() == got[k].tobytes(), k
    assert np.array([again["scale"]]).tobytes() == np.array([got["scale"]]).tobytes()


def test_single_problem_failures_leave_the_outputs():
    c = CASES[2]
    Q, w = state(c, "supplied")
    w = w.copy()
    v = c["f"] + 3
    w[(c["I"][:, 0] == v) | (c["I"][:, 1] == v)] = 0.0      # nothing holds view v: singular
    r = capi.window_uncertainty(c["I"], c["QQ"], Q, c["f"], weights=w, pairs=some_pairs(c), allow_rc=(capi.ERR_SOLVER,))
    assert r["rc"] == capi.ERR_SOLVER and np.isnan(r["scale"])
    for k in KEYS:
        assert np.isnan(r[k]).all(), k                      # (the wrapper presets NaN)


# ---- 2. the batch is bitwise the single-problem call ----------------------------------------------------------------------------
def pack(cases, mode, pairs=None):
    """the packed arrays of a batch; pairs: per problem an (np, 2) array (default some_pairs; an empty one: no pairs)"""
    st = [state(c, mode) for c in cases]
    P = [some_pairs(c) for c in cases] if pairs is None else pairs
    return dict(sizes=np.array([(c["nv"], c["f"], c["ne"]) for c in cases], dtype=np.int32),
                I=np.concatenate([c["I"] for c in cases]).astype(np.int32),
                QQ=np.concatenate([c["QQ"] for c in cases]).astype(np.float64),
                Q=np.concatenate([q for q, _ in st]).astype(np.float64),
                w=None if mode == "poses" else np.concatenate([w for _, w in st]),
                P=P, npairs=np.array([len(p) for p in P], dtype=np.int32),
                pairs=np.concatenate(P).astype(np.int32).reshape(-1, 2))


def run(cases, mode, pairs=None, allow_rc=(), QQ_t=None, Q_t=None, I=None, pairs_flat=None, w=None, ids=torch.int32,
        want=(True, True, True, True)):
    """torch_api.window_uncertainty_batch with every output preset to MARK"""
    p = pack(cases, mode, pairs)
    n, m = len(p["Q"]), len(p["I"])
    ei = torch.tensor(p["I"] if I is None else I, dtype=ids, device=dev())
    QQ_t = t64(p["QQ"]) if QQ_t is None else QQ_t
    Q_t = t64(p["Q"]) if Q_t is None else Q_t
    w = p["w"] if w is None else w
    outs = [torch.full((k,), MARK, dtype=torch.float64, device=dev()) if on else False
            for k, on in zip((n, m, m, m), want)]
    flat = p["pairs"] if pairs_flat is None else pairs_flat
    has = len(flat) > 0
    r = torch_api.window_uncertainty_batch(p["sizes"], ei, QQ_t, Q_t, None if w is None else t64(w), SIG,
                                           torch.tensor(flat, dtype=ids, device=dev()) if has else None,
                                           p["npairs"] if has else None, *outs, allow_rc=allow_rc)
    torch.cuda.synchronize()
    assert Q_t.cpu().numpy().tobytes() == p["Q"].tobytes()                  # Q is never written
    r["host"] = {k: None if r[k] is None else r[k].cpu().numpy() for k in KEYS}
    r["packed"] = p
    return r


def slices(p):
    s = p["sizes"].astype(np.int64)
    cs = lambda a: np.concatenate([[0], np.cumsum(a)])
    return cs(s[:, 2]), cs(s[:, 0]), cs(p["npairs"].astype(np.int64))


def assert_bitwise(cases, mode, r, only=None):
    p = r["packed"]
    eo, vo, po = slices(p)
    for b, c in enumerate(cases):
        if only is not None and b not in only:
            continue
        a = alone(c, mode, p["P"][b])
        assert r["status"][b] == 0, (c["name"], r["status"][b])
        for k, off in (("var", vo), ("pair_var", po), ("edge_var", eo), ("leverage", eo), ("chi2", eo)):
            if r["host"][k] is None:
                continue
            assert r["host"][k][off[b]:off[b + 1]].tobytes() == a[k].tobytes(), (c["name"], k)
        assert np.array([r["scale"][b]]).tobytes() == np.array([a["scale"]]).tobytes(), c["name"]


MIXED = CASES + SUPPLIED_ONLY


@pytest.mark.parametrize("mode", MODES)
def test_mixed_batch_is_bitwise_the_single_problem_calls(mode):
    cases = MIXED if mode == "supplied" else CASES
    r = run(cases, mode)
    assert r["rc"] == 0
    assert_bitwise(cases, mode, r)
    rev = cases[::-1]
    assert_bitwise(rev, mode, run(rev, mode))              # the same batch reversed


@pytest.mark.parametrize("mode", MODES)
def test_more_workgroups_than_compute_units(mode):
    cases = [SMALL3[b % 3] for b in range(1026)]
    assert 1026 > 1024 >= torch.cuda.get_device_properties(dev()).multi_processor_count
    r = run(cases, mode)
    assert r["rc"] == 0 and (r["status"] == 0).all()
    assert_bitwise(cases, mode, r)


@pytest.mark.parametrize("mode", MODES)
def test_pairs_for_some_problems_only_and_more_than_one_launch_stages(mode):
    """problem 1 has 1500 pairs (the single-problem call stages 1024 per launch), problems 0 and 3 none"""
    cases = [CASES[2], CASES[4], CASES[1], CASES[6], CASES[5]]
    rng = np.random.default_rng(8)
    none = np.zeros((0, 2), dtype=np.int32)
    P = [none, rng.integers(0, cases[1]["nv"], size=(1500, 2)).astype(np.int32), some_pairs(cases[2]), none,
         some_pairs(cases[4], k=40, seed=3)]
    r = run(cases, mode, pairs=P)
    assert r["rc"] == 0 and len(r["host"]["pair_var"]) == 1500 + len(P[2]) + len(P[4])
    assert_bitwise(cases, mode, r)


def test_outputs_that_are_not_asked_for_are_not_needed():
    cases = CASES[1:5]
    full = run(cases, "supplied")
    for want in ((True, False, False, False), (False, False, True, False), (False, True, False, True)):
        r = run(cases, "supplied", want=want)
        assert r["rc"] == 0
        for k, on in zip(("var", "edge_var", "leverage", "chi2"), want):
            assert (r[k] is not None) == on
            if on:
                assert r["host"][k].tobytes() == full["host"][k].tobytes(), k
        assert r["host"]["pair_var"].tobytes() == full["host"]["pair_var"].tobytes()
        assert r["scale"].tobytes() == full["scale"].tobytes()


# ---- 3. chained behind the solve, no host synchronise between them ---------------------------------------------------------------
def test_chained_behind_the_batched_solve_on_one_stream():
    cases = [c for c in CASES if "bridges" not in c]
    p = pack(cases, "poses")
    ei = torch.tensor(p["I"], dtype=torch.int32, device=dev())
    QQ_t, Q_t = t64(p["QQ"]), t64(p["Q"])
    flat = torch.tensor(p["pairs"], dtype=torch.int32, device=dev())
    s = torch_api.window_solve_batch(p["sizes"], ei, QQ_t, Q_t, 4, SIG, 100, 100, 1e-3)
    r = torch_api.window_uncertainty_batch(p["sizes"], ei, QQ_t, s["Q"], s["weights"], SIG, flat, p["npairs"])
    torch.cuda.synchronize()
    assert s["rc"] == 0 and r["rc"] == 0
    Qh, wh = Q_t.cpu().numpy(), s["weights"].cpu().numpy()
    eo, vo, po = slices(p)
    host = {k: r[k].cpu().numpy() for k in KEYS}
    for b, c in enumerate(cases):
        Q, d = Qh[vo[b]:vo[b + 1]], wh[eo[b]:eo[b + 1]]
        assert consistency(c, d) < 1e-9
        ref = reference(c, d, p["P"][b], Q)
        for k, off in (("var", vo), ("pair_var", po), ("edge_var", eo), ("leverage", eo), ("chi2", eo)):
            assert_same(host[k][off[b]:off[b + 1]], ref[k], "%s %s" % (c["name"], k))
        assert r["scale"][b] == pytest.approx(ref["scale"], rel=1e-9, nan_ok=True)


# ---- 4. layouts ------------------------------------------------------------------------------------------------------------------
FOUR = [CASES[2], CASES[5], CASES[1], CASES[6]]


@pytest.fixture(scope="module")
def four():
    r = run(FOUR, "supplied")
    assert_bitwise(FOUR, "supplied", r)
    return r


def same_outputs(r, ref):
    for k in KEYS:
        assert r["host"][k].tobytes() == ref["host"][k].tobytes(), k
    assert r["scale"].tobytes() == ref["scale"].tobytes() and (r["status"] == 0).all()


def test_qq_as_columns_of_a_wider_tensor(four):
    QQ = four["packed"]["QQ"]
    wide = torch.full((len(QQ), 6), 123.5, dtype=torch.float64, device=dev())
    wide[:, 1:5] = t64(QQ)
    same_outputs(run(FOUR, "supplied", QQ_t=wide[:, 1:5]), four)


def test_q_as_four_planes_with_rows_beyond_the_batch(four):
    Q = four["packed"]["Q"]
    N = len(Q)
    planes = torch.full((4, N + 5), 321.25, dtype=torch.float64, device=dev())
    planes[:, :N] = t64(Q).t()
    r = run(FOUR, "supplied", Q_t=planes[:, :N].t())
    same_outputs(r, four)
    assert (planes[:, N:] == 321.25).all()


def test_qq_behind_a_pointer_that_is_8_but_not_16_byte_aligned(four):
    QQ = four["packed"]["QQ"]
    flat = torch.full((4 * len(QQ) + 2,), 9.75, dtype=torch.float64, device=dev())
    view = flat[1:1 + 4 * len(QQ)].view(len(QQ), 4)
    view.copy_(t64(QQ))
    assert view.data_ptr() % 16 == 8 and torch_api.matrix_strides(view) == (4, 1)
    same_outputs(run(FOUR, "supplied", QQ_t=view), four)


def test_int64_ids_are_narrowed_on_the_device(four):
    same_outputs(run(FOUR, "supplied", ids=torch.int64), four)


class Raw:
    """the C call itself on marker-filled outputs"""

    def __init__(self, cases, mode="supplied", pairs=None):
        self.p = p = pack(cases, mode, pairs)
        n, m, np_ = len(p["Q"]), len(p["I"]), len(p["pairs"])
        self.I = torch.tensor(p["I"], dtype=torch.int32, device=dev())
        self.QQ, self.Q = t64(p["QQ"]), t64(p["Q"])
        self.w = None if p["w"] is None else t64(p["w"])
        self.pairs = torch.tensor(p["pairs"], dtype=torch.int32, device=dev())
        mk = lambda k: torch.full((max(k, 1),), MARK, dtype=torch.float64, device=dev())
        self.out = dict(var=mk(n), pair_var=mk(np_), edge_var=mk(m), leverage=mk(m), chi2=mk(m))
        self.scale = np.full(len(cases), MARK)
        self.res = np.full(len(cases), -99, dtype=np.int32)

    def call(self, nb=None, sizes=None, Q=None, q_strides=(4, 1), QQ=None, qq_strides=(4, 1), npairs="own", pairs="own",
             pair_var="own", nothing=False, I=None):
        p = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
        i32 = C.POINTER(C.c_int32)
        sizes = np.ascontiguousarray(self.p["sizes"] if sizes is None else sizes, dtype=np.int32)
        npr = self.p["npairs"] if isinstance(npairs, str) else npairs
        o = {k: (None if nothing else v) for k, v in self.out.items()}
        rc = capi.lib().irotavg_window_uncertainty_batch_dev(
            len(sizes) if nb is None else nb, sizes.ctypes.data_as(i32), p(self.I if I is None else I),
            p(self.QQ if QQ is None else QQ), qq_strides[0], qq_strides[1], p(self.Q if Q is None else Q), q_strides[0],
            q_strides[1], p(self.w), SIG, p(o["var"]), None if npr is None else npr.ctypes.data_as(i32),
            p(self.pairs) if isinstance(pairs, str) else p(pairs), p(o["pair_var"]) if isinstance(pair_var, str) else p(pair_var),
            p(o["edge_var"]), p(o["leverage"]), p(o["chi2"]),
            None if nothing else self.scale.ctypes.data_as(C.POINTER(C.c_double)), self.res.ctypes.data_as(i32),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert self.Q.cpu().numpy().tobytes() == self.p["Q"].tobytes()      # Q is never written
        return rc

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def untouched(self):
        for k, v in self.host().items():
            assert (v == MARK).all(), k
        assert (self.scale == MARK).all() and (self.res == -99).all()


def test_q_with_a_negative_row_stride(four):
    """torch has no negative strides: the reversed buffer goes through the raw call, Q_dev = its last row, rs = -4"""
    R = Raw(FOUR)
    N = len(R.p["Q"])
    buf = torch.full((N + 2, 4), 55.5, dtype=torch.float64, device=dev())
    buf[1:N + 1] = t64(R.p["Q"][::-1])
    before = buf.cpu().numpy().tobytes()
    assert R.call(Q=buf.data_ptr() + 32 * N, q_strides=(-4, 1)) == 0
    for k, v in R.host().items():
        assert v.tobytes() == four["host"][k].tobytes(), k
    assert R.scale.tobytes() == four["scale"].tobytes() and (R.res == 0).all()
    assert buf.cpu().numpy().tobytes() == before


def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream(four):
    p = four["packed"]
    ei = torch.tensor(p["I"], dtype=torch.int32, device=dev())
    flat = torch.tensor(p["pairs"], dtype=torch.int32, device=dev())
    qq_half, q_half, w_half = t64(p["QQ"] * 0.5), t64(p["Q"] * 0.5), t64(p["w"] * 0.5)
    big = torch.ones(1 << 25, dtype=torch.float64, device=dev())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        busy = big
        for _ in range(16):                                # keeps the stream busy while the call is made
            busy = busy * 1.5
        qq_t, q_t, w_t = qq_half * 2.0, q_half * 2.0, w_half * 2.0          # exact: the inputs of the synchronised run
        r = torch_api.window_uncertainty_batch(p["sizes"], ei, qq_t, q_t, w_t, SIG, flat, p["npairs"])
        doubled = {k: r[k] * 2.0 for k in KEYS}            # consumed right behind the call, no synchronise
    side.synchronize()
    assert busy[0] == 1.5 ** 16 and busy[-1] == 1.5 ** 16
    for k in KEYS:
        assert (doubled[k].cpu().numpy() * 0.5).tobytes() == four["host"][k].tobytes(), k
    assert r["scale"].tobytes() == four["scale"].tobytes() and (r["status"] == 0).all()


# ---- 5. per-problem failures -------------------------------------------------------------------------------------------------------
def check_one_failed(R, cases, bad, status, rc):
    """problem `bad` reports `status` and keeps every marker; the other three are bitwise their single-problem results"""
    assert rc == status                                    # the first non-zero status (the only one)
    eo, vo, po = slices(R.p)
    h = R.host()
    for b, c in enumerate(cases):
        rows = dict(var=vo, pair_var=po, edge_var=eo, leverage=eo, chi2=eo)
        if b == bad:
            assert R.res[b] == status and R.scale[b] == MARK
            for k, off in rows.items():
                assert (h[k][off[b]:off[b + 1]] == MARK).all(), k
            continue
        a = alone(c, "supplied", R.p["P"][b])
        assert R.res[b] == 0
        for k, off in rows.items():
            assert h[k][off[b]:off[b + 1]].tobytes() == a[k].tobytes(), (c["name"], k)
        assert np.array([R.scale[b]]).tobytes() == np.array([a["scale"]]).tobytes()


@pytest.mark.parametrize("bad", [0, 2])
@pytest.mark.parametrize("value", ["nv", -1])
def test_an_edge_id_outside_the_problem_is_refused_by_its_workgroup_alone(bad, value):
    R = Raw(FOUR)
    eo, _, _ = slices(R.p)
    I = R.p["I"].copy()
    I[eo[bad] + FOUR[bad]["ne"] // 2, 1 if value == -1 else 0] = FOUR[bad]["nv"] if value == "nv" else -1
    check_one_failed(R, FOUR, bad, capi.ERR_BAD_ARG, R.call(I=torch.tensor(I, dtype=torch.int32, device=dev())))


@pytest.mark.parametrize("value", ["nv", -1, 2 ** 31 - 1])
def test_a_pair_id_outside_the_problem_is_refused_by_its_workgroup_alone(value):
    R = Raw(FOUR)
    _, _, po = slices(R.p)
    bad = 1
    flat = R.p["pairs"].copy()
    flat[po[bad] + 2, 1] = FOUR[bad]["nv"] if value == "nv" else value
    check_one_failed(R, FOUR, bad, capi.ERR_BAD_ARG, R.call(pairs=torch.tensor(flat, dtype=torch.int32, device=dev())))


def test_a_singular_problem_reports_it_and_keeps_its_rows():
    R = Raw(FOUR)
    eo, _, _ = slices(R.p)
    bad, c = 3, FOUR[3]
    v = c["f"] + 5
    w = R.p["w"].copy()
    hit = (c["I"][:, 0] == v) | (c["I"][:, 1] == v)
    assert hit.any()
    w[eo[bad]:eo[bad + 1]][hit] = 0.0                      # weight exactly 0 on every edge of one free view
    R.w = t64(w)
    check_one_failed(R, FOUR, bad, capi.ERR_SOLVER, R.call())


def test_the_first_failure_in_problem_order_is_returned():
    R = Raw(FOUR)
    eo, _, _ = slices(R.p)
    I = R.p["I"].copy()
    I[eo[2], 0] = -1                                       # problem 2: a bad id; problem 1: singular
    w = R.p["w"].copy()
    w[eo[1]:eo[2]] = 0.0
    R.w = t64(w)
    assert R.call(I=torch.tensor(I, dtype=torch.int32, device=dev())) == capi.ERR_SOLVER
    assert list(R.res) == [0, capi.ERR_SOLVER, capi.ERR_BAD_ARG, 0]


# ---- 6. whole-call refusals leave every marker ----------------------------------------------------------------------------------------
PAST = [p for p in WC.past_limits() if p[1] == 0]


@pytest.mark.parametrize("name,kernel,c", PAST, ids=[p[0] for p in PAST])
def test_one_problem_past_a_limit_refuses_the_batch(name, kernel, c):
    R = Raw(FOUR)
    sizes = np.concatenate([R.p["sizes"][:1], [[c["nv"], c["f"], len(c["I"])]], R.p["sizes"][1:]])
    assert R.call(sizes=sizes) == capi.ERR_BAD_ARG
    R.untouched()


def test_refusals_leave_every_marker():
    R = Raw(FOUR)
    N, M = len(R.p["Q"]), len(R.p["I"])
    host_q, host_pairs = np.zeros((N, 4)), np.zeros((max(len(R.p["pairs"]), 1), 2), dtype=np.int32)
    calls = [
        ("nb = 0", dict(nb=0)),
        ("nothing asked for", dict(nothing=True, npairs=None)),
        ("a pair count without the ids", dict(pairs=None)),
        ("a pair count without the output", dict(pair_var=None)),
        ("a negative pair count", dict(npairs=np.array([1, -1, 2, 3], dtype=np.int32))),
        ("host Q", dict(Q=host_q.ctypes.data)),
        ("host pairs", dict(pairs=host_pairs.ctypes.data)),
        ("aliasing Q strides", dict(q_strides=(2, 1))),
        ("QQ too short for its strides", dict(qq_strides=(1, 2 ** 31))),
        ("misaligned pairs", dict(pairs=R.pairs.data_ptr() + 4)),
        ("more pairs than the array holds", dict(npairs=np.array([1, 2, 3, 2 ** 30], dtype=np.int32))),
    ]
    for what, kw in calls:
        assert R.call(**kw) == capi.ERR_BAD_ARG, what
        R.untouched()
    assert R.call() == 0                                   # the same arguments without the fault
    assert (R.res == 0).all() and not (R.scale == MARK).any()
