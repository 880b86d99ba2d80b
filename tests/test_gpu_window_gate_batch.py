"""irotavg_window_gate and irotavg_window_gate_batch_dev on the device (irotavg_amd/csrc/wincov.hip, devapi.hip, capi.cpp;
capi.window_gate, torch_api.window_gate_batch; docs/window_gate_batch.md).

Two yardsticks, as in test_gpu_window_uncertainty_batch.py. The single-problem call is held against the NumPy reference
of test_window_gate_cpu.py with assert_same of test_gpu_viewgraph_uncertainty.py: relative 1e-9 where the reference is
finite and non-zero, NaN / +inf / 0 positions exact. The batched call is held against the single-problem call, BITWISE.
Both weight definitions: "supplied" (the weights window_solve returned, at the rotations it returned) and "poses"
(weights = None: 1 / (|r|^2 + sigma^2) at Q0).

The candidates of a (case, mode) are one list of 600 (candidate_set: the named ones first, then random ones); a count n
takes its first n. The single-problem results are computed once per (case, mode, n, sigma) and shared (ALONE)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
from irotavg_amd import capi, torch_api, viewgraph  # noqa: E402
from test_gpu_viewgraph_uncertainty import assert_same  # noqa: E402
from test_gpu_window_uncertainty_batch import dev, state, t64  # noqa: E402
from test_viewgraph_uncertainty_cpu import extract_problem, make_pair  # noqa: E402
from test_window_gate_cpu import (GATE_TRUE, NEGATED, assert_negation_changes_nothing, candidate_set, gate_reference,  # noqa: E402
                                  planted_closures)
from test_window_uncertainty_cpu import CASES, SIG, SMALL3, consistency, pose_weights  # noqa: E402

pytestmark = pytest.mark.gpu
MARK = -7.0
KEYS = ("angle", "pair_var", "chi2")
MODES = ("supplied", "poses")
MOST = 600
COUNTS = (1, 255, 256, 257, 600)   # around the single call's 256 per launch and the kernel's 256-thread stride


# ---- the candidates and the single-problem call, shared ------------------------------------------------------------------------
CANDS, ALONE, NAMES = {}, {}, {}


def cands_of(c, mode, n):
    """the first n of the 600 candidates of (case, mode), made at the poses of that mode"""
    key = (c["name"], mode)
    if key not in CANDS:
        cI, cQ, NAMES[key] = candidate_set(c, state(c, mode)[0], MOST)
        for a in (cI, cQ):
            a.setflags(write=False)
        CANDS[key] = (cI, cQ)
    cI, cQ = CANDS[key]
    return cI[:n], cQ[:n]


def alone(c, mode, n, sigma=SIG):
    """capi.window_gate on the problem alone, all outputs; computed once, never modified"""
    key = (c["name"], mode, n, sigma)
    if key not in ALONE:
        Q, w = state(c, mode)
        cI, cQ = cands_of(c, mode, n)
        r = capi.window_gate(c["I"], c["QQ"], Q, c["f"], cI, cQ, weights=w, sigma=sigma)
        assert r["rc"] == 0
        for k in KEYS:
            r[k].setflags(write=False)
        ALONE[key] = r
    return ALONE[key]


# ---- 1. the single-problem call against the reference ----------------------------------------------------------------------------
SINGLE = [(c, m) for c in CASES for m in MODES]


@pytest.mark.parametrize("c,mode", SINGLE, ids=["%s-%s" % (c["name"], m) for c, m in SINGLE])
def test_single_problem_against_the_reference(c, mode):
    Q, w = state(c, mode)
    d = pose_weights(c) if w is None else w
    assert consistency(c, d) < 1e-9                        # the reference is trustworthy at these weights
    ref = gate_reference(c, d, cands_of(c, mode, MOST), Q)
    for n in COUNTS:
        got = alone(c, mode, n, sigma=c["sigma"])
        for k in KEYS:
            assert_same(got[k], ref[k][:n], "%s %s %d %s" % (c["name"], mode, n, k))
        assert got["scale"] == pytest.approx(ref["scale"], rel=1e-9, nan_ok=True)
        assert (got["pair_var"] >= 0).all() and np.isfinite(got["angle"]).all()
    if (c["nu"], c["ne"]) == (1, 1):
        assert np.isnan(got["scale"]) and np.isnan(got["chi2"]).all() and np.isfinite(got["pair_var"]).all()
    at = {name: k for k, name in enumerate(NAMES[(c["name"], mode)]) if name != "random"}
    for a, b in NEGATED:                                   # q and -q on the device: the same rotation
        assert_negation_changes_nothing(got, at[a], at[b], "%s %s %s" % (c["name"], mode, a))
    cI, cQ = cands_of(c, mode, 257)
    again = capi.window_gate(c["I"], c["QQ"], Q, c["f"], cI, cQ, weights=w, sigma=c["sigma"])
    for k in KEYS:                                         # two identical calls: bitwise equal
        assert again[k].tobytes() == alone(c, mode, 257, sigma=c["sigma"])[k].tobytes(), k
    only = capi.window_gate(c["I"], c["QQ"], Q, c["f"], cI[:0], cQ[:0], weights=w, sigma=c["sigma"])   # the scale alone
    assert np.array([only["scale"]]).tobytes() == np.array([got["scale"]]).tobytes() and len(only["chi2"]) == 0


def test_single_problem_failures_leave_the_outputs():
    c = CASES[2]
    Q, w = state(c, "supplied")
    w = w.copy()
    v = c["f"] + 3
    w[(c["I"][:, 0] == v) | (c["I"][:, 1] == v)] = 0.0      # nothing holds view v: singular
    cI, cQ = cands_of(c, "supplied", 9)
    r = capi.window_gate(c["I"], c["QQ"], Q, c["f"], cI, cQ, weights=w, allow_rc=(capi.ERR_SOLVER,))
    assert r["rc"] == capi.ERR_SOLVER and np.isnan(r["scale"])
    for k in KEYS:
        assert np.isnan(r[k]).all(), k                      # (the wrapper presets NaN)


# ---- 2. the batch is bitwise the single-problem call ----------------------------------------------------------------------------
def pack(cases, mode, counts):
    st = [state(c, mode) for c in cases]
    cd = [cands_of(c, mode, n) for c, n in zip(cases, counts)]
    return dict(sizes=np.array([(c["nv"], c["f"], c["ne"]) for c in cases], dtype=np.int32),
                I=np.concatenate([c["I"] for c in cases]).astype(np.int32),
                QQ=np.concatenate([c["QQ"] for c in cases]).astype(np.float64),
                Q=np.concatenate([q for q, _ in st]).astype(np.float64),
                w=None if mode == "poses" else np.concatenate([w for _, w in st]),
                ncand=np.array(counts, dtype=np.int32),
                cI=np.concatenate([a for a, _ in cd]).astype(np.int32).reshape(-1, 2),
                cQ=np.concatenate([b for _, b in cd]).astype(np.float64).reshape(-1, 4))


def offsets(p):
    return np.concatenate([[0], np.cumsum(p["ncand"].astype(np.int64))])


def run(cases, mode, counts, want=(True, True, True), cQ_t=None, ids=torch.int32, allow_rc=()):
    """torch_api.window_gate_batch with every requested output preset to MARK"""
    p = pack(cases, mode, counts)
    nc = len(p["cI"])
    outs = [torch.full((nc,), MARK, dtype=torch.float64, device=dev()) if on else False for on in want]
    Q_t = t64(p["Q"])
    r = torch_api.window_gate_batch(p["sizes"], torch.tensor(p["I"], dtype=torch.int32, device=dev()), t64(p["QQ"]), Q_t,
                                    torch.tensor(p["cI"], dtype=ids, device=dev()), t64(p["cQ"]) if cQ_t is None else cQ_t,
                                    p["ncand"], None if p["w"] is None else t64(p["w"]), SIG, *outs, allow_rc=allow_rc)
    torch.cuda.synchronize()
    assert Q_t.cpu().numpy().tobytes() == p["Q"].tobytes()                  # Q is never written
    r["host"] = {k: None if r[k] is None else r[k].cpu().numpy() for k in KEYS}
    r["packed"] = p
    return r


def assert_bitwise(cases, mode, counts, r):
    off = offsets(r["packed"])
    for b, (c, n) in enumerate(zip(cases, counts)):
        a = alone(c, mode, n)
        assert r["status"][b] == 0, (c["name"], r["status"][b])
        for k in KEYS:
            if r["host"][k] is not None:
                assert r["host"][k][off[b]:off[b + 1]].tobytes() == a[k].tobytes(), (b, c["name"], n, k)
        assert np.array([r["scale"][b]]).tobytes() == np.array([a["scale"]]).tobytes(), c["name"]


def cycle(n, counts=(257, 0, 1, 600, 12)):
    return [counts[b % len(counts)] for b in range(n)]


@pytest.mark.parametrize("mode", MODES)
def test_mixed_batch_is_bitwise_the_single_problem_calls(mode):
    counts = cycle(len(CASES))
    r = run(CASES, mode, counts)
    assert r["rc"] == 0
    assert_bitwise(CASES, mode, counts, r)
    again = run(CASES, mode, counts)                       # two identical batched calls: bitwise equal
    for k in KEYS:
        assert again["host"][k].tobytes() == r["host"][k].tobytes(), k
    assert again["scale"].tobytes() == r["scale"].tobytes()
    rev, rc = CASES[::-1], counts[::-1]
    assert_bitwise(rev, mode, rc, run(rev, mode, rc))      # the same batch reversed
    shifted = counts[1:] + counts[:1]                      # every case with another count (the largest one gets 600)
    assert_bitwise(CASES, mode, shifted, run(CASES, mode, shifted))


@pytest.mark.parametrize("mode", MODES)
def test_more_workgroups_than_compute_units(mode):
    cases = [SMALL3[b % 3] for b in range(600)]
    assert 600 > torch.cuda.get_device_properties(dev()).multi_processor_count
    counts = cycle(600, (0, 1, 257, 600))
    r = run(cases, mode, counts)
    assert r["rc"] == 0 and (r["status"] == 0).all()
    assert_bitwise(cases, mode, counts, r)


def test_each_output_alone_and_the_scale_alone():
    cases, counts = CASES[1:6], [600, 0, 257, 1, 9]
    full = run(cases, "supplied", counts)
    assert_bitwise(cases, "supplied", counts, full)
    for want in ((True, False, False), (False, True, False), (False, False, True), (False, False, False)):
        r = run(cases, "supplied", counts, want=want)
        assert r["rc"] == 0
        for k, on in zip(KEYS, want):
            assert (r[k] is not None) == on
            if on:
                assert r["host"][k].tobytes() == full["host"][k].tobytes(), k
        assert r["scale"].tobytes() == full["scale"].tobytes()
    none = run(cases, "supplied", [0] * len(cases))        # no candidate anywhere: the scale is the answer
    assert none["rc"] == 0 and none["scale"].tobytes() == full["scale"].tobytes() and len(none["host"]["chi2"]) == 0


# ---- 3. chained behind the solve, no host synchronise between them ---------------------------------------------------------------
def test_chained_behind_the_batched_solve_on_one_side_stream():
    cases = [c for c in CASES if "bridges" not in c]
    counts = cycle(len(cases), (12, 257, 0, 30))
    p = pack(cases, "poses", counts)
    ei = torch.tensor(p["I"], dtype=torch.int32, device=dev())
    QQ_t, Q_t, cQ_t = t64(p["QQ"]), t64(p["Q"]), t64(p["cQ"])
    ci = torch.tensor(p["cI"], dtype=torch.int32, device=dev())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        s = torch_api.window_solve_batch(p["sizes"], ei, QQ_t, Q_t, 4, SIG, 100, 100, 1e-3)
        r = torch_api.window_gate_batch(p["sizes"], ei, QQ_t, s["Q"], ci, cQ_t, p["ncand"], s["weights"], SIG)
    side.synchronize()
    assert s["rc"] == 0 and r["rc"] == 0
    Qh, wh = Q_t.cpu().numpy(), s["weights"].cpu().numpy()
    sz = p["sizes"].astype(np.int64)
    eo, vo, co = (np.concatenate([[0], np.cumsum(a)]) for a in (sz[:, 2], sz[:, 0], p["ncand"].astype(np.int64)))
    host = {k: r[k].cpu().numpy() for k in KEYS}
    for b, c in enumerate(cases):
        Q, d = Qh[vo[b]:vo[b + 1]], wh[eo[b]:eo[b + 1]]
        assert consistency(c, d) < 1e-9
        ref = gate_reference(c, d, (p["cI"][co[b]:co[b + 1]], p["cQ"][co[b]:co[b + 1]]), Q)
        for k in KEYS:
            assert_same(host[k][co[b]:co[b + 1]], ref[k], "chain %s %s" % (c["name"], k))
        assert r["scale"][b] == pytest.approx(ref["scale"], rel=1e-9, nan_ok=True)


# ---- 4. layouts of the candidates ---------------------------------------------------------------------------------------------------
FOUR = [CASES[2], CASES[5], CASES[1], CASES[6]]
FOUR_N = [257, 30, 0, 600]


@pytest.fixture(scope="module")
def four():
    r = run(FOUR, "supplied", FOUR_N)
    assert_bitwise(FOUR, "supplied", FOUR_N, r)
    return r


def same_outputs(r, ref):
    for k in KEYS:
        assert r["host"][k].tobytes() == ref["host"][k].tobytes(), k
    assert r["scale"].tobytes() == ref["scale"].tobytes() and (r["status"] == 0).all()


def test_cand_qq_row_major_is_the_16_byte_path(four):
    cQ = t64(four["packed"]["cQ"])
    assert cQ.data_ptr() % 16 == 0 and torch_api.matrix_strides(cQ) == (4, 1)
    same_outputs(run(FOUR, "supplied", FOUR_N, cQ_t=cQ), four)


def test_cand_qq_as_four_planes_with_rows_beyond_the_batch(four):
    cQ = four["packed"]["cQ"]
    N = len(cQ)
    planes = torch.full((4, N + 5), 321.25, dtype=torch.float64, device=dev())
    planes[:, :N] = t64(cQ).t()
    view = planes[:, :N].t()
    assert torch_api.matrix_strides(view) == (1, N + 5)
    same_outputs(run(FOUR, "supplied", FOUR_N, cQ_t=view), four)


def test_cand_qq_as_columns_of_a_wider_tensor(four):
    cQ = four["packed"]["cQ"]
    wide = torch.full((len(cQ), 6), 123.5, dtype=torch.float64, device=dev())
    wide[:, 1:5] = t64(cQ)
    assert torch_api.matrix_strides(wide[:, 1:5]) == (6, 1)
    same_outputs(run(FOUR, "supplied", FOUR_N, cQ_t=wide[:, 1:5]), four)


def test_cand_qq_behind_a_pointer_that_is_8_but_not_16_byte_aligned(four):
    cQ = four["packed"]["cQ"]
    flat = torch.full((4 * len(cQ) + 2,), 9.75, dtype=torch.float64, device=dev())
    view = flat[1:1 + 4 * len(cQ)].view(len(cQ), 4)
    view.copy_(t64(cQ))
    assert view.data_ptr() % 16 == 8 and torch_api.matrix_strides(view) == (4, 1)
    same_outputs(run(FOUR, "supplied", FOUR_N, cQ_t=view), four)


def test_int64_candidate_ids_are_narrowed_on_the_device(four):
    same_outputs(run(FOUR, "supplied", FOUR_N, ids=torch.int64), four)


class Raw:
    """the C call itself on marker-filled outputs"""

    def __init__(self, cases=FOUR, counts=FOUR_N, mode="supplied"):
        self.p = p = pack(cases, mode, counts)
        nc = len(p["cI"])
        self.I = torch.tensor(p["I"], dtype=torch.int32, device=dev())
        self.QQ, self.Q = t64(p["QQ"]), t64(p["Q"])
        self.w = None if p["w"] is None else t64(p["w"])
        self.cI = torch.tensor(p["cI"], dtype=torch.int32, device=dev())
        self.cQ = t64(p["cQ"])
        self.out = {k: torch.full((max(nc, 1),), MARK, dtype=torch.float64, device=dev()) for k in KEYS}
        self.scale = np.full(len(cases), MARK)
        self.res = np.full(len(cases), -99, dtype=np.int32)

    def call(self, nb=None, sizes=None, ncand=None, cI="own", cQ="own", cq_strides=(4, 1), nothing=False, angle="own"):
        p = lambda t: None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())
        own = lambda v, mine: mine if isinstance(v, str) else v
        i32 = C.POINTER(C.c_int32)
        sizes = np.ascontiguousarray(self.p["sizes"] if sizes is None else sizes, dtype=np.int32)
        nc = np.ascontiguousarray(self.p["ncand"] if ncand is None else ncand, dtype=np.int32)
        o = {k: (None if nothing else v) for k, v in self.out.items()}
        rc = capi.lib().irotavg_window_gate_batch_dev(
            len(sizes) if nb is None else nb, sizes.ctypes.data_as(i32), p(self.I), p(self.QQ), 4, 1, p(self.Q), 4, 1,
            p(self.w), SIG, nc.ctypes.data_as(i32), p(own(cI, self.cI)), p(own(cQ, self.cQ)), cq_strides[0], cq_strides[1],
            p(own(angle, o["angle"])), p(o["pair_var"]), p(o["chi2"]),
            None if nothing else self.scale.ctypes.data_as(C.POINTER(C.c_double)), self.res.ctypes.data_as(i32),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert self.Q.cpu().numpy().tobytes() == self.p["Q"].tobytes()      # Q is never written
        return rc

    def host(self):
        return {k: v.cpu().numpy()[:len(self.p["cI"])] for k, v in self.out.items()}

    def untouched(self):
        for k, v in self.out.items():
            assert (v.cpu().numpy() == MARK).all(), k
        assert (self.scale == MARK).all() and (self.res == -99).all()


def test_cand_qq_with_a_negative_row_stride(four):
    """torch has no negative strides: the reversed buffer goes through the raw call, cand_QQ_dev = its last row, rs = -4"""
    R = Raw()
    N = len(R.p["cQ"])
    buf = torch.full((N + 2, 4), 55.5, dtype=torch.float64, device=dev())
    buf[1:N + 1] = t64(R.p["cQ"][::-1])
    before = buf.cpu().numpy().tobytes()
    assert R.call(cQ=buf.data_ptr() + 32 * N, cq_strides=(-4, 1)) == 0
    for k, v in R.host().items():
        assert v.tobytes() == four["host"][k].tobytes(), k
    assert R.scale.tobytes() == four["scale"].tobytes() and (R.res == 0).all()
    assert buf.cpu().numpy().tobytes() == before


# ---- 5. the guard and per-problem failures ------------------------------------------------------------------------------------------
def check_one_failed(R, bad, status, rc):
    """problem `bad` reports `status` and keeps every marker; the other three are bitwise their single-problem results"""
    assert rc == status                                    # the first non-zero status (the only one)
    off = offsets(R.p)
    h = R.host()
    for b, (c, n) in enumerate(zip(FOUR, FOUR_N)):
        if b == bad:
            assert R.res[b] == status and R.scale[b] == MARK
            for k in KEYS:
                assert (h[k][off[b]:off[b + 1]] == MARK).all(), k
            continue
        a = alone(c, "supplied", n)
        assert R.res[b] == 0
        for k in KEYS:
            assert h[k][off[b]:off[b + 1]].tobytes() == a[k].tobytes(), (c["name"], k)
        assert np.array([R.scale[b]]).tobytes() == np.array([a["scale"]]).tobytes()


@pytest.mark.parametrize("bad", [0, 3])
@pytest.mark.parametrize("value", ["nv", -1, "i==j", 2 ** 31 - 1])
def test_a_candidate_id_the_guard_refuses_fails_its_problem_alone(bad, value):
    R = Raw()
    off = offsets(R.p)
    cI = R.p["cI"].copy()
    row = off[bad] + FOUR_N[bad] - 2                       # (problem 3: past the first chunk of 256 and the thread stride)
    if value == "i==j":
        cI[row, 1] = cI[row, 0]
    else:
        cI[row, 1 if value == -1 else 0] = FOUR[bad]["nv"] if value == "nv" else value
    check_one_failed(R, bad, capi.ERR_BAD_ARG, R.call(cI=torch.tensor(cI, dtype=torch.int32, device=dev())))


def singular_weights(R, bad):
    """weight exactly 0 on every edge of one free view of problem `bad`"""
    sz = R.p["sizes"].astype(np.int64)
    eo = np.concatenate([[0], np.cumsum(sz[:, 2])])
    c = FOUR[bad]
    v = c["f"] + 5
    w = R.p["w"].copy()
    hit = (c["I"][:, 0] == v) | (c["I"][:, 1] == v)
    assert hit.any()
    w[eo[bad]:eo[bad + 1]][hit] = 0.0
    return w


def test_a_singular_problem_reports_it_and_keeps_its_rows():
    R = Raw()
    R.w = t64(singular_weights(R, 3))
    check_one_failed(R, 3, capi.ERR_SOLVER, R.call())


def test_the_first_failure_in_problem_order_is_returned():
    R = Raw()
    off = offsets(R.p)
    cI = R.p["cI"].copy()
    cI[off[3] + 300, 0] = -1                               # problem 3: a bad candidate id; problem 1: singular
    R.w = t64(singular_weights(R, 1))
    assert R.call(cI=torch.tensor(cI, dtype=torch.int32, device=dev())) == capi.ERR_SOLVER
    assert list(R.res) == [0, capi.ERR_SOLVER, 0, capi.ERR_BAD_ARG]
    R = Raw()
    cI[off[0] + 5] = (2, 2)                                # and now problem 0 first
    R.w = t64(singular_weights(R, 1))
    assert R.call(cI=torch.tensor(cI, dtype=torch.int32, device=dev())) == capi.ERR_BAD_ARG
    assert list(R.res) == [capi.ERR_BAD_ARG, capi.ERR_SOLVER, 0, capi.ERR_BAD_ARG]


def test_whole_call_refusals_leave_every_marker():
    R = Raw()
    N = len(R.p["cI"])
    host_q, host_i = np.zeros((N, 4)), np.zeros((N, 2), dtype=np.int32)
    calls = [
        ("nb = 0", dict(nb=0)),
        ("nothing asked for", dict(nothing=True)),
        ("candidates without their ids", dict(cI=None)),
        ("candidates without their measurements", dict(cQ=None)),
        ("a negative count", dict(ncand=[1, -1, 2, 3])),
        ("host cand_QQ", dict(cQ=host_q.ctypes.data)),
        ("host cand_I", dict(cI=host_i.ctypes.data)),
        ("host output", dict(angle=host_q.ctypes.data)),
        ("aliasing cand_QQ strides", dict(cq_strides=(2, 1))),
        ("cand_QQ too short for its strides", dict(cq_strides=(1, 2 ** 31))),
        ("misaligned cand_I", dict(cI=R.cI.data_ptr() + 4)),
        ("more candidates than the arrays hold", dict(ncand=[1, 2, 3, 2 ** 30])),
    ]
    for what, kw in calls:
        assert R.call(**kw) == capi.ERR_BAD_ARG, what
        R.untouched()
    assert R.call() == 0                                   # the same arguments without the fault
    assert (R.res == 0).all() and not (R.scale == MARK).any()


# ---- 6. the planted closures ---------------------------------------------------------------------------------------------------------
def test_the_gate_ranks_planted_wrong_closures_above_every_true_one():
    c, cI, cQ = planted_closures()
    g = capi.window_gate(c["I"], c["QQ"], c["Q0"], c["f"], cI, cQ)
    r = torch_api.window_gate_batch(np.array([(c["nv"], c["f"], c["ne"])]), torch.tensor(c["I"], dtype=torch.int32, device=dev()),
                                    t64(c["QQ"]), t64(c["Q0"]), torch.tensor(cI, dtype=torch.int32, device=dev()), t64(cQ),
                                    [len(cI)])
    torch.cuda.synchronize()
    for chi in (g["chi2"], r["chi2"].cpu().numpy()):
        print("true max %.3f, wrong min %.3f" % (chi[:GATE_TRUE].max(), chi[GATE_TRUE:].min()))
        assert np.all(np.isfinite(chi))
        assert chi[GATE_TRUE:].min() > chi[:GATE_TRUE].max()
    assert r["chi2"].cpu().numpy().tobytes() == g["chi2"].tobytes()


# ---- 7. the view-graph route gives the same bits ---------------------------------------------------------------------------------------
def test_the_viewgraph_gate_on_the_window_route_is_bitwise_the_single_call():
    n, win = 40, 10
    vg, vo, _ = make_pair(n, 7, (0,))
    P = extract_problem(vo, win)                            # the problem's structure: edge order and view numbering
    assert P["skipped"] == 0
    v2i = P["v2i"]
    views = sorted(v2i)
    # the arrays as the library forms them: its own rmat2quat of the poses and of the connections as they were given
    Q = np.array([viewgraph.rmat2quat(vg.R(P["i2v"][r])) for r in range(P["nv"])])
    QQ = np.array([viewgraph.rmat2quat(vo.conn[j][i]) for i, j in P["conn"]])
    rng = np.random.default_rng(11)
    rotations = candidate_set(CASES[2], count=MOST)[1]      # any rotations will do: near 0, near pi, w < 0
    cands = []
    for t in range(300):                                    # more than one launch stages, both orders
        a, b = (int(x) for x in rng.choice(views, size=2, replace=False))
        cands.append((a, b, viewgraph.quat2rmat(np.array(rotations[t]))))
    g = vg.gateConnections(win, [c[:2] for c in cands], [c[2] for c in cands])
    assert g["route"] == 1 and g["skipped"] == 0 and (g["n_views"], g["n_edges"], g["n_fixed"]) == (P["nv"], P["ne"], P["f"])
    cI = np.array([(v2i[min(a, b)], v2i[max(a, b)]) for a, b, _ in cands], dtype=np.int32)
    cQ = np.array([viewgraph.rmat2quat(R if a < b else R.T) for a, b, R in cands])
    w = capi.window_gate(P["I"], QQ, Q, P["f"], cI, cQ, weights=None, sigma=5 * np.pi / 180)
    for k in KEYS:
        assert w[k].tobytes() == g[k][:len(cands)].tobytes(), k
    assert np.array([w["scale"]]).tobytes() == np.array([g["scale"]]).tobytes()
