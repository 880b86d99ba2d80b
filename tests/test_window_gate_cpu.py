"""irotavg_window_gate / irotavg_window_gate_batch_dev (docs/window_gate_batch.md) without a GPU: the candidate set and the
NumPy reference the GPU test (test_gpu_window_gate_batch.py) uses, checked here for their properties; the planted-closure
input; the symbols; every refusal that comes before a device is needed; the torch front-end's own checks; the candidate
offsets.

The reference is built from what the repository has: `reference` / `residuals` of test_window_uncertainty_cpu.py (the
scale, K1's residual through oracle.np_twin), dense_reference (test_rotation_variance_cpu.py) for pair_var, and the
candidate formula of viewgraph_uncertainty_reference: chi2 = |r|^2 / (s^2 (pair_var + sigma^4))."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import window_cases as WC  # noqa: E402
from irotavg_amd import capi, synth  # noqa: E402
from oracle import np_twin as T  # noqa: E402
from test_rotation_variance_cpu import dense_reference  # noqa: E402
from test_window_uncertainty_cpu import (CASES, GOOD, SIG, SMALL3, named, pose_weights, reference,  # noqa: E402
                                         solved_weights_twin)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE, BATCH = "irotavg_window_gate", "irotavg_window_gate_batch_dev"
IDENT = np.array([0.0, 0.0, 0.0, 1.0])


# ---- the candidates ------------------------------------------------------------------------------------------------------------
def measured(Q, i, j, off):
    """the measurement of (i, j) that is `off` (a rotation vector) away from the poses: off = 0 has a zero residual"""
    return synth.qmul(synth.qexp(np.asarray(off, dtype=np.float64)[None])[0], synth.qmul(Q[j], synth.qconj(Q[i])))


def unit(rng):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


def candidate_set(c, Q=None, count=None, seed=0):
    """(cand_I (nc, 2) int32, cand_QQ (nc, 4), names) for problem c at the poses Q (default Q0): free-free (where the
    problem has two free views), free-fixed, fixed-free, fixed-fixed (where f >= 2), a duplicate of an existing edge, a
    measurement consistent with the poses to 0.01 rad, one off by 0.3-0.6 rad, one within 0.05 rad of pi, the last two
    again with the quaternion negated (w < 0), on bridge0 the identity between two identity poses. count: cut or padded
    with random pairs and rotations of up to 0.5 rad to exactly that many."""
    Q = np.asarray(c["Q0"] if Q is None else Q, dtype=np.float64)
    nv, f, nu = c["nv"], c["f"], c["nv"] - c["f"]
    rng = np.random.default_rng([seed, nv, c["ne"]])
    P, names = [], []

    def add(name, i, j, qq):
        names.append(name)
        P.append((int(i), int(j), np.asarray(qq, dtype=np.float64)))
    if nu >= 2:
        add("free-free", f, nv - 1, measured(Q, f, nv - 1, 0.02 * unit(rng)))
    add("free-fixed", nv - 1, 0, measured(Q, nv - 1, 0, 0.02 * unit(rng)))
    add("fixed-free", 0, f, measured(Q, 0, f, 0.02 * unit(rng)))
    if f >= 2:
        add("fixed-fixed", 0, f - 1, measured(Q, 0, f - 1, 0.02 * unit(rng)))
    k = int(np.flatnonzero(c["I"][:, 0] != c["I"][:, 1])[0])
    add("duplicate", c["I"][k, 0], c["I"][k, 1], c["QQ"][k])
    a, b = (f, nv - 1) if nu >= 2 else (0, nv - 1)
    near = measured(Q, a, b, 0.01 * unit(rng))
    add("consistent", a, b, near)
    add("off", b, a, measured(Q, b, a, (0.3 + 0.3 * rng.random()) * unit(rng)))
    at_pi = measured(Q, a, b, (np.pi - 0.03) * unit(rng))
    add("near-pi", a, b, at_pi)
    add("near-pi-negated", a, b, -at_pi)
    add("consistent-negated", a, b, -near)
    if c["name"] == "bridge0":
        assert (Q[0] == IDENT).all() and (Q[nv - 1] == IDENT).all()
        add("identity", 0, nv - 1, IDENT)
    while count is not None and len(P) < count:
        i, j = rng.choice(nv, size=2, replace=False)
        add("random", i, j, measured(Q, i, j, 0.5 * rng.random() * unit(rng)))
    if count is not None:
        P, names = P[:count], names[:count]
    cI = np.array([(i, j) for i, j, _ in P], dtype=np.int32).reshape(-1, 2)
    cQ = np.array([q for _, _, q in P], dtype=np.float64).reshape(-1, 4)
    return cI, cQ, names


# ---- the reference -------------------------------------------------------------------------------------------------------------
def gate_reference(c, d, cands, Q=None):
    """dict(angle, pair_var, chi2, scale) of the candidates (cand_I, cand_QQ[, names]) of problem c at weights d (and
    rotations Q, default Q0)"""
    cI, cQ = np.asarray(cands[0], dtype=np.int32).reshape(-1, 2), np.asarray(cands[1], dtype=np.float64).reshape(-1, 4)
    Qp = np.asarray(c["Q0"] if Q is None else Q, dtype=np.float64)
    r = T.log_map(T.delta_rel(cI, cQ, Qp))[:, :3] if len(cI) else np.zeros((0, 3))
    ang = np.sqrt(np.sum(r ** 2, axis=1))
    pv = dense_reference(c["I"], c["nv"], c["f"], d, [tuple(p) for p in cI])[1].reshape(-1)
    s2 = reference(c, d, (), Q)["scale"]
    with np.errstate(divide="ignore", invalid="ignore"):
        chi = ang ** 2 / (s2 * (pv + c["sigma"] ** 4))
    return dict(angle=ang, pair_var=pv, chi2=chi, scale=s2)


NEGATED = (("near-pi", "near-pi-negated"), ("consistent", "consistent-negated"))
NEG_ANGLE = 8 * np.finfo(float).eps * 2 * np.pi   # absolute, rad


def assert_negation_changes_nothing(r, a, b, what):
    """Candidates a and b of the answers r differ in the sign of the quaternion alone: the same rotation. pair_var does not
    see the measurement: bitwise equal. The residual's angle is 2 atan2(s, w) for one and 2 atan2(s, -w) - 2 pi for the
    other (log_map's wrap; edge_log's on the device), equal in exact arithmetic and a few roundings of a number near 2 pi
    apart in fp64: at most NEG_ANGLE = 8 eps 2 pi, ABSOLUTE. Everything behind the angle is the same function of it, so
    chi2 = angle^2 / (...) moves by at most 2 NEG_ANGLE / angle, relative (plus its own roundings)."""
    pv, ang, chi = (np.asarray(r[k]) for k in ("pair_var", "angle", "chi2"))
    d = abs(ang[a] - ang[b])
    print("%s: q against -q: |angle difference| %.3e (bound %.3e), chi2 %r %r" % (what, d, NEG_ANGLE, chi[a], chi[b]))
    assert pv[[a]].tobytes() == pv[[b]].tobytes(), what
    assert d <= NEG_ANGLE, what
    if np.isnan(chi[a]) or np.isnan(chi[b]):
        assert np.isnan(chi[a]) and np.isnan(chi[b]), what
    else:
        assert abs(chi[a] - chi[b]) <= (2 * NEG_ANGLE / ang[a] + 8 * np.finfo(float).eps) * chi[a], what


def modes_of(c):
    out = [("poses", pose_weights(c), None)]
    if c["name"] != "bridge0" and c["nu"] > 1:
        Q, w = solved_weights_twin(c)
        out.append(("solved", w, Q))
    return out


@pytest.mark.parametrize("c", CASES + SMALL3, ids=lambda c: c["name"])
def test_the_candidate_set_and_the_reference_have_the_properties(c):
    nv, f = c["nv"], c["f"]
    for mode, d, Q in modes_of(c):
        cI, cQ, names = candidate_set(c, Q)
        at = {n: k for k, n in enumerate(names)}
        r = gate_reference(c, d, (cI, cQ), Q)
        print("%s %s: %d candidates, angle %.3g .. %.3g, chi2 %.3g .. %.3g" % (
            c["name"], mode, len(cI), r["angle"].min(), r["angle"].max(), np.nanmin(r["chi2"]) if np.isfinite(r["chi2"]).any() else np.nan,
            np.nanmax(r["chi2"]) if np.isfinite(r["chi2"]).any() else np.nan))
        # the set holds what it is meant to hold
        assert ((cI >= 0) & (cI < nv)).all() and (cI[:, 0] != cI[:, 1]).all()
        assert {"free-fixed", "fixed-free", "duplicate", "consistent", "off", "near-pi", "near-pi-negated"} <= set(names)
        assert ("free-free" in at) == (c["nu"] >= 2) and ("fixed-fixed" in at) == (f >= 2)
        i, j = cI[at["free-fixed"]]
        assert i >= f > j
        i, j = cI[at["fixed-free"]]
        assert i < f <= j
        k = at["duplicate"]
        assert (c["I"] == cI[k]).all(axis=1).any() and (cQ[k] == c["QQ"][(c["I"] == cI[k]).all(axis=1)][0]).all()
        assert r["angle"][at["consistent"]] == pytest.approx(0.01, rel=1e-6)
        assert 0.3 <= r["angle"][at["off"]] <= 0.6
        assert np.pi - 0.05 < r["angle"][at["near-pi"]] < np.pi
        assert cQ[at["near-pi-negated"]][3] < 0 or cQ[at["near-pi"]][3] < 0
        assert cQ[at["consistent-negated"]][3] < 0 or cQ[at["consistent"]][3] < 0
        # the properties of the answers
        assert np.isfinite(r["angle"]).all() and np.isfinite(r["pair_var"]).all() and (r["pair_var"] >= 0).all()
        if "fixed-fixed" in at:
            assert r["pair_var"][at["fixed-fixed"]] == 0.0
        # q and -q are the same rotation
        for a, b in NEGATED:
            assert_negation_changes_nothing(r, at[a], at[b], "%s %s %s" % (c["name"], mode, a))
        if np.isnan(r["scale"]):
            assert (c["nu"], c["ne"]) == (1, 1) and np.isnan(r["chi2"]).all()
        else:
            assert np.isfinite(r["chi2"]).all() and (r["chi2"] >= 0).all()
        if "identity" in at:
            assert r["angle"][at["identity"]] == 0.0 and r["chi2"][at["identity"]] == 0.0


def test_the_cases_the_issue_names_are_covered():
    one = [c for c in CASES if (c["nu"], c["nv"], c["ne"]) == (1, 2, 1)][0]
    r = gate_reference(one, pose_weights(one), candidate_set(one))
    assert np.isnan(r["scale"]) and np.isnan(r["chi2"]).all() and np.isfinite(r["angle"]).all() and np.isfinite(r["pair_var"]).all()
    b0 = [c for c in CASES if c["name"] == "bridge0"][0]
    assert "identity" in candidate_set(b0)[2]
    for n in (1, 255, 256, 257, 600):
        cI, cQ, names = candidate_set(CASES[2], count=n)
        assert len(cI) == len(cQ) == len(names) == n
    assert candidate_set(CASES[2], count=600)[2][:10] == candidate_set(CASES[2])[2][:10]   # padding keeps the named ones


# ---- the planted-closure input ---------------------------------------------------------------------------------------------------
GATE_NV, GATE_TRUE, GATE_WRONG, GATE_SEED = 61, 20, 5, 1
GATE_GAP, GATE_CHI2 = 10.0, 11.34    # wrong / true ratio the reference must show; the 99 % point of chi-square with 3 d.o.f.


def planted_closures(seed=GATE_SEED):
    """A window-size graph (one fixed view, 60 free ones, each linked to up to 4 predecessors, 0.01 rad of measurement
    noise) at its ground-truth poses perturbed by 0.01 rad (a stand-in for a converged solve that needs no GPU), with
    GATE_TRUE candidate closures between views at least 20 apart that agree with ground truth (same noise) and GATE_WRONG
    that are 0.3-0.6 rad off. Returns (case, cand_I, cand_QQ); the first GATE_TRUE candidates are the true ones."""
    rng = np.random.default_rng([seed, 77])
    nv = GATE_NV
    Qgt = rng.normal(size=(nv, 4))
    Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    I = np.array([(j - k, j) for j in range(1, nv) for k in range(1, 5) if j - k >= 0], dtype=np.int32)
    QQ = synth.qmul(synth.qexp(rng.normal(scale=0.01 / np.sqrt(3), size=(len(I), 3))), synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]])))
    Q0 = synth.qmul(synth.qexp(rng.normal(scale=0.01 / np.sqrt(3), size=(nv, 3))), Qgt)
    Q0[0] = Qgt[0]
    c = named("planted-closures", dict(I=I, QQ=QQ, Q0=Q0, f=1, nv=nv))
    cI, cQ = [], []
    for t in range(GATE_TRUE + GATE_WRONG):
        a = int(rng.integers(0, nv - 20))
        b = int(rng.integers(a + 20, nv))
        off = rng.normal(scale=0.01 / np.sqrt(3), size=3)
        if t >= GATE_TRUE:
            off = (0.3 + 0.3 * rng.random()) * unit(rng)
        if t % 2:                                                    # both orientations
            a, b = b, a
        cI.append((a, b))
        cQ.append(measured(Qgt, a, b, off))
    return c, np.array(cI, dtype=np.int32), np.array(cQ)


def test_the_planted_closures_are_separated_in_the_reference():
    c, cI, cQ = planted_closures()
    assert c["nu"] <= 64 and c["ne"] <= 640 and len(cI) == GATE_TRUE + GATE_WRONG
    r = gate_reference(c, pose_weights(c), (cI, cQ))
    chi = r["chi2"]
    true_max, wrong_min = chi[:GATE_TRUE].max(), chi[GATE_TRUE:].min()
    print("planted closures: true max %.3f, wrong min %.1f, ratio %.1f, wrong angles %.3f .. %.3f" % (
        true_max, wrong_min, wrong_min / true_max, r["angle"][GATE_TRUE:].min(), r["angle"][GATE_TRUE:].max()))
    assert np.isfinite(chi).all()
    assert (r["angle"][GATE_TRUE:] > 0.25).all() and (r["angle"][GATE_TRUE:] < 0.65).all()
    assert wrong_min >= GATE_GAP * true_max
    assert true_max < GATE_CHI2


# ---- the symbols -----------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    for name in (SINGLE, BATCH):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name) and getattr(capi.lib(), name).argtypes is not None
    assert callable(capi.window_gate)
    from irotavg_amd import torch_api
    assert callable(torch_api.window_gate_batch)


# ---- irotavg_window_gate: refusals before a device ---------------------------------------------------------------------------------
MARK = -7.0
CI, CQ, _ = candidate_set(GOOD)


def single(c=GOOD, weights=True, cI=CI, cQ=CQ, ncand=None, ids=True, meas=True, angle=True, pv=True, chi=True, scale=True,
           f=None, I=None, ldcq=None):
    """the raw call on marker-filled outputs: (rc, outputs); nothing may be written by a refused call"""
    I = capi.edges(c["I"] if I is None else I)
    QQ, Q = capi.fmat(c["QQ"]), capi.fmat(c["Q0"])
    m, n = len(I), Q.shape[0]
    w = np.ones(m)
    cI = np.ascontiguousarray(cI, dtype=np.int32).reshape(-1, 2)
    cQf = capi.fmat(np.asarray(cQ, dtype=np.float64).reshape(-1, 4))
    nc = len(cI)
    out = dict(angle=np.full(max(nc, 1), MARK), pair_var=np.full(max(nc, 1), MARK), chi2=np.full(max(nc, 1), MARK))
    s = C.c_double(MARK)
    dp, ip = capi._d, capi._i
    rc = capi.lib().irotavg_window_gate(
        m, n, c["f"] if f is None else f, ip(I), dp(QQ), max(m, 1), dp(Q), n, dp(w) if weights else None, SIG,
        nc if ncand is None else ncand, ip(cI) if ids and nc else None, dp(cQf) if meas and nc else None,
        max(nc, 1) if ldcq is None else ldcq, dp(out["angle"]) if angle else None, dp(out["pair_var"]) if pv else None,
        dp(out["chi2"]) if chi else None, C.byref(s) if scale else None)
    out["scale"] = np.array([s.value])
    return rc, out


def untouched(out):
    return all((a == MARK).all() for a in out.values())


@pytest.mark.parametrize("name,kernel,c", [p for p in WC.past_limits() if p[1] == 0], ids=lambda p: str(p))
def test_single_refuses_what_window_fits_refuses(name, kernel, c):
    c = named(name, c)
    rc, out = single(c, cI=[(0, 1)], cQ=[IDENT])
    assert rc == capi.ERR_BAD_ARG and untouched(out)


def test_single_refuses_bad_ids_counts_and_an_empty_request():
    nv = GOOD["nv"]
    for bad in (-1, nv, 2 ** 31 - 1):
        for col in (0, 1):
            I = GOOD["I"].copy()
            I[3, col] = bad
            rc, out = single(I=I)
            assert rc == capi.ERR_BAD_ARG and untouched(out)
            cI = CI.copy()
            cI[len(cI) // 2, col] = bad
            rc, out = single(cI=cI)
            assert rc == capi.ERR_BAD_ARG and untouched(out)
    for v in (0, GOOD["f"], nv - 1):                                         # i == j: fixed or free
        cI = CI.copy()
        cI[-1] = (v, v)
        rc, out = single(cI=cI)
        assert rc == capi.ERR_BAD_ARG and untouched(out)
    for f in (-1, nv, nv + 5):
        rc, out = single(f=f)
        assert rc == capi.ERR_BAD_ARG and untouched(out)
    rc, out = single(ncand=-1)
    assert rc == capi.ERR_BAD_ARG and untouched(out)
    rc, out = single(ids=False)                                              # a count without the ids
    assert rc == capi.ERR_BAD_ARG and untouched(out)
    rc, out = single(meas=False)                                             # ... without the measurements
    assert rc == capi.ERR_BAD_ARG and untouched(out)
    rc, out = single(ldcq=len(CI) - 1)                                       # a leading dimension below the count
    assert rc == capi.ERR_BAD_ARG and untouched(out)
    rc, out = single(angle=False, pv=False, chi=False, scale=False)          # no output pointer at all
    assert rc == capi.ERR_BAD_ARG and untouched(out)
    rc, out = single(cI=[], cQ=[], scale=False)                              # no candidates and no scale
    assert rc == capi.ERR_BAD_ARG and untouched(out)
    L = capi.lib()
    assert L.irotavg_window_gate(1, 2, 1, None, None, 1, None, 2, None, SIG, 0, None, None, 1, None, None, None,
                                 None) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [dict(), dict(weights=False), dict(angle=False, pv=False), dict(cI=[], cQ=[]),
                                dict(angle=False, pv=False, chi=False), dict(scale=False, chi=False)], ids=str)
def test_a_well_formed_single_call_needs_a_device(kw):
    if capi.lib().irotavg_device_count() > 0:
        pytest.skip("a HIP device exists")
    rc, out = single(**kw)
    assert rc == capi.ERR_NO_DEVICE and untouched(out)
    with pytest.raises(capi.IrotavgError) as e:
        capi.window_gate(GOOD["I"], GOOD["QQ"], GOOD["Q0"], GOOD["f"], CI, CQ)
    assert e.value.code == capi.ERR_NO_DEVICE


def test_the_single_wrapper_checks_its_arrays():
    with pytest.raises(ValueError, match="weights"):
        capi.window_gate(GOOD["I"], GOOD["QQ"], GOOD["Q0"], GOOD["f"], CI, CQ, weights=np.ones(3))
    with pytest.raises(ValueError, match="cand_QQ"):
        capi.window_gate(GOOD["I"], GOOD["QQ"], GOOD["Q0"], GOOD["f"], CI, CQ[:-1])


# ---- irotavg_window_gate_batch_dev: refusals before a device ------------------------------------------------------------------------
# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE = {k: C.c_void_p(0x10000 * (i + 1)) for i, k in enumerate(("I", "QQ", "Q", "w", "cI", "cQ", "ang", "pv", "chi"))}
SIZES = [(12, 2, 40), (320, 256, 640), (2, 1, 1)]
NCAND = [3, 0, 600]


def batch(sizes=SIZES, nb=None, qq=(4, 1), q=(4, 1), cq=(4, 1), ncand=NCAND, null_sizes=False, scale=True, results=True, **ptr):
    s = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 3)
    p = dict(FAKE)
    p.update(ptr)
    nc = None if ncand is None else np.ascontiguousarray(ncand, dtype=np.int32)
    sc = np.full(max(len(s), 1), MARK)
    res = np.full(max(len(s), 1), -99, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    rc = capi.lib().irotavg_window_gate_batch_dev(
        len(s) if nb is None else nb, None if null_sizes else s.ctypes.data_as(i32), p["I"], p["QQ"], qq[0], qq[1], p["Q"],
        q[0], q[1], p["w"], SIG, None if nc is None else nc.ctypes.data_as(i32), p["cI"], p["cQ"], cq[0], cq[1], p["ang"],
        p["pv"], p["chi"], sc.ctypes.data_as(C.POINTER(C.c_double)) if scale else None,
        res.ctypes.data_as(i32) if results else None, None)
    assert (res == -99).all() and (sc == MARK).all()
    return rc


@pytest.mark.parametrize("bad", [(66, 1, 100), (321, 300, 100), (70, 6, 641), (20, 20, 30), (20, 1, 0), (20, -1, 30),
                                 (0, 0, 5), (-3, 0, 5), (20, 21, 30), (2 ** 31 - 1, 2 ** 31 - 2, 5), (5, 1, -2)])
def test_batch_refuses_a_problem_outside_the_limits(bad):
    assert batch(SIZES[:2] + [bad] + SIZES[2:], ncand=[3, 0, 1, 600]) == capi.ERR_BAD_ARG


def test_batch_refuses_counts_pointers_candidates_and_an_empty_request():
    assert batch(nb=0) == capi.ERR_BAD_ARG
    assert batch(nb=-1) == capi.ERR_BAD_ARG
    assert batch(nb=262145) == capi.ERR_BAD_ARG
    assert batch(null_sizes=True) == capi.ERR_BAD_ARG
    for k in ("I", "QQ", "Q"):
        assert batch(**{k: None}) == capi.ERR_BAD_ARG
    for k in FAKE:                                                           # not 8-byte aligned
        assert batch(**{k: C.c_void_p(FAKE[k].value + 4)}) == capi.ERR_BAD_ARG, k
    assert batch(ncand=[3, -1, 600]) == capi.ERR_BAD_ARG                     # a negative count
    assert batch(ncand=[3, 0, -2 ** 31]) == capi.ERR_BAD_ARG
    assert batch(cI=None) == capi.ERR_BAD_ARG                                # candidates counted without their arrays
    assert batch(cQ=None) == capi.ERR_BAD_ARG
    nothing = dict(ang=None, pv=None, chi=None)
    assert batch(scale=False, **nothing) == capi.ERR_BAD_ARG                 # no output pointer at all
    assert batch(scale=False, results=False, **nothing) == capi.ERR_BAD_ARG
    assert batch(ncand=[0, 0, 0], scale=False) == capi.ERR_BAD_ARG           # no candidates and no scale
    assert batch(ncand=None, scale=False) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("rs,cs", [(0, 0), (0, 1), (4, 0), (1, 1), (2, 1), (3, 1), (1, 2), (1, 99), (-2, 1), (2, 3),
                                   (2 ** 40, 1), (-2 ** 63, 1), (1, -2 ** 63)])
def test_batch_refuses_strides_that_alias(rs, cs):
    assert batch(qq=(rs, cs)) == capi.ERR_BAD_ARG
    assert batch(q=(rs, cs)) == capi.ERR_BAD_ARG
    assert batch(cq=(rs, cs)) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("rs,cs", [(4, 1), (1, 681), (6, 1), (-4, 1), (1, -700), (4, -1), (2 ** 31, 1)])
def test_a_well_formed_batch_call_needs_a_device(rs, cs):
    if capi.lib().irotavg_device_count() > 0:
        pytest.skip("a HIP device exists")
    assert batch(qq=(rs, cs), q=(rs, cs), cq=(rs, cs)) == capi.ERR_NO_DEVICE
    assert batch(qq=(rs, cs), w=None, ncand=[2 ** 30, 0, 2 ** 30]) == capi.ERR_NO_DEVICE   # a sum past int32
    assert batch(cq=(rs, cs), ang=None, pv=None) == capi.ERR_NO_DEVICE
    assert batch(cq=(rs, cs), ang=None, pv=None, chi=None) == capi.ERR_NO_DEVICE                   # the scale alone
    assert batch(ncand=[0, 0, 0], cI=None, cQ=None, cq=(0, 0)) == capi.ERR_NO_DEVICE               # ... without candidates
    assert batch(ncand=None, cI=None, cQ=None, ang=None, pv=None, chi=None) == capi.ERR_NO_DEVICE
    assert batch(scale=False, results=False, chi=None, pv=None) == capi.ERR_NO_DEVICE              # one output is a request


# ---- the torch front-end ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_c_calls(monkeypatch):
    """Any use of the C library from here on is an error."""
    from irotavg_amd import torch_api

    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    return torch_api


def tensors(m=41, n=14, nc=5):
    return (torch.zeros((m, 2), dtype=torch.int32), torch.zeros((m, 4), dtype=torch.float64),
            torch.zeros((n, 4), dtype=torch.float64), torch.zeros((nc, 2), dtype=torch.int32),
            torch.zeros((nc, 4), dtype=torch.float64))


TSIZES = np.array([(12, 2, 40), (2, 1, 1)])
TNC = [2, 3]


def test_wrapper_rejects_cpu_tensors_before_the_c_call(no_c_calls):
    ei, QQ, Q, ci, cq = tensors()
    with pytest.raises(TypeError, match="ROCm device"):
        no_c_calls.window_gate_batch(TSIZES, ei, QQ, Q, ci, cq, TNC)
    with pytest.raises(TypeError):
        no_c_calls.window_gate_batch(TSIZES, ei, QQ, Q, ci.numpy(), cq, TNC)
    with pytest.raises(TypeError):
        no_c_calls.window_gate_batch(TSIZES, ei, QQ, Q, ci, cq.numpy(), TNC)


def test_wrapper_rejects_wrong_dtypes_before_the_c_call(no_c_calls):
    ei, QQ, Q, ci, cq = tensors()
    f = no_c_calls.window_gate_batch
    with pytest.raises(TypeError, match="float64"):
        f(TSIZES, ei, QQ.float(), Q, ci, cq, TNC)
    with pytest.raises(TypeError, match="float64"):
        f(TSIZES, ei, QQ, Q.float(), ci, cq, TNC)
    with pytest.raises(TypeError, match="float64"):
        f(TSIZES, ei, QQ, Q, ci, cq.float(), TNC)
    with pytest.raises(TypeError, match="int32"):
        f(TSIZES, ei.to(torch.int16), QQ, Q, ci, cq, TNC)
    with pytest.raises(TypeError, match="int32"):
        f(TSIZES, ei, QQ, Q, ci.to(torch.float64), cq, TNC)
    with pytest.raises(TypeError, match="integers"):
        f(TSIZES.astype(np.float64), ei, QQ, Q, ci, cq, TNC)
    with pytest.raises(TypeError, match="ncand must be integers"):
        f(TSIZES, ei, QQ, Q, ci, cq, np.array([2.0, 3.0]))


def test_wrapper_rejects_wrong_shapes_before_the_c_call(no_c_calls):
    ei, QQ, Q, ci, cq = tensors()
    f = no_c_calls.window_gate_batch
    with pytest.raises(ValueError, match="sizes"):
        f(TSIZES.ravel(), ei, QQ, Q, ci, cq, TNC)
    with pytest.raises(ValueError, match="edge_index"):
        f(TSIZES, ei[:-1], QQ, Q, ci, cq, TNC)
    with pytest.raises(ValueError, match="QQ"):
        f(TSIZES, ei, QQ[:, :3], Q, ci, cq, TNC)
    with pytest.raises(ValueError, match="Q must"):
        f(TSIZES, ei, QQ, Q[:-1], ci, cq, TNC)
    with pytest.raises(ValueError, match="ncand"):
        f(TSIZES, ei, QQ, Q, ci, cq, None)
    with pytest.raises(ValueError, match="ncand"):
        f(TSIZES, ei, QQ, Q, ci, cq, [1, 2, 2])                              # one count per problem
    with pytest.raises(ValueError, match="ncand"):
        f(TSIZES, ei, QQ, Q, ci, cq, [6, -1])
    with pytest.raises(ValueError, match="cand_index"):
        f(TSIZES, ei, QQ, Q, ci, cq, [2, 2])                                 # sum ncand differs
    with pytest.raises(ValueError, match="cand_index"):
        f(TSIZES, ei, QQ, Q, ci.reshape(2, 5), cq, TNC)
    with pytest.raises(ValueError, match="cand_QQ"):
        f(TSIZES, ei, QQ, Q, ci, cq[:-1], TNC)
    with pytest.raises(ValueError, match="cand_QQ"):
        f(TSIZES, ei, QQ, Q, ci, cq[:, :3], TNC)


def test_candidate_offsets_are_the_cumulative_sums():
    from irotavg_amd import torch_api
    rng = np.random.default_rng(16)
    c = rng.integers(0, 700, size=900)
    c[::5] = 0
    c32, off, total = torch_api.pair_offsets(c, 900)
    assert c32.dtype == np.int32 and c32.flags.c_contiguous and (c32 == c).all()
    np.testing.assert_array_equal(off, np.cumsum(c) - c)
    assert total == c.sum() and off[0] == 0 and off.dtype == np.int64
    big = np.full(262144, 2 ** 31 - 1, dtype=np.int64)                      # sums that do not fit int32
    _, off, total = torch_api.pair_offsets(big, 262144)
    assert total == 262144 * (2 ** 31 - 1) and off[-1] == 262143 * (2 ** 31 - 1)
