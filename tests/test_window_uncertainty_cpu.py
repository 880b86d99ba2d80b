"""irotavg_window_uncertainty / irotavg_window_uncertainty_batch_dev (docs/window_uncertainty_batch.md) without a GPU: the
cases and the NumPy reference the GPU test (test_gpu_window_uncertainty_batch.py) uses, checked here for being
trustworthy; the symbols; every refusal that comes before a device is needed; the torch front-end's own checks; the pair
offsets.

The reference is the project's own: dense_reference / scale_reference (test_rotation_variance_cpu.py), edge_reference
(test_edge_diagnostics_cpu.py), residuals from oracle.np_twin. A case is used only where max |M Sigma - I| < 1e-9 in that
reference and no informative edge other than a planted bridge has a leverage within 1e-6 of 1 (there the class of chi2,
finite or +inf, would hang on the last bit of 1 - leverage)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import window_cases as WC  # noqa: E402
from irotavg_amd import capi, synth  # noqa: E402
from oracle import np_twin as T  # noqa: E402
from test_edge_diagnostics_cpu import edge_reference, quirk_graph  # noqa: E402
from test_rotation_variance_cpu import dense_reference, edge_terms, scale_reference  # noqa: E402

SIG = WC.SIG
SINGLE, BATCH = "irotavg_window_uncertainty", "irotavg_window_uncertainty_batch_dev"


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def named(name, c, sigma=SIG, **kw):
    c = dict(c)
    c.update(name=name, ne=len(c["I"]), nu=c["nv"] - c["f"], sigma=sigma, **kw)
    return c


def quirk_case():
    """quirk_graph at a size the window kernels take (57 free views): rows make_A drops ((free, fixed)), (fixed, free),
    (fixed, fixed), a self loop, long-range edges; measurements from a ground truth with 0.02 rad of noise."""
    I, _, n, f = quirk_graph(seed=3, n=60, f=3)
    rng = np.random.default_rng(33)
    Qgt = rng.normal(size=(n, 4))
    Qgt /= np.linalg.norm(Qgt, axis=1, keepdims=True)
    QQ = synth.qmul(synth.qexp(rng.normal(scale=0.02, size=(len(I), 3))), synth.qmul(Qgt[I[:, 1]], synth.qconj(Qgt[I[:, 0]])))
    Q0 = synth.qmul(synth.qexp(rng.normal(scale=0.03, size=(n, 3))), Qgt)
    Q0[:f] = Qgt[:f]
    return dict(I=I.astype(np.int32), QQ=QQ, Q0=Q0, f=f, nv=n)


def bridge_case(with_residual):
    """WC.planted(4) (3 fixed views at identity, 8 free ones) and one or two leaves, each held by ONE edge from a fixed
    view: bridges, leverage 1. Leaf A has a zero residual (identity pose, identity measurement): chi2 = 0 / 0 = NaN.
    Leaf B (with_residual) is measured 0.3 rad away from its pose: chi2 = +inf.
    Leverage is EXACTLY 1 only where the weight is a power of two (the 1 x 1 block of the leaf: d^2, scaled to 1,
    inverted, scaled back). Supplied weights plant d = 2 on the bridges. The weights of the poses are 1 / (|r|^2 +
    sigma^2): for leaf A that is 16 with sigma = 1/4, for leaf B no sigma makes it exact, so the case with leaf B is run
    with supplied weights only and the one without it in both modes."""
    c = WC.planted(4)
    nv = c["nv"]
    I, QQ, Q0 = [c["I"], [[0, nv]]], [c["QQ"], [[0, 0, 0, 1.0]]], [c["Q0"], [[0, 0, 0, 1.0]]]
    bridges = [len(c["I"])]
    if with_residual:
        I.append([[1, nv + 1]])
        QQ.append([WC.qrot(0.3, (1, 2, 2))])
        Q0.append([[0, 0, 0, 1.0]])
        bridges.append(len(c["I"]) + 1)
    return dict(I=np.concatenate(I).astype(np.int32), QQ=np.concatenate(QQ), Q0=np.concatenate(Q0), f=c["f"],
                nv=nv + len(bridges), bridges=bridges)


def shapes():
    """(nu, nv, ne) the kernel can go wrong at: nu = 1 with one edge (s^2 NaN), 2, 7 (not a multiple of the four row
    groups), 16 / 17, every limit at once, one edge past a 256-thread stride, f = 1 and f > 1."""
    S = [(1, 2, 1), (2, 4, 7), (7, 10, 25), (7, 8, 30), (16, 20, 60), (17, 18, 70), (20, 30, 257), (64, 320, 640),
         (64, 65, 640)]
    out = [named("size-%d-%d-%d" % s, WC.size_case(*s, seed=5)) for s in S]
    out.append(named("quirk", quirk_case()))
    out.append(named("bridge0", bridge_case(False), sigma=0.25))
    return out


CASES = shapes()                                              # both weight modes
SUPPLIED_ONLY = [named("bridge", bridge_case(True))]          # see bridge_case
SMALL3 = [named("rep-%d-%d-%d" % s, WC.size_case(*s, seed=21)) for s in ((10, 14, 40), (3, 4, 9), (12, 13, 50))]


def some_pairs(c, k=9, seed=0):
    """pairs of view ids: i == j, both fixed (where f >= 2), one fixed, free-free, random ones"""
    nv, f = c["nv"], c["f"]
    rng = np.random.default_rng([seed, nv])
    P = [(nv - 1, nv - 1), (0, 0), (0, nv - 1), (nv - 1, 0), (f, nv - 1), (f - 1, f)]
    if f >= 2:
        P.append((0, f - 1))
    P += [tuple(int(x) for x in rng.integers(0, nv, size=2)) for _ in range(k)]
    return np.array(P, dtype=np.int32)


# ---- the reference -------------------------------------------------------------------------------------------------------------
def residuals(c, Q=None):
    return T.log_map(T.delta_rel(c["I"], c["QQ"], c["Q0"] if Q is None else Q))[:, :3]


def pose_weights(c, Q=None):
    """d_k = 1 / (|r_k|^2 + sigma^2): Geman-McClure at a zero step, the view-graph definition"""
    return 1.0 / (np.sum(residuals(c, Q) ** 2, axis=1) + c["sigma"] ** 2)


def consistency(c, d):
    """max |M Sigma - I| of the reference's own inverse"""
    nu = c["nv"] - c["f"]
    p, q, w = edge_terms(c["I"], c["f"], d)
    M = np.zeros((nu, nu))
    np.add.at(M, (p, p), w)
    two = q >= 0
    np.add.at(M, (q[two], q[two]), w[two])
    np.add.at(M, (p[two], q[two]), -w[two])
    np.add.at(M, (q[two], p[two]), -w[two])
    return float(np.abs(M @ np.linalg.inv(M) - np.eye(nu)).max())


def reference(c, d, pairs=(), Q=None):
    """dict(var, pair_var, edge_var, leverage, chi2, scale) of problem c at weights d (and rotations Q, default Q0)"""
    res = residuals(c, Q)
    var, pv = dense_reference(c["I"], c["nv"], c["f"], d, [tuple(p) for p in pairs])
    e = edge_reference(c["I"], c["nv"], c["f"], d, res)
    assert e["scale"] == scale_reference(c["I"], c["f"], d, res, c["nv"] - c["f"]) or np.isnan(e["scale"])
    return dict(var=var, pair_var=pv, edge_var=e["edge_var"], leverage=e["leverage"], chi2=e["chi2"], scale=e["scale"])


def solved_weights_twin(c):
    """what a solve leaves, from the NumPy twin (the GPU test takes the library's): for picking cases on the CPU"""
    r = T.irls(c["QQ"], c["I"], c["Q0"], c["f"], 4, SIG, 30, 1e-3)
    return r["Q"], r["weights"]


@pytest.mark.parametrize("c", CASES + SUPPLIED_ONLY + SMALL3, ids=lambda c: c["name"])
def test_the_cases_are_ones_the_reference_can_be_trusted_on(c):
    assert 1 <= c["nu"] <= 64 and c["nv"] <= 320 and 1 <= c["ne"] <= 640
    modes = [("poses", pose_weights(c), None)]
    if c["name"] != "bridge0" and "bridges" not in c and c["nu"] > 1:
        Q, w = solved_weights_twin(c)
        modes.append(("solved", w, Q))
    for mode, d, Q in modes:
        worst = consistency(c, d)
        r = reference(c, d, some_pairs(c), Q)
        keep = c["I"][:, 1] >= c["f"]
        plain = keep.copy()
        plain[c.get("bridges", [])] = False
        # (with m_A <= nu, s^2 is NaN and every chi2 with it: the class of 1 - leverage does not matter there)
        gap = float((1.0 - r["leverage"][plain]).min()) if plain.any() and not np.isnan(r["scale"]) else 1.0
        print("%s %s: max|M Sigma - I| %.2e, min(1 - leverage) %.2e" % (c["name"], mode, worst, gap))
        assert worst < 1e-9
        assert gap > 1e-6
        nu = c["nv"] - c["f"]
        assert abs(r["leverage"].sum() - nu) <= 1e-9 * nu
        assert (r["edge_var"][~keep] == 0).all() and (r["var"][:c["f"]] == 0).all()


def test_the_shapes_the_issue_names_are_there():
    got = {(c["nu"], c["nv"], c["ne"]) for c in CASES}
    assert {(1, 2, 1), (64, 320, 640), (20, 30, 257)} <= got
    assert {2, 7, 16, 17} <= {c["nu"] for c in CASES}
    assert {c["f"] for c in CASES} >= {1, 3}
    one = [c for c in CASES if c["nu"] == 1 and c["ne"] == 1][0]
    r = reference(one, pose_weights(one))
    assert np.isnan(r["scale"]) and np.isnan(r["chi2"]).all() and np.isfinite(r["var"]).all()
    q = [c for c in CASES if c["name"] == "quirk"][0]
    assert (q["I"][:, 1] < q["f"]).any() and (q["I"][:, 0] == q["I"][:, 1]).any()


def test_the_planted_bridges_have_exact_answers_in_the_reference():
    b0 = [c for c in CASES if c["name"] == "bridge0"][0]
    r = reference(b0, pose_weights(b0))
    k = b0["bridges"][0]
    assert pose_weights(b0)[k] == 16.0 and r["leverage"][k] == 1.0 and np.isnan(r["chi2"][k])
    b = SUPPLIED_ONLY[0]
    d = pose_weights(b)
    d[b["bridges"]] = 2.0
    r = reference(b, d)
    ka, kb = b["bridges"]
    assert r["leverage"][ka] == 1.0 and r["leverage"][kb] == 1.0 and r["edge_var"][kb] == 0.25
    assert np.isnan(r["chi2"][ka]) and np.isposinf(r["chi2"][kb])


# ---- the symbols -----------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_listed():
    for name in (SINGLE, BATCH):
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name) and getattr(capi.lib(), name).argtypes is not None


# ---- irotavg_window_uncertainty: refusals before a device --------------------------------------------------------------------------
MARK = -7.0


def single(c, weights=True, var=True, pairs=None, pair_out=True, ev=True, lev=True, chi=True, scale=True, npairs=None,
           f=None, I=None):
    """the raw call on marker-filled outputs: (rc, outputs); nothing may be written by a refused call"""
    I = capi.edges(c["I"] if I is None else I)
    QQ, Q = capi.fmat(c["QQ"]), capi.fmat(c["Q0"])
    m, n = len(I), Q.shape[0]
    w = np.ones(m)
    P = np.zeros((0, 2), dtype=np.int32) if pairs is None else np.ascontiguousarray(pairs, dtype=np.int32)
    out = dict(var=np.full(n, MARK), pair_var=np.full(max(len(P), 1), MARK), edge_var=np.full(m, MARK),
               leverage=np.full(m, MARK), chi2=np.full(m, MARK))
    s = C.c_double(MARK)
    dp, ip = capi._d, capi._i
    rc = capi.lib().irotavg_window_uncertainty(
        m, n, c["f"] if f is None else f, ip(I), dp(QQ), max(m, 1), dp(Q), n, dp(w) if weights else None, SIG,
        dp(out["var"]) if var else None, len(P) if npairs is None else npairs, ip(P) if len(P) else None,
        dp(out["pair_var"]) if pair_out else None, dp(out["edge_var"]) if ev else None, dp(out["leverage"]) if lev else None,
        dp(out["chi2"]) if chi else None, C.byref(s) if scale else None)
    out["scale"] = np.array([s.value])
    return rc, out


def untouched(out):
    return all((a == MARK).all() for a in out.values())


GOOD = named("good", WC.size_case(7, 10, 25, seed=5))


@pytest.mark.parametrize("name,kernel,c", [p for p in WC.past_limits() if p[1] == 0], ids=lambda p: str(p))
def test_single_refuses_what_window_fits_refuses(name, kernel, c):
    rc, out = single(named(name, c))
    assert rc == capi.ERR_BAD_ARG and untouched(out)


def test_single_refuses_bad_ids_counts_and_an_empty_request():
    for bad in (-1, GOOD["nv"], 2 ** 31 - 1):
        for col in (0, 1):
            I = GOOD["I"].copy()
            I[3, col] = bad
            rc, out = single(GOOD, I=I)
            assert rc == capi.ERR_BAD_ARG and untouched(out)
        rc, out = single(GOOD, pairs=[(0, 1), (bad, 2)])
        assert rc == capi.ERR_BAD_ARG and untouched(out)
        rc, out = single(GOOD, pairs=[(2, bad)])
        assert rc == capi.ERR_BAD_ARG and untouched(out)
    for f in (-1, GOOD["nv"], GOOD["nv"] + 5):
        rc, out = single(GOOD, f=f)
        assert rc == capi.ERR_BAD_ARG and untouched(out)
    rc, out = single(GOOD, npairs=-1)
    assert rc == capi.ERR_BAD_ARG and untouched(out)
    rc, out = single(GOOD, pairs=[(0, 1)], pair_out=False)                  # a pair count without its output
    assert rc == capi.ERR_BAD_ARG and untouched(out)
    rc, out = single(GOOD, npairs=2)                                        # ... without its ids
    assert rc == capi.ERR_BAD_ARG and untouched(out)
    rc, out = single(GOOD, var=False, ev=False, lev=False, chi=False, scale=False)   # nothing asked for
    assert rc == capi.ERR_BAD_ARG and untouched(out)
    L = capi.lib()
    assert L.irotavg_window_uncertainty(1, 2, 1, None, None, 1, None, 2, None, SIG, None, 0, None, None, None, None, None,
                                        None) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [dict(), dict(weights=False), dict(var=False, ev=False, lev=False, chi=False),
                                dict(var=False, ev=False, lev=False, chi=False, scale=False, pairs=[(0, 4)]),
                                dict(pairs=[(1, 1), (0, 9), (9, 0)])], ids=str)
def test_a_well_formed_single_call_needs_a_device(kw):
    if capi.lib().irotavg_device_count() > 0:
        pytest.skip("a HIP device exists")
    rc, out = single(GOOD, **kw)
    assert rc == capi.ERR_NO_DEVICE and untouched(out)
    with pytest.raises(capi.IrotavgError) as e:
        capi.window_uncertainty(GOOD["I"], GOOD["QQ"], GOOD["Q0"], GOOD["f"])
    assert e.value.code == capi.ERR_NO_DEVICE


# ---- irotavg_window_uncertainty_batch_dev: refusals before a device ------------------------------------------------------------------
# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE = {k: C.c_void_p(0x10000 * (i + 1)) for i, k in enumerate(("I", "QQ", "Q", "w", "var", "pairs", "pv", "ev", "lev", "chi"))}
SIZES = [(12, 2, 40), (320, 256, 640), (2, 1, 1)]


def batch(sizes=SIZES, nb=None, qq=(4, 1), q=(4, 1), npairs=None, null_sizes=False, scale=True, results=True, **ptr):
    s = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 3)
    p = dict(FAKE)
    p.update(ptr)
    npr = None if npairs is None else np.ascontiguousarray(npairs, dtype=np.int32)
    sc = np.full(max(len(s), 1), MARK)
    res = np.full(max(len(s), 1), -99, dtype=np.int32)
    i32 = C.POINTER(C.c_int32)
    rc = capi.lib().irotavg_window_uncertainty_batch_dev(
        len(s) if nb is None else nb, None if null_sizes else s.ctypes.data_as(i32), p["I"], p["QQ"], qq[0], qq[1], p["Q"],
        q[0], q[1], p["w"], SIG, p["var"], None if npr is None else npr.ctypes.data_as(i32), p["pairs"], p["pv"], p["ev"],
        p["lev"], p["chi"], sc.ctypes.data_as(C.POINTER(C.c_double)) if scale else None,
        res.ctypes.data_as(i32) if results else None, None)
    assert (res == -99).all() and (sc == MARK).all()
    return rc


@pytest.mark.parametrize("bad", [(66, 1, 100), (321, 300, 100), (70, 6, 641), (20, 20, 30), (20, 1, 0), (20, -1, 30),
                                 (0, 0, 5), (-3, 0, 5), (20, 21, 30), (2 ** 31 - 1, 2 ** 31 - 2, 5), (5, 1, -2)])
def test_batch_refuses_a_problem_outside_the_limits(bad):
    assert batch(SIZES[:2] + [bad] + SIZES[2:]) == capi.ERR_BAD_ARG


def test_batch_refuses_counts_pointers_pairs_and_an_empty_request():
    assert batch(nb=0) == capi.ERR_BAD_ARG
    assert batch(nb=-1) == capi.ERR_BAD_ARG
    assert batch(nb=262145) == capi.ERR_BAD_ARG
    assert batch(null_sizes=True) == capi.ERR_BAD_ARG
    for k in ("I", "QQ", "Q"):
        assert batch(**{k: None}) == capi.ERR_BAD_ARG
    for k in FAKE:                                                           # not 8-byte aligned
        npairs = [1, 0, 2] if k in ("pairs", "pv") else None
        assert batch(npairs=npairs, **{k: C.c_void_p(FAKE[k].value + 4)}) == capi.ERR_BAD_ARG, k
    assert batch(npairs=[1, -1, 2]) == capi.ERR_BAD_ARG                      # a negative pair count
    assert batch(npairs=[1, 0, 2], pairs=None) == capi.ERR_BAD_ARG           # a pair count without its arrays
    assert batch(npairs=[1, 0, 2], pv=None) == capi.ERR_BAD_ARG
    nothing = dict(var=None, ev=None, lev=None, chi=None, scale=False)
    assert batch(**nothing) == capi.ERR_BAD_ARG                              # nothing asked for
    assert batch(npairs=[0, 0, 0], **nothing) == capi.ERR_BAD_ARG
    assert batch(results=False, **nothing) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("rs,cs", [(0, 0), (0, 1), (4, 0), (1, 1), (2, 1), (3, 1), (1, 2), (1, 99), (-2, 1), (2, 3),
                                   (2 ** 40, 1), (-2 ** 63, 1), (1, -2 ** 63)])
def test_batch_refuses_strides_that_alias(rs, cs):
    assert batch(qq=(rs, cs)) == capi.ERR_BAD_ARG
    assert batch(q=(rs, cs)) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("rs,cs", [(4, 1), (1, 681), (6, 1), (-4, 1), (1, -700), (4, -1), (2 ** 31, 1)])
def test_a_well_formed_batch_call_needs_a_device(rs, cs):
    if capi.lib().irotavg_device_count() > 0:
        pytest.skip("a HIP device exists")
    assert batch(qq=(rs, cs), q=(rs, cs)) == capi.ERR_NO_DEVICE
    assert batch(qq=(rs, cs), q=(rs, cs), w=None, npairs=[3, 0, 2000]) == capi.ERR_NO_DEVICE
    only_scale = dict(var=None, ev=None, lev=None, chi=None)
    assert batch(qq=(rs, cs), **only_scale) == capi.ERR_NO_DEVICE
    assert batch(scale=False, results=False, npairs=[0, 1, 0], **only_scale) == capi.ERR_NO_DEVICE   # one pair is a request


# ---- the torch front-end ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_c_calls(monkeypatch):
    """Any use of the C library from here on is an error."""
    from irotavg_amd import torch_api

    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    return torch_api


def tensors(m=41, n=14):
    return (torch.zeros((m, 2), dtype=torch.int32), torch.zeros((m, 4), dtype=torch.float64),
            torch.zeros((n, 4), dtype=torch.float64))


TSIZES = np.array([(12, 2, 40), (2, 1, 1)])


def test_wrapper_rejects_cpu_tensors_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    with pytest.raises(TypeError, match="ROCm device"):
        no_c_calls.window_uncertainty_batch(TSIZES, ei, QQ, Q)
    with pytest.raises(TypeError):
        no_c_calls.window_uncertainty_batch(TSIZES, ei.numpy(), QQ, Q)


def test_wrapper_rejects_wrong_dtypes_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    f = no_c_calls.window_uncertainty_batch
    with pytest.raises(TypeError, match="float64"):
        f(TSIZES, ei, QQ.float(), Q)
    with pytest.raises(TypeError, match="float64"):
        f(TSIZES, ei, QQ, Q.float())
    with pytest.raises(TypeError, match="int32"):
        f(TSIZES, ei.to(torch.int16), QQ, Q)
    with pytest.raises(TypeError, match="integers"):
        f(TSIZES.astype(np.float64), ei, QQ, Q)
    with pytest.raises(TypeError, match="integers"):
        f(TSIZES, ei, QQ, Q, pairs=torch.zeros((3, 2), dtype=torch.int32), npairs=np.array([1.0, 2.0]))
    with pytest.raises(TypeError, match="int32"):
        f(TSIZES, ei, QQ, Q, pairs=torch.zeros((3, 2), dtype=torch.float64), npairs=[1, 2])


def test_wrapper_rejects_wrong_shapes_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    f = no_c_calls.window_uncertainty_batch
    with pytest.raises(ValueError, match="sizes"):
        f(TSIZES.ravel(), ei, QQ, Q)
    with pytest.raises(ValueError, match="edge_index"):
        f(TSIZES, ei[:-1], QQ, Q)
    with pytest.raises(ValueError, match="QQ"):
        f(TSIZES, ei, QQ[:, :3], Q)
    with pytest.raises(ValueError, match="Q must"):
        f(TSIZES, ei, QQ, Q[:-1])
    pairs = torch.zeros((3, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match="together"):
        f(TSIZES, ei, QQ, Q, pairs=pairs)
    with pytest.raises(ValueError, match="together"):
        f(TSIZES, ei, QQ, Q, npairs=[1, 2])
    with pytest.raises(ValueError, match="npairs"):
        f(TSIZES, ei, QQ, Q, pairs=pairs, npairs=[1, 1, 1])                  # one count per problem
    with pytest.raises(ValueError, match="npairs"):
        f(TSIZES, ei, QQ, Q, pairs=pairs, npairs=[4, -1])
    with pytest.raises(ValueError, match="pairs"):
        f(TSIZES, ei, QQ, Q, pairs=pairs, npairs=[1, 1])                     # sum npairs differs


def test_pair_offsets_are_the_cumulative_sums():
    from irotavg_amd import torch_api
    rng = np.random.default_rng(6)
    c = rng.integers(0, 5000, size=700)
    c[::7] = 0
    c32, off, total = torch_api.pair_offsets(c, 700)
    assert c32.dtype == np.int32 and c32.flags.c_contiguous and (c32 == c).all()
    np.testing.assert_array_equal(off, np.cumsum(c) - c)
    assert total == c.sum() and off[0] == 0 and off.dtype == np.int64
    big = np.full(262144, 2 ** 31 - 1, dtype=np.int64)                      # sums that do not fit int32
    _, off, total = torch_api.pair_offsets(big, 262144)
    assert total == 262144 * (2 ** 31 - 1) and off[-1] == 262143 * (2 ** 31 - 1)
    assert torch_api.pair_offsets(None, 3)[0] is None and torch_api.pair_offsets(None, 3)[2] == 0
    _, off, total = torch_api.pair_offsets(torch.tensor(c), 700)            # a host tensor is a host array
    assert total == c.sum()
