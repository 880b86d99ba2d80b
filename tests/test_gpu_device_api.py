"""The device-pointer handle API on the GPU (irotavg_graph_*_dev, irotavg_amd/csrc/devapi.hip, irotavg_amd/torch_api.py)
against the host-pointer API on the same inputs. The device route is a copy in front of and behind the same kernels,
so the tolerance of every comparison is BITWISE equality; the host-side handle of each pair is created with
IROTAVG_HOST_BUILD=0, so both sides run the same build code."""
import contextlib
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from irotavg_amd import capi, graphio, ral, synth
from irotavg_amd.torch_api import TorchGraph

pytestmark = pytest.mark.gpu

SIGMA = 5 * np.pi / 180
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("edge_var", "leverage", "chi2")
SENTINEL = -777.25


def dev():
    return torch.device("cuda", torch.cuda.current_device())


@contextlib.contextmanager
def device_build():
    old = os.environ.get("IROTAVG_HOST_BUILD")
    os.environ["IROTAVG_HOST_BUILD"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["IROTAVG_HOST_BUILD"]
        else:
            os.environ["IROTAVG_HOST_BUILD"] = old


def host_graph(I, QQ, n, f, **opts):
    with device_build():
        return capi.Graph(I, QQ, n, f, **opts)


def start(I, QQ, n, f, Q_fixed):
    Q = np.zeros((n, 4))
    Q[:, 3] = 1
    Q[:f] = Q_fixed[:f]
    return ral.init_mst(Q, QQ, I, f)


def sequence(n, m, ncl=0, seed=1):
    S = synth.make_graph(n, m, 0.0, seed=seed)
    I, QQ = S["I"], S["QQ"]
    if ncl:
        rng = np.random.default_rng(seed + 100)
        a = rng.integers(0, n - 400, size=ncl)
        b = np.minimum(a + rng.integers(200, n - a), n - 1)
        I = np.concatenate([I, np.stack([a, b], 1)])
        QQ = np.concatenate([QQ, synth.qmul(S["Qgt"][b], synth.qconj(S["Qgt"][a]))])
    return I.astype(np.int32), QQ, S["Qgt"]


def build_case(case):
    """I, QQ, n, f, Q0, opts"""
    if case == "fixture":          # ral/data: one dense level
        g = graphio.read_ravg_input(os.path.join(ROOT, "tests", "golden", "ravg_input.txt"))
        f = g["f"]
        Q0 = ral.init_mst(g["Q"].copy(), g["QQ"], g["I"], max(g["n_abs_read"], f))
        return g["I"], g["QQ"], g["n"], f, Q0, {}
    if case == "pcg":              # general topology: the multigrid PCG
        n = 5000
        S = synth.make_graph(n, 20 * n, 0.02, seed=11)
        I = S["I"].astype(np.int32)
        return I, S["QQ"], n, 1, start(I, S["QQ"], n, 1, S["Qgt"]), dict(band_direct=-1)
    if case == "full":             # 100k views / 2M edges
        n, m, ncl = 100000, 2000000, 0
    else:                          # a view sequence above 2048 free views, without / with loop closures
        n, m, ncl = 3000, 12 * 3000 - 78, (40 if case == "closures" else 0)
    I, QQ, Qgt = sequence(n, m, ncl=ncl, seed=21)
    return I, QQ, n, 1, start(I, QQ, n, 1, Qgt), {}


def t64(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev())


def tidx(I, dtype=torch.int32):
    return torch.tensor(np.ascontiguousarray(I), dtype=dtype, device=dev())


def same(a, b):
    """bitwise, NaN == NaN"""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape
    np.testing.assert_array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                  b.view(np.uint64) if b.dtype == np.float64 else b)


def solve(G, l1=2):
    a = G.l1ra(l1, 1e-3)
    b = G.irls(4, SIGMA, 50, 1e-3)
    return a["iters"], b["iters"]


def compare_state(H, D):
    """rotations, weights and residuals of a host handle and a device-built one, through both kinds of getters"""
    H.edge_residual()
    D.edge_residual()
    Qh, wh, rh = H.get_rotations(), H.get_weights(), H.get_residuals()
    same(D.get_rotations(), Qh)
    same(D.get_weights(), wh)
    same(D.get_residuals(), rh)
    same(D.rotations(), np.ascontiguousarray(Qh))
    same(D.weights(), wh)
    same(D.residuals(), np.ascontiguousarray(rh))


# ---- 1. fingerprint and solve --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fixture", "band", "closures", "pcg", "full"])
def test_fingerprint_and_solve(case):
    I, QQ, n, f, Q0, opts = build_case(case)
    with host_graph(I, QQ, n, f, **opts) as H, TorchGraph(tidx(I), t64(QQ), n, f, **opts) as D:
        assert D.fingerprint() == H.fingerprint()
        assert D.direct_info() == H.direct_info()
        if case in ("band", "closures", "full"):
            assert D.stats()["band_block"] > 0
        if case == "closures":
            assert D.direct_info()["closures"] == 40
        if case == "pcg":
            assert D.stats()["band_block"] == 0
        H.set_rotations(Q0)
        D.set_rotations(t64(Q0))
        assert solve(D) == solve(H)
        if case == "pcg":
            assert D.stats()["pcg_solves"] > 0
        compare_state(H, D)


# ---- 2. layouts ----------------------------------------------------------------------------------------------------------
def plane_ld(rows):
    return rows + 6 + rows % 2          # ld > rows and even: the 16-byte path, also when rows is odd


def layouts(A):
    """a (rows, 4) array as device tensors of three layouts + the base tensors they view"""
    rows = A.shape[0]
    out = {}
    out["contiguous"] = (t64(A), None)
    base = torch.full((4, plane_ld(rows)), 3.5, dtype=torch.float64, device=dev())     # column-major planes, ld > rows
    base[:, :rows] = t64(A).t()
    out["planes"] = (base[:, :rows].t(), base)
    wide = torch.full((rows, 6), 3.5, dtype=torch.float64, device=dev())         # a column slice of a wider tensor
    wide[:, 1:5] = t64(A)
    out["strided"] = (wide[:, 1:5], wide)
    return out


@pytest.mark.parametrize("case", ["closures", "odd"])
def test_layouts(case):
    if case == "odd":          # odd m and odd n: the two-rows-per-thread paths end in a single row
        I, QQ, Qgt = sequence(2999, 12 * 2999 - 78 - 1, seed=5)
        n, f, Q0, opts = 2999, 1, start(I, QQ, 2999, 1, Qgt), {}
        assert len(I) % 2 == 1
    else:
        I, QQ, n, f, Q0, opts = build_case(case)
    ei = tidx(I)
    ei_before = ei.clone()
    results = []
    for name, (q, base) in layouts(QQ).items():
        strides = (q.stride(0), q.stride(1))
        assert strides == dict(contiguous=(4, 1), planes=(1, plane_ld(len(I))), strided=(6, 1))[name]
        keep = (q.clone(), None if base is None else base.clone())
        with TorchGraph(ei, q, n, f, **opts) as D:
            fp = D.fingerprint()
            # rotations set and read through every layout round-trip bitwise
            for lname, (r, rbase) in layouts(Q0).items():
                rkeep = None if rbase is None else rbase.clone()
                D.set_rotations(r)
                same(D.get_rotations(), Q0)
                for oname, (o, obase) in layouts(np.zeros_like(Q0)).items():
                    got = D.rotations(out=o)
                    assert got is o
                    same(o, Q0)
                    if obase is not None:                         # nothing outside the view was written
                        mask = torch.ones_like(obase, dtype=torch.bool)
                        (mask[:, :n] if oname == "planes" else mask[:, 1:5]).fill_(False)
                        assert bool((obase[mask] == 3.5).all())
                same(r, Q0)                                       # the input is unchanged
                if rbase is not None:
                    same(rbase, rkeep)
            iters = solve(D)
            D.edge_residual()
            results.append((name, fp, iters, D.get_rotations(), D.get_weights(), D.get_residuals()))
        same(q, keep[0])                                          # the caller's tensors are unchanged
        if base is not None:
            same(base, keep[1])
    same(ei, ei_before)
    with host_graph(I, QQ, n, f, **opts) as H:
        H.set_rotations(Q0)
        ref = (H.fingerprint(), solve(H))
        H.edge_residual()
        ref += (H.get_rotations(), H.get_weights(), H.get_residuals())
    for name, fp, iters, Q, w, r in results:
        assert fp == ref[0] and iters == ref[1], name
        same(Q, ref[2])
        same(w, ref[3])
        same(r, ref[4])


def test_int64_edge_index_is_narrowed_on_the_device():
    I, QQ, n, f, Q0, opts = build_case("band")
    with TorchGraph(tidx(I), t64(QQ), n, f) as A, TorchGraph(tidx(I, torch.int64), t64(QQ), n, f) as B:
        assert A.fingerprint() == B.fingerprint()
    big = tidx(I, torch.int64)
    big[7, 1] = 2 ** 32 + 5            # would alias view 5 if it were truncated
    with pytest.raises(ValueError):
        TorchGraph(big, t64(QQ), n, f)


# ---- 3. queries ----------------------------------------------------------------------------------------------------------
def solved_pair(case, l1=2):
    I, QQ, n, f, Q0, opts = build_case(case)
    H = host_graph(I, QQ, n, f, **opts)
    D = TorchGraph(tidx(I), t64(QQ), n, f, **opts)
    H.set_rotations(Q0)
    D.set_rotations(t64(Q0))
    assert solve(H, l1) == solve(D, l1)
    return I, n, f, H, D


def stats_wo_time(G):
    return {k: v for k, v in G.stats().items() if not k.startswith("seconds")}


@pytest.mark.parametrize("case", ["fixture", "band", "closures"])
def test_queries_equal_the_host_calls(case):
    I, n, f, H, D = solved_pair(case)
    with H, D:
        H.edge_residual()
        D.edge_residual()
        before = (D.get_rotations(), D.get_weights(), D.get_residuals(), stats_wo_time(D))
        rv_h = H.rotation_variance()
        rv_d = D.variance()
        assert rv_d["rc"] == capi.OK
        same(rv_d["var"], rv_h["var"])
        assert np.float64(rv_d["scale"]).view(np.uint64) == np.float64(rv_h["scale"]).view(np.uint64)
        assert np.isfinite(rv_d["scale"]) and bool((rv_d["var"][:f] == 0).all())
        full = H.edge_diagnostics()
        for want in itertools.product((False, True), repeat=3):          # every subset of the three arrays
            r = D.edge_diagnostics(*want)
            for k, on in zip(KEYS, want):
                if on:
                    same(r[k], full[k])
                else:
                    assert r[k] is None
            assert np.float64(r["scale"]).view(np.uint64) == np.float64(full["scale"]).view(np.uint64)
        # read-only: state, weights, residuals, counters
        same(D.get_rotations(), before[0])
        same(D.get_weights(), before[1])
        same(D.get_residuals(), before[2])
        assert stats_wo_time(D) == before[3]
        # ... and a following irls is the one of the twin
        Qa = H.get_rotations()
        Qp = synth.qmul(synth.qexp(np.random.default_rng(4).normal(scale=0.01, size=(n, 3))), Qa)
        Qp[:f] = Qa[:f]
        H.set_rotations(Qp)
        D.set_rotations(t64(Qp))
        a, b = H.irls(4, SIGMA, 50, 1e-3), D.irls(4, SIGMA, 50, 1e-3)
        assert a["iters"] == b["iters"]
        same(a["scores"], b["scores"])
        compare_state(H, D)


def sentinels(D):
    return dict(var=torch.full((D.n_total,), SENTINEL, dtype=torch.float64, device=D.device),
                **{k: torch.full((D.m,), SENTINEL, dtype=torch.float64, device=D.device) for k in KEYS})


def assert_untouched(s):
    for k, t in s.items():
        assert bool((t == SENTINEL).all()), k


def test_pcg_handle_is_unsupported_and_writes_nothing():
    I, QQ, n, f, Q0, opts = build_case("pcg")
    with TorchGraph(tidx(I), t64(QQ), n, f, **opts) as D:
        D.set_rotations(t64(Q0))
        s = sentinels(D)
        r = D.variance(out=s["var"], allow_rc=(capi.ERR_UNSUPPORTED,))
        assert r["rc"] == capi.ERR_UNSUPPORTED and np.isnan(r["scale"])
        r = D.edge_diagnostics(s["edge_var"], s["leverage"], s["chi2"], allow_rc=(capi.ERR_UNSUPPORTED,))
        assert r["rc"] == capi.ERR_UNSUPPORTED and np.isnan(r["scale"])
        torch.cuda.synchronize()
        assert_untouched(s)


@pytest.mark.parametrize("case", ["fixture", "band", "closures"])
def test_singular_system_is_an_error_and_writes_nothing(case):
    I, QQ, n, f, Q0, opts = build_case(case)
    with TorchGraph(tidx(I), t64(QQ), n, f, **opts) as D, host_graph(I, QQ, n, f, **opts) as H:
        D.set_rotations(t64(Q0))
        H.set_rotations(Q0)
        v = f + (n - f) // 2
        d = np.ones(len(I))
        d[(I[:, 0] == v) | (I[:, 1] == v)] = 0.0          # view v is cut off
        D.set_weights(t64(d))
        H.set_weights(d)
        same(D.get_weights(), d)
        s = sentinels(D)
        r = D.variance(out=s["var"], allow_rc=(capi.ERR_SOLVER,))
        assert r["rc"] == capi.ERR_SOLVER and np.isnan(r["scale"])
        r = D.edge_diagnostics(s["edge_var"], s["leverage"], s["chi2"], allow_rc=(capi.ERR_SOLVER,))
        assert r["rc"] == capi.ERR_SOLVER and np.isnan(r["scale"])
        torch.cuda.synchronize()
        assert_untouched(s)
        # the handle is as good as before: the same irls as the twin that was never queried
        D.set_weights(t64(np.ones(len(I))))
        H.set_weights(np.ones(len(I)))
        a, b = H.irls(4, SIGMA, 50, 1e-3), D.irls(4, SIGMA, 50, 1e-3)
        assert a["iters"] == b["iters"]
        compare_state(H, D)


# ---- 4. stream ordering -----------------------------------------------------------------------------------------------------
def busy_zero(k=8192, reps=6):
    """A float64 zero on the device that is ready only after `reps` large matrix products on the current stream."""
    A = torch.randn((k, k), device=dev())
    for _ in range(reps):
        A = A @ A
        A = A / A.norm()
    return (A[0, 0] * 0.0).to(torch.float64)


@pytest.mark.parametrize("which", ["side_stream", "null_stream"])
def test_stream_ordering_without_a_synchronise(which):
    I, QQ, n, f, Q0, opts = build_case("closures")
    qq_base, q0_base, ei = t64(QQ), t64(Q0), tidx(I)
    busy_zero(reps=1)                          # the first product of a process sets the BLAS library up on the host
    torch.cuda.synchronize()                   # the uploads; from here on nothing synchronises until the results are read
    stream = torch.cuda.Stream() if which == "side_stream" else torch.cuda.default_stream()
    if which == "null_stream":
        assert stream.cuda_stream == 0
    with torch.cuda.stream(stream):
        z = busy_zero()
        qq = qq_base + z                       # the tensor that becomes QQ: behind the products
        q0 = q0_base + z
        pending = not stream.query()
        D = TorchGraph(ei, qq, n, f, **opts)   # inputs not ready when the call is made
        pending2 = None
        z2 = busy_zero(reps=3)
        q0 = q0 + z2
        pending2 = not stream.query()
        D.set_rotations(q0)                    # asynchronous, behind the second batch of products
        iters = solve(D)
        D.edge_residual()
        R = D.rotations() * 1.0                # consumed by torch ops on the same stream, no synchronise
        w = D.weights() + 0.0
        r = D.residuals() + 0.0
        ed = D.edge_diagnostics()
        lev = ed["leverage"] * 1.0
        var = D.variance()["var"] * 1.0
    print("work pending on the stream at create_dev: %s, at set_rotations_dev: %s" % (pending, pending2))
    assert pending and pending2, "the queued products had finished before the calls: the test showed nothing"
    stream.synchronize()
    assert float(z) == 0.0 and float(z2) == 0.0
    QQh, Q0h = qq.cpu().numpy(), q0.cpu().numpy()
    with D, host_graph(I, QQh, n, f, **opts) as H:
        H.set_rotations(Q0h)
        assert solve(H) == iters
        H.edge_residual()
        same(R, np.ascontiguousarray(H.get_rotations()))
        same(w, H.get_weights())
        same(r, np.ascontiguousarray(H.get_residuals()))
        same(lev, H.edge_diagnostics()["leverage"])
        same(var, H.rotation_variance()["var"])


# ---- 5. errors that must not reach a kernel -----------------------------------------------------------------------------------
def raw_create(I_ptr, QQ_ptr, m, n, f, rs=4, cs=1, device=-1):
    h = C.c_void_p(0xdead)
    o = capi.default_options(device=device)
    rc = capi.lib().irotavg_graph_create_dev(C.byref(h), m, n, f, C.c_void_p(I_ptr), C.c_void_p(QQ_ptr), rs, cs,
                                             C.byref(o), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, h


def valid_call_succeeds(I, QQ, n, f, Q0):
    with TorchGraph(tidx(I), t64(QQ), n, f) as D:
        D.set_rotations(t64(Q0))
        assert D.irls(4, SIGMA, 50, 1e-3)["rc"] == capi.OK
        assert np.isfinite(D.rotations().cpu().numpy()).all()


def test_host_pointer_is_a_bad_argument():
    I, QQ, n, f, Q0, _ = build_case("band")
    ei, qq = tidx(I), t64(QQ)
    QQh = np.ascontiguousarray(QQ)
    Ih = np.ascontiguousarray(I)
    rc, h = raw_create(ei.data_ptr(), QQh.ctypes.data, len(I), n, f)          # NumPy memory as QQ_dev
    assert rc == capi.ERR_BAD_ARG and not h.value
    rc, h = raw_create(Ih.ctypes.data, qq.data_ptr(), len(I), n, f)           # ... as I_dev
    assert rc == capi.ERR_BAD_ARG and not h.value
    with TorchGraph(ei, qq, n, f) as D:                                       # ... as the array of a handle call
        L, s = capi.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
        Qh = np.ascontiguousarray(Q0)
        wh = np.ones(len(I))
        assert L.irotavg_graph_set_rotations_dev(D._h, C.c_void_p(Qh.ctypes.data), 4, 1, s) == capi.ERR_BAD_ARG
        assert L.irotavg_graph_get_rotations_dev(D._h, C.c_void_p(Qh.ctypes.data), 4, 1, s) == capi.ERR_BAD_ARG
        assert L.irotavg_graph_set_weights_dev(D._h, C.c_void_p(wh.ctypes.data), s) == capi.ERR_BAD_ARG
        assert L.irotavg_graph_get_weights_dev(D._h, C.c_void_p(wh.ctypes.data), s) == capi.ERR_BAD_ARG
        assert L.irotavg_graph_rotation_variance_dev(D._h, C.c_void_p(Qh.ctypes.data), None, s) == capi.ERR_BAD_ARG
        assert L.irotavg_graph_edge_diagnostics_dev(D._h, C.c_void_p(wh.ctypes.data), None, None, None, s) == capi.ERR_BAD_ARG
        same(Qh, Q0)
        # a device array that is too short for its strides: the highest element lies outside device memory or the check
        # of the strides refuses it
        assert L.irotavg_graph_set_rotations_dev(D._h, C.c_void_p(t64(Q0).data_ptr()), 2, 1, s) == capi.ERR_BAD_ARG
    valid_call_succeeds(I, QQ, n, f, Q0)


def test_wrong_device_is_a_bad_argument():
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    I, QQ, n, f, Q0, _ = build_case("band")
    other = torch.device("cuda", (torch.cuda.current_device() + 1) % torch.cuda.device_count())
    qq_other = torch.tensor(QQ, dtype=torch.float64, device=other)
    rc, h = raw_create(tidx(I).data_ptr(), qq_other.data_ptr(), len(I), n, f, device=torch.cuda.current_device())
    assert rc == capi.ERR_BAD_ARG and not h.value
    with pytest.raises(ValueError):
        TorchGraph(tidx(I), qq_other, n, f)
    valid_call_succeeds(I, QQ, n, f, Q0)


def test_edge_index_out_of_range_is_a_bad_argument():
    I, QQ, n, f, Q0, _ = build_case("band")
    for bad in (n, -1):
        Ib = I.copy()
        Ib[len(I) // 2, 1] = bad
        ei, qq = tidx(Ib), t64(QQ)
        rc, h = raw_create(ei.data_ptr(), qq.data_ptr(), len(I), n, f)
        assert rc == capi.ERR_BAD_ARG and not h.value
        with pytest.raises(ValueError):
            TorchGraph(ei, qq, n, f)
    valid_call_succeeds(I, QQ, n, f, Q0)
