"""The rotation-variance query and the edge diagnostics on the device (irotavg_amd/csrc/marginals.hip, edgediag.hip) at the
block edges of their own factorisation: the cases of variance_cases.py against the NumPy references of
test_rotation_variance_cpu.py / test_edge_diagnostics_cpu.py (held to each other, and shown to see a wrong index, in
test_variance_cases_cpu.py). Every handle is first asked whether it IS the case -- block size and closure count as
variance_cases.plan() computed them in Python -- so that a case which no longer reaches its edge fails instead of passing
somewhere else.

Tolerance: relative 1e-9, the figure of test_gpu_rotation_variance.py and test_gpu_edge_diagnostics.py for these queries (the
references agree with each other to 1e-11 and better); 1e-6 for pairs through the multigrid PCG, as there. Every test prints its
worst relative error."""
import functools

import numpy as np
import pytest

import variance_cases as VC
from irotavg_amd import capi
from irotavg_amd.torch_api import TorchGraph   # (imported here as in test_gpu_device_api.py: torch must be loaded before the
from test_edge_diagnostics_cpu import band_edge_reference, edge_reference          # library first touches the device)
from test_gpu_device_api import same, t64, tidx
from test_gpu_edge_diagnostics import KEYS, check_all, state_of, untouched
from test_gpu_rotation_variance import _stats_wo_time
from test_rotation_variance_cpu import band_reference, dense_reference, scale_reference

pytestmark = pytest.mark.gpu

RTOL = 1e-9
RTOL_PCG = 1e-6


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def worst(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    if not got.size:
        return 0.0
    with np.errstate(all="ignore"):
        err = np.where(got == ref, 0.0, np.abs(got - ref) / np.abs(ref))
    return float(np.where(np.isfinite(err), err, np.inf).max())


def check_variance(r, var, pv, case, rtol=RTOL):
    """r: dict(var, pair_var) of a query. Fixed views exactly zero, free views and the pairs that are not zero by definition
    within rtol of (var, pv), the pairs that are (i == j, both ends fixed) exactly zero."""
    f = case["f"]
    if r["var"] is not None:
        assert np.all(r["var"][:f] == 0)
        e = worst(r["var"][f:], var[f:])
        print("%s: marginals, worst relative error over %d views: %.3e" % (case["name"], case["nu"], e))
        assert e < rtol
    z = VC.zero_pairs(case)
    assert np.all(np.asarray(r["pair_var"])[z] == 0) and np.all(np.asarray(pv)[z] == 0)
    e = worst(np.asarray(r["pair_var"])[~z], np.asarray(pv)[~z])
    print("%s: pairs, worst relative error over %d pairs: %.3e" % (case["name"], int((~z).sum()), e))
    assert e < rtol


def check_edges(r, ref, case):
    """test_gpu_edge_diagnostics.check_all (classes of 0 / inf / NaN equal, the rest within 1e-9, the trace, the range) and
    the closures of weight zero: a finite edge_var, leverage and chi2 exactly zero."""
    print("%s: edge diagnostics" % case["name"])
    check_all(r, ref, case["nu"])
    dead = case["far"][case["d"][case["far"]] == 0]
    if len(dead):
        assert np.all(np.isfinite(r["edge_var"][dead])) and np.all(r["edge_var"][dead] > 0)
        assert np.all(r["leverage"][dead] == 0) and np.all(r["chi2"][dead] == 0)


# ---- references: computed once per case, read-only ---------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def variance_reference(name):
    """(var, pair variances, band-only var or None): the block reference at the case's own B on the band route, the dense
    inverse elsewhere."""
    c = VC.CASE[name]
    if c["route"] == "band":
        return _frozen(*band_reference(c["I"], c["n"], c["f"], c["d"], c["B"], VC.pairs_of(c)))
    return _frozen(*dense_reference(c["I"], c["n"], c["f"], c["d"], VC.pairs_of(c))) + (None,)


def edges_reference(c, res):
    if c["route"] == "band":
        return band_edge_reference(c["I"], c["n"], c["f"], c["d"], c["B"], res)
    return edge_reference(c["I"], c["n"], c["f"], c["d"], res)


def is_the_case(G, c):
    assert G.stats()["band_block"] == c["B"], "the handle's block size is not the case's: the case does not reach its edge"
    assert G.direct_info()["closures"] == c["closures"], "the handle's closure count is not the case's"


def handle(c):
    G = capi.Graph(c["I"], c["QQ"], c["n"], c["f"], **c["opts"])
    try:
        is_the_case(G, c)
        G.set_rotations(c["Q"])
        G.set_weights(c["d"])
    except BaseException:
        G.close()
        raise
    return G


def both_queries(c):
    with handle(c) as G:
        r = G.rotation_variance(c["pairs"])
        e = G.edge_diagnostics()
        _, res = state_of(G)
    return r, e, res


# ---- 1. the band route ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.BAND)
def test_band_case(name):
    c = VC.CASE[name]
    assert c["B"] > 0 and c["nu"] > VC.DENSE_MAX and len(c["pairs"]) == (1025 if name in VC.MANY_PAIRS else 60)
    r, e, res = both_queries(c)
    var, pv, band = variance_reference(name)
    if c["closures"] and not c["live"]:
        np.testing.assert_array_equal(var, band)       # k = 0: the band-only reference
    check_variance(r, var, pv, c)
    if c["live"]:
        # closures only add information. (Against the BAND-ONLY reference, so within the tolerance of the comparison: far
        # from every closure the two sides differ by rounding alone.)
        assert np.all(r["var"][c["f"]:] <= band[c["f"]:] * (1 + RTOL))
    check_edges(e, edges_reference(c, res), c)
    assert r["scale"] == pytest.approx(scale_reference(c["I"], c["f"], c["d"], res, c["nu"]), rel=RTOL)


# ---- 2. the planner's limit: one closure more and the handle solves iteratively ------------------------------------------------
def test_one_closure_past_the_limit_is_a_pcg_handle():
    c = VC.CASE["lim_1025"]
    assert c["nfar"] == 1025 and VC.CASE["lim_1024"]["nfar"] == 1024
    with handle(c) as G:
        assert G.stats()["band_block"] == 0
        rv = G.rotation_variance(c["pairs"], allow_rc=(capi.ERR_UNSUPPORTED,))
        assert rv["rc"] == capi.ERR_UNSUPPORTED
        assert np.isnan(rv["var"]).all() and np.isnan(rv["pair_var"]).all() and np.isnan(rv["scale"])
        r = G.rotation_variance(c["pairs"], marginals=False)
        assert r["var"] is None and np.isfinite(r["scale"])
        e = G.edge_diagnostics(allow_rc=(capi.ERR_UNSUPPORTED,))
        assert e["rc"] == capi.ERR_UNSUPPORTED and untouched(e)
    _, pv, _ = variance_reference("lim_1025")
    check_variance(r, None, pv, c, rtol=RTOL_PCG)


# ---- 3. the dense route -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.DENSE)
def test_dense_case(name):
    c = VC.CASE[name]
    assert c["nu"] <= VC.DENSE_MAX
    if name == "d_2048_direct":
        assert c["B"] > 0            # (is_the_case holds the handle to it: a banded handle whose query runs dense)
    if name == "d_1":
        assert [1, 0] in c["pairs"].tolist()
    r, e, res = both_queries(c)
    var, pv, _ = variance_reference(name)
    check_variance(r, var, pv, c)
    check_edges(e, edges_reference(c, res), c)


# ---- 4. the device-pointer forms: bitwise the host-pointer call on the same handle ------------------------------------------
@pytest.mark.parametrize("name", ["b8_257", "b16_129", "d_64"])
def test_device_pointer_forms_are_bitwise_the_host_forms(name):
    c = VC.CASE[name]
    with TorchGraph(tidx(c["I"]), t64(c["QQ"]), c["n"], c["f"], **c["opts"]) as D:
        is_the_case(D, c)
        D.set_rotations(t64(c["Q"]))
        D.set_weights(t64(c["d"]))
        rh = D.rotation_variance(c["pairs"])          # the host-pointer form (capi.Graph's) ...
        rd = D.variance()                             # ... and irotavg_graph_rotation_variance_dev
        eh = D.host_edge_diagnostics()
        ed = D.edge_diagnostics()
        same(rd["var"], rh["var"])
        assert np.float64(rd["scale"]).view(np.uint64) == np.float64(rh["scale"]).view(np.uint64)
        for k in KEYS:
            same(ed[k], eh[k])
        assert np.float64(ed["scale"]).view(np.uint64) == np.float64(eh["scale"]).view(np.uint64)
    var, pv, _ = variance_reference(name)
    check_variance(rh, var, pv, c)                    # (this handle was planned on the device: bcr_plan_dev)


# ---- 5. deterministic and read-only --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b32_span", "b8_fixed3"])
def test_queries_repeat_bitwise_and_change_nothing(name):
    c = VC.CASE[name]
    with handle(c) as G:
        Q0, w0, s0 = G.get_rotations(), G.get_weights(), _stats_wo_time(G)
        np.testing.assert_array_equal(w0, c["d"])
        r1, e1 = G.rotation_variance(c["pairs"]), G.edge_diagnostics()
        r2, e2 = G.rotation_variance(c["pairs"]), G.edge_diagnostics()
        for k in ("var", "pair_var"):
            np.testing.assert_array_equal(r1[k].view(np.uint64), r2[k].view(np.uint64))
        for k in KEYS:
            np.testing.assert_array_equal(e1[k].view(np.uint64), e2[k].view(np.uint64))
        assert r1["scale"] == r2["scale"] == e1["scale"] == e2["scale"]
        np.testing.assert_array_equal(G.get_rotations(), Q0)
        np.testing.assert_array_equal(G.get_weights(), w0)
        assert _stats_wo_time(G) == s0
    print("%s: two calls of each query bitwise equal; rotations, weights and counters unchanged" % name)
