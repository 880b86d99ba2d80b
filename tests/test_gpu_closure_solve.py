"""ONE linear solve of the banded direct solver WITH LOOP CLOSURES (irotavg_amd/csrc/bcr.hip, bcr_solve_t: the two split passes
of the reduction around k_bcr_closure_forward / _forward_wave, k_bcr_closure_S / _S_pairs, k_bcr_closure_solve_lds or
dense_invert_spd + k_bcr_closure_lambda, k_bcr_closure_correct, on the step programs of bcr_closure_plan) against the
references of tests/closure_cases.py (checked on the CPU by test_closure_cases_cpu.py). test_gpu_band_solve.py is the same
for the closure-free half and asserts closures == 0 first.

Why a single solve, and why ls_solve. Everything else that looks at a closure solve sits behind k_bcr_gate: in irls a closure
solve whose residual is above max(pcg_rtol, 1e-12) is redone by conjugate gradients on the true operator, one counter
(direct_guarded) goes up and the converged rotations are the same. ls_solve runs no gate: bcr_solve, then g.X is copied
out. Here that raw X is compared with a long-double solve of the whole operator under

    ratio(X) = (max|X - x_ld| / max|x_ld|) / max(e_ref, nu 2^-52) < 16,
    e_ref = the larger error of numpy.linalg.solve on the dense operator and of the Woodbury formula in float64 around a
            NumPy restatement of the kernel's reduction (closure_cases: the bar comes from the references alone).

Per case: Graph(I, QQ, n, f, band_direct=1), set_rotations(Q0), edge_residual(), set_weights(w), X = ls_solve(). Asserted:
* direct_info(): block, (blocks, chunks, reduced) per level, closures, fused_assembly as the case expects -- with closures no
  sixteen-block top and no fused assembly; a WIDE IN-BAND edge (more than 32 views, neighbouring blocks) is no closure:
  `wide-b32` reports closures == 0, the ordinary level shape and fused_assembly == 1. 1025 closures on 1029 views:
  block == 0, the whole assertion. The mixed case on a device whose compute-unit count gives no mixed level FAILS with that
  message;
* stats(): direct_solves == 1, pcg_solves == 0, direct_guarded == 0, direct_up_fallbacks == 0, direct_dead_pivots == 0;
* X finite, ratio(X) < 16, max(direct_residual()) <= 16 x the larger residual ||b - L x|| / ||b|| of x_lu64 and x_wb64
  formed in long double;
* then, on the same handle, irls(4, 5 deg, 3, 1e-6): direct_guarded == 0 and pcg_iters == 0 -- the raw solves passed the gate
  and nothing was repaired. Not on `spread` and `b24-s` (weights over six decades: the gate's limit of 1e-12 is below what
  float64 gives there) and not on `cancel`, where the call must return OK or ERR_SOLVER and leave finite rotations;
* IROTAVG_BCR_S_TILES=1 (the tile kernel at every closure count) adds the same entries in another order: compared with the
  references, not bitwise.

The device-array plan (TestDevicePlan): a TorchGraph built from device arrays reports the same direct_info() as the
host-pointer handle and returns the same X to the bit -- k_plan_far collects the closures in any order, the host sorts them by
edge id. `anchor-late` is a sequence with closures whose first free view is tied through LATER views only: bcr_plan's cheap
coverage rule fails on it and the exact union-find test passes.

Measured on one MI355X (bar 16; route = the family of closure_cases._cases; residual = max(direct_residual()), references =
the larger long-double-formed residual of x_lu64 and x_wb64; guarded = direct_guarded after the irls call on the same handle):

    case               route   levels (blocks)           r   ratio  e_ref     floor     residual  references  guarded (irls)
    one-b8             shape   [8]                       3   0.43  6.84e-15  1.42e-14  6.99e-16  6.43e-16    0
    one-b8-61          shape   [8]                       3   0.57  3.08e-15  1.35e-14  4.72e-16  5.42e-16    0
    two-b8-nb9         shape   [9, 2]                    7   0.37  5.37e-15  1.53e-14  8.70e-16  7.41e-16    0
    two-b16-nb9        shape   [9, 2]                    7   0.13  2.06e-15  3.13e-14  5.03e-16  4.83e-16    0
    two-b24-nb9        shape   [9, 2]                    7   0.15  1.41e-14  4.73e-14  9.58e-16  7.90e-16    0
    two-b32-nb9        shape   [9, 2]                    7   0.05  4.01e-15  6.33e-14  7.43e-16  7.41e-16    0
    up-b8-nb129        shape   [129, 17, 3]             30   0.12  2.43e-14  2.28e-13  1.07e-15  2.63e-15    0
    up-b12-nb65        shape   [65, 9, 2]               30   0.09  1.56e-14  1.73e-13  7.41e-16  1.33e-15    0
    up-b16-nb65        shape   [65, 9, 2]               30   0.09  2.49e-14  2.30e-13  9.71e-16  1.12e-15    0
    up-b20-nb65        shape   [65, 9, 2]               30   0.07  2.33e-14  2.88e-13  1.20e-15  1.26e-15    0
    up-b24-nb65        shape   [65, 9, 2]               30   0.09  2.87e-14  3.46e-13  1.77e-15  1.83e-15    0
    up-b28-nb65        shape   [65, 9, 2]               30   0.11  3.95e-14  4.03e-13  1.32e-15  1.14e-15    0
    up-b32-nb65        shape   [65, 9, 2]               30   0.03  3.21e-14  4.61e-13  1.47e-15  1.03e-15    0
    mixed-b8           mixed   [4109, 525, 66, 9, 2]     6   0.34  3.28e-12  7.30e-12  5.59e-15  1.78e-13    0
    count-r8           count   [129, 17, 3]              8   0.28  5.65e-14  2.28e-13  1.40e-15  1.72e-15    0
    count-r96          count   [129, 17, 3]             96   0.06  2.43e-14  2.28e-13  2.26e-15  5.55e-15    0
    count-r97          count   [129, 17, 3]             97   0.13  3.27e-14  2.28e-13  2.09e-15  5.57e-15    0
    count-r192         count   [129, 17, 3]            192   0.57  2.06e-14  2.28e-13  1.22e-14  1.16e-14    0
    count-r193         count   [129, 17, 3]            193   0.25  1.99e-14  2.28e-13  6.13e-15  6.87e-15    0
    count-r400         count   [129, 17, 3]            400   0.33  5.46e-14  2.28e-13  9.89e-15  3.39e-14    0
    count-r401         count   [129, 17, 3]            401   0.90  7.95e-14  2.28e-13  2.98e-14  3.61e-14    0
    count-r1024        count   [129, 17, 3]           1024   1.44  9.96e-14  2.28e-13  1.04e-13  7.33e-14    0
    count-b32-r256     count   [35, 5]                 256   0.05  1.42e-14  2.48e-13  1.04e-15  9.73e-16    0
    count-b32-r257     count   [35, 5]                 257   0.05  1.71e-14  2.48e-13  8.96e-16  1.12e-15    0
    tiles-count-r8     switch  [129, 17, 3]              8   0.28  5.65e-14  2.28e-13  1.32e-15  1.72e-15    0
    tiles-up-b8-nb129  switch  [129, 17, 3]             30   0.12  2.43e-14  2.28e-13  1.02e-15  2.63e-15    0
    tiles-count-r96    switch  [129, 17, 3]             96   0.09  2.43e-14  2.28e-13  2.00e-15  5.55e-15    0
    dead               weights [129, 17, 3]             12   0.27  7.88e-14  2.28e-13  1.75e-15  1.86e-15    0
    dup                weights [129, 17, 3]              8   0.37  1.06e-13  2.28e-13  1.52e-15  2.03e-15    0
    star               weights [129, 17, 3]             16   0.19  4.34e-14  2.28e-13  1.13e-15  1.67e-15    0
    spread             weights [129, 17, 3]             30   0.90  3.75e-12  2.28e-13  2.37e-14  5.17e-14    0
    b24-s              weights [65, 9, 2]               30   0.21  4.96e-14  3.46e-13  1.41e-15  3.65e-15    0
    cancel             cancel  [129, 17, 3]              2   1.10  2.29e-09  2.28e-13  3.36e-10  7.53e-10    0
    wide-b32           wide    [17, 3]                   0   0.13  2.45e-14  1.20e-13  1.18e-15  9.99e-16    0
    wide-b32-cl        wide    [17, 3]                   1   0.11  8.08e-15  1.20e-13  8.78e-16  8.63e-16    0
    wide-b24-cl        wide    [17, 3]                   1   0.14  1.67e-14  8.99e-14  8.15e-16  1.12e-15    0
    anchor-late        anchor  [129, 17, 3]             30   0.08  2.06e-14  2.28e-13  1.68e-15  3.19e-15    0
    count-r1025: block == 0 (the iterative solver), nothing else asserted.

The device-array handles (TestDevicePlan: two-b8-nb9, up-b8-nb129, wide-b32-cl, anchor-late) reported the host handle's
direct_info() and returned its X to the bit, so their rows are the ones above. The largest ratio is 1.44, at 1024 closures on
1029 views, where the Woodbury system is as large as the operator; `cancel` is at 1.10 of an e_ref of 2.3e-9 -- the device
degrades no faster than the formula in float64 -- and its irls call returned OK with no guarded solve. Everywhere else the
raw closure solve is within the larger of nu 2^-52 and the references' own error; no solve was repaired (direct_guarded 0,
`spread` and `b24-s` included). No defect found in the Woodbury kernels or the step programs. The wide in-band edges are
kept in the block tridiagonal operator by the plan, by bcr_gather_row and by the fused assembly's window alike (ratio 0.13,
fused_assembly 1). `anchor-late` was the one finding: bcr_plan_dev returned at the first uncovered row without the exact
test bcr_plan falls back to (such a sequence was solved directly from host pointers and iteratively from device arrays);
it now copies the edge list to the host in that rare case and decides by bcr_band_part_anchored as bcr_plan does.
"""
import numpy as np
import pytest

import closure_cases as CC
from irotavg_amd import capi
from test_gpu_device_api import TorchGraph, host_graph, same, t64, tidx   # (imports torch ahead of the library's first load)

pytestmark = pytest.mark.gpu

SIGMA = 5 * np.pi / 180
NO_GATE_CHECK = ("cancel", "spread", "b24-s")


def device_solve(c, monkeypatch, make=None, put=np.asarray):
    """(X, direct_info, stats, direct_residual, what the irls call behind the solve left) of one handle."""
    with monkeypatch.context() as mp:
        for k, v in c["env"].items():
            mp.setenv(k, v)                                    # (handle-scope switches, read at creation)
        G = make() if make else capi.Graph(c["I"], c["QQ"], c["n"], c["f"], band_direct=1)
    with G:
        info = G.direct_info()
        if info["block"] == 0:
            return None, info, G.stats(), None, None
        G.set_rotations(put(c["Q0"]))
        G.edge_residual()
        G.set_weights(put(c["w"]))
        X = G.ls_solve()
        info, st = G.direct_info(), G.stats()
        res = G.direct_residual()
        out = G.irls(4, SIGMA, 3, 1e-6, allow_rc=(capi.ERR_SOLVER,) if c["name"] == "cancel" else ())
        after = dict(rc=out["rc"], stats=G.stats(), finite=bool(np.isfinite(G.get_rotations()).all()))
    return X, info, st, res, after


def check_solve(c, X, info, st, res, after, tag="closure-solve"):
    levels = [(lv["blocks"], lv["chunks"], lv["reduced"]) for lv in info["levels"]]
    if c["route"] == "mixed":
        assert len(levels) > 1 and levels[1][2] < levels[1][0], \
            "no mixed level 1 on this device (the case is sized for 256 compute units): %s" % (levels,)
    assert info["block"] == c["B"] == st["band_block"], (info, c["B"])
    assert levels == c["levels"], (levels, c["levels"])
    assert info["closures"] == c["closures"], info
    assert info["fused_assembly"] == c["fused"], info
    ref = CC.references(c, block=info["block"], levels=levels, top16=c["top16"])
    r = CC.ratio(ref, X)
    resref = max(ref["res_lu64"], ref["res_wb64"])
    print("%s %-18s %-7s levels %-20s r %4d ratio %6.2f  e_ref %.2e  floor %.2e  residual %.2e (references %.2e)  guarded %d"
          % (tag, c["name"], c["route"], [lv[0] for lv in levels], c["closures"], r, ref["e_ref"], ref["floor"],
             float(np.max(res)), resref, after["stats"]["direct_guarded"]))
    assert st["direct_solves"] == 1 and st["pcg_solves"] == 0, st
    assert st["direct_up_fallbacks"] == 0 and st["direct_guarded"] == 0 and st["direct_dead_pivots"] == 0, st
    assert np.isfinite(X).all()
    assert r < CC.BAR
    assert float(np.max(res)) <= 16.0 * resref
    if c["name"] == "cancel":
        assert after["rc"] in (capi.OK, capi.ERR_SOLVER) and after["finite"]
    elif c["name"] not in NO_GATE_CHECK:
        # the raw solves passed the gate: nothing was repaired
        assert after["rc"] == capi.OK and after["finite"]
        assert after["stats"]["direct_guarded"] == 0 and after["stats"]["pcg_iters"] == 0, after["stats"]
    return r


@pytest.mark.parametrize("name", [c["name"] for c in CC.CASES])
def test_one_closure_solve_matches_the_long_double_reference(name, monkeypatch):
    c = CC.CASE[name]
    X, info, st, res, after = device_solve(c, monkeypatch)
    if not c["direct"]:
        assert info["block"] == 0                              # more closures than a small graph keeps: the iterative solver
        return
    check_solve(c, X, info, st, res, after)


class TestDevicePlan:
    """bcr_plan_dev (edge list on the device) against bcr_plan (edge list on the host): the same decision, the same closures
    in the same order, the same X to the bit."""

    @pytest.mark.parametrize("name", ["two-b8-nb9", "up-b8-nb129", "wide-b32-cl", "anchor-late"])
    def test_device_plan_equals_host_plan(self, name, monkeypatch):
        c = CC.CASE[name]
        opts = dict(band_direct=1)
        H = device_solve(c, monkeypatch, make=lambda: host_graph(c["I"], c["QQ"], c["n"], c["f"], **opts))
        D = device_solve(c, monkeypatch, make=lambda: TorchGraph(tidx(c["I"]), t64(c["QQ"]), c["n"], c["f"], **opts), put=t64)
        assert H[1]["block"] == c["B"] and H[1]["closures"] == c["closures"], H[1]
        assert D[1] == H[1], (D[1], H[1])
        same(D[0], H[0])
        check_solve(c, *D, tag="closure-devplan")
