"""ONE linear solve x = L^-1 b of the banded direct solver (irotavg_amd/csrc/bcr.hip) against the references of
tests/band_cases.py (checked on the CPU by test_band_cases_cpu.py), on every route through its kernels.

Why a single solve. Every other test of this solver looks at converged IRLS rotations (an IRLS fixed point corrects a solve
that is wrong at 1e-7), at one solve at 1e-9 relative, at a residual of 1e-11, or at two forms of the same arithmetic being
bitwise equal. Here x is compared with a long-double banded Cholesky solve under

    ratio(X) = (max|X - x_ld| / max|x_ld|) / max(e_ref, nu 2^-52) < 16,
    e_ref = the larger error of LAPACK's float64 solve and of a float64 NumPy restatement of the kernel's own algorithm

(band_cases: the bar comes from the references alone), the level shape the handle reports (direct_info) is the one the
case is named for and is what the restatement is run with, and the handle's counters say which launches ran.

Per case: Graph(I, QQ, n, f, band_direct=1), set_rotations(Q0), edge_residual(), set_weights(w), X = ls_solve(). Asserted:
* direct_info(): block, (blocks, chunks, reduced) per level, no closures, fused_assembly = 1 exactly when a chunk's rows are
  whole slices (blocks of 8 / 16 / 24 / 32) and IROTAVG_BCR_NO_FUSED_ASM is not set. A mixed case on a device whose
  compute-unit count gives no mixed level FAILS with that message;
* stats(): direct_solves == 1, pcg_solves == 0, direct_up_fallbacks == 0, direct_guarded == 0. IROTAVG_BCR_UP_CAP=0 reports
  the same: bcr_pass asks bcr_up_reserve for a share of the device, gets none and launches the levels one by one -- a refused
  reservation is no fall-back (direct_up_fallbacks counts only a wait inside the single launch that gave up, bcr_up_failed);
* direct_dead_pivots == 0 on every case, the dead-pivot cases included: bcr_invert adds to the counter it is handed, and
  bcr_reduce_level hands one over only on a handle with closures (`far ? S.dead.p : nullptr`; the single-launch upper levels
  and the sixteen-block top pass none at all), and the statistic is written by run_irls alone, after a gate refused a step.
  On a closure-free handle a dead pivot is silent; what the case plants shows as X[row] == 0 exactly, asserted here, and as
  the restatement's own count (test_band_cases_cpu.py);
* X finite, ratio(X) < 16, direct_residual() <= 16 x the residual ||b - L x|| / ||b|| of x_bcr64 formed in long double;
* the switches IROTAVG_BCR_NO_FUSED_ASM and IROTAVG_BCR_UP_CAP=0 return the base case's X to the bit (the same arithmetic in
  other launches); all weights x 2^10 return the unscaled twin's X to the bit (a power of two passes exactly through
  v_rcp_f64 + two Newton steps and every product; the dead-pivot limit is relative to the block's own diagonal).

Measured on one MI355X (bar 16; the case names carry the route, the block size and the size, band_cases._cases):

    case                 route  levels (blocks)        ratio   e_ref     floor     residual  of x_bcr64
    one-b8-64-u          one    [8]                     0.33   6.56e-15  1.42e-14  1.03e-15  6.63e-16
    one-b8-63-u          one    [8]                     0.33   2.20e-15  1.40e-14  3.38e-16  4.48e-16
    one-b8-5-u           one    [1]                     3.10   3.65e-16  1.11e-15  3.41e-16  2.69e-16
    one-b8-64-s          one    [8]                     0.69   9.95e-14  1.42e-14  1.08e-14  9.02e-15
    one-b8-63-s          one    [8]                     1.03   5.01e-14  1.40e-14  1.71e-15  2.27e-15
    one-b8-5-s           one    [1]                     2.56   4.84e-16  1.11e-15  7.20e-16  6.05e-16
    one-b12-96-u         one    [8]                     0.28   3.14e-15  2.13e-14  4.25e-16  5.43e-16
    one-b12-95-u         one    [8]                     0.23   2.29e-15  2.11e-14  4.36e-16  3.74e-16
    one-b12-5-u          one    [1]                     6.46   2.37e-16  1.11e-15  2.69e-16  1.44e-16
    one-b16-128-u        one    [8]                     0.12   4.63e-15  2.84e-14  4.01e-16  4.26e-16
    one-b16-127-u        one    [8]                     0.17   7.86e-15  2.82e-14  5.28e-16  7.67e-16
    one-b16-5-u          one    [1]                     4.39   2.92e-16  1.11e-15  2.64e-16  3.67e-16
    one-b20-160-u        one    [8]                     0.10   6.08e-15  3.55e-14  6.10e-16  7.49e-16
    one-b20-159-u        one    [8]                     0.13   2.63e-15  3.53e-14  4.61e-16  4.59e-16
    one-b20-5-u          one    [1]                     5.89   4.77e-16  1.11e-15  3.73e-16  3.05e-16
    one-b24-192-u        one    [8]                     0.07   4.01e-15  4.26e-14  7.33e-16  5.58e-16
    one-b24-191-u        one    [8]                     0.25   7.37e-15  4.24e-14  9.18e-16  6.30e-16
    one-b24-5-u          one    [1]                     5.52   2.92e-16  1.11e-15  2.24e-16  3.39e-16
    one-b28-224-u        one    [8]                     0.07   3.84e-15  4.97e-14  6.64e-16  7.71e-16
    one-b28-223-u        one    [8]                     0.07   2.53e-15  4.95e-14  5.18e-16  4.63e-16
    one-b28-5-u          one    [1]                     2.74   2.01e-15  1.11e-15  1.02e-15  9.34e-16
    one-b32-256-u        one    [8]                     0.06   3.49e-15  5.68e-14  6.15e-16  5.77e-16
    one-b32-255-u        one    [8]                     0.10   4.93e-15  5.66e-14  5.80e-16  6.53e-16
    one-b32-5-u          one    [1]                     5.90   4.00e-16  1.11e-15  2.28e-16  2.21e-16
    one-b32-256-s        one    [8]                     0.27   5.63e-14  5.68e-14  2.47e-15  2.76e-15
    one-b32-255-s        one    [8]                     0.19   1.14e-14  5.66e-14  6.77e-16  5.53e-16
    one-b32-5-s          one    [1]                     1.16   4.99e-14  1.11e-15  1.19e-13  1.92e-13
    two-b8-nb9           two    [9, 2]                  0.36   3.82e-15  1.53e-14  4.13e-16  3.92e-16
    two-b8-nb16          two    [16, 2]                 0.26   8.59e-15  2.78e-14  4.21e-16  4.18e-16
    two-b8-nb17          two    [17, 3]                 0.19   1.11e-14  2.95e-14  6.40e-16  5.16e-16
    two-b8-nb64          two    [64, 8]                 0.31   4.32e-14  1.13e-13  8.21e-16  9.90e-16
    two-b16-nb9          two    [9, 2]                  0.13   3.51e-15  3.13e-14  4.42e-16  5.65e-16
    two-b16-nb16         two    [16, 2]                 0.21   1.46e-14  5.62e-14  7.25e-16  6.65e-16
    two-b16-nb17         two    [17, 3]                 0.12   8.92e-15  5.97e-14  8.59e-16  7.23e-16
    two-b16-nb64         two    [64, 8]                 0.12   6.52e-14  2.27e-13  8.35e-16  1.29e-15
    two-b24-nb9          two    [9, 2]                  0.14   4.65e-15  4.73e-14  8.32e-16  5.76e-16
    two-b24-nb16         two    [16, 2]                 0.16   2.23e-14  8.46e-14  5.55e-16  5.65e-16
    two-b24-nb17         two    [17, 3]                 0.06   9.83e-15  8.99e-14  6.51e-16  6.44e-16
    two-b24-nb64         two    [64, 8]                 0.07   1.16e-13  3.40e-13  6.18e-16  6.84e-16
    two-b28-nb9          two    [9, 2]                  0.08   2.16e-15  5.53e-14  6.36e-16  5.61e-16
    two-b28-nb64         two    [64, 8]                 0.10   8.28e-14  3.97e-13  7.61e-16  8.06e-16
    sep-b28-nb65         sep    [65, 9, 2]              0.15   7.88e-14  4.03e-13  1.02e-15  1.26e-15
    two-b32-nb9          two    [9, 2]                  0.06   7.30e-15  6.33e-14  9.56e-16  8.90e-16
    two-b32-nb64         two    [64, 8]                 0.06   4.54e-14  4.54e-13  6.96e-16  7.83e-16
    sep-b32-nb65         sep    [65, 9, 2]              0.02   8.30e-14  4.61e-13  1.48e-15  1.17e-15
    top16-b8-nb65        top16  [65, 9]                 0.31   1.05e-13  1.15e-13  1.12e-15  1.19e-15
    top16-b8-nb72        top16  [72, 9]                 0.68   7.33e-14  1.27e-13  9.88e-16  1.02e-15
    top16-b8-nb73        top16  [73, 10]                0.61   6.36e-14  1.29e-13  1.47e-15  1.68e-15
    top16-b8-nb121       top16  [121, 16]               0.71   1.67e-13  2.14e-13  1.80e-15  2.46e-15
    top16-b8-nb128       top16  [128, 16]               0.89   2.07e-13  2.27e-13  7.65e-16  6.90e-16
    top16-b12-nb65       top16  [65, 9]                 0.31   3.13e-14  1.73e-13  7.54e-16  1.06e-15
    top16-b12-nb72       top16  [72, 9]                 0.48   5.73e-14  1.91e-13  1.41e-15  2.10e-15
    top16-b12-nb73       top16  [73, 10]                0.23   5.14e-14  1.94e-13  7.72e-16  8.99e-16
    top16-b12-nb121      top16  [121, 16]               0.23   9.79e-14  3.22e-13  2.25e-15  2.23e-15
    top16-b12-nb128      top16  [128, 16]               0.49   2.81e-13  3.40e-13  1.12e-15  1.18e-15
    top16-b20-nb65       top16  [65, 9]                 0.09   6.61e-14  2.88e-13  1.11e-15  1.19e-15
    top16-b20-nb72       top16  [72, 9]                 0.17   5.00e-14  3.19e-13  1.17e-15  1.25e-15
    top16-b20-nb73       top16  [73, 10]                0.13   5.76e-14  3.24e-13  1.32e-15  1.42e-15
    top16-b20-nb121      top16  [121, 16]               0.17   1.32e-13  5.37e-13  2.03e-15  1.60e-15
    top16-b20-nb128      top16  [128, 16]               0.09   1.28e-13  5.68e-13  1.36e-15  7.88e-16
    top16-b24-nb65       top16  [65, 9]                 0.17   7.69e-14  3.46e-13  1.47e-15  1.81e-15
    top16-b24-nb72       top16  [72, 9]                 0.09   7.66e-14  3.83e-13  1.32e-15  1.05e-15
    top16-b24-nb73       top16  [73, 10]                0.24   3.47e-14  3.88e-13  1.25e-15  1.10e-15
    top16-b24-nb121      top16  [121, 16]               0.15   1.07e-13  6.44e-13  1.16e-15  1.37e-15
    top16-b24-nb128      top16  [128, 16]               0.10   1.11e-13  6.81e-13  1.17e-15  9.43e-16
    up-b8-nb129-u        up     [129, 17, 3]            0.80   2.34e-13  2.28e-13  1.80e-15  2.04e-15
    up-b8-nb129-s        up     [129, 17, 3]            0.13   1.33e-11  2.28e-13  6.57e-14  1.01e-13
    up-b8-nb1025-u       up     [1025, 129, 17, 3]      0.90   2.10e-12  1.82e-12  2.34e-15  2.52e-15
    up-b8-nb1025-s       up     [1025, 129, 17, 3]      0.26   2.19e-10  1.82e-12  7.08e-14  3.20e-14
    up-b24-nb129-u       up     [129, 17, 3]            0.10   1.49e-13  6.87e-13  1.75e-15  1.42e-15
    up-b24-nb129-s       up     [129, 17, 3]            0.72   5.94e-13  6.87e-13  2.86e-15  3.85e-15
    sep-b32-nb513        sep    [513, 65, 9, 2]         0.06   9.95e-13  3.64e-12  3.84e-15  3.13e-15
    mixed-b8             mixed  [4109, 525, 66, 9]      0.55   1.93e-11  7.30e-12  1.01e-14  1.97e-14
    mixed-b32            mixed  [2053, 261, 33, 5]      0.26   7.61e-12  1.46e-11  4.77e-15  5.30e-15
    switch-nofusedasm    switch [129, 17, 3]            0.13   1.33e-11  2.28e-13  6.57e-14  1.01e-13
    switch-notop16       switch [129, 17, 3]            0.13   1.33e-11  2.28e-13  6.76e-14  1.01e-13
    switch-upcap0        switch [129, 17, 3]            0.13   1.33e-11  2.28e-13  6.57e-14  1.01e-13
    switch-nomixed       switch [4109, 514, 65, 9]      0.55   1.93e-11  7.30e-12  1.21e-14  1.95e-14
    up-b16-nb129-s       up     [129, 17, 3]            0.69   1.47e-12  4.58e-13  6.38e-15  1.01e-14
    big-b8-nb129-s       big    [129, 17, 3]            0.13   1.33e-11  2.28e-13  6.57e-14  1.01e-13
    big-b16-nb129-s      big    [129, 17, 3]            0.69   1.47e-12  4.58e-13  6.38e-15  1.01e-14
    big-b24-nb129-s      big    [129, 17, 3]            0.72   5.94e-13  6.87e-13  2.86e-15  3.85e-15
    weak-b8-1025         weak   [129, 17, 3]            2.35   7.76e-04  2.28e-13  1.45e-05  1.04e-05
    dead-b8-row0         dead   [129, 17, 3]            0.62   2.38e-13  2.28e-13  1.67e-15  1.91e-15
    dead-b8-sep          dead   [129, 17, 3]            0.61   1.92e-13  2.28e-13  9.65e-16  1.01e-15
    dead-b8-last         dead   [129, 17, 3]            0.28   1.81e-13  2.28e-13  7.14e-16  6.62e-16

The largest ratios, 2.6 - 6.5, are the five-view cases, whose floor is 5 x 2^-52 while cond(L) is 10 - 14: at that size the
bar measures the right-hand side, not the solve. The device forms the residuals r itself (edge_residual: two quaternion
products and a log map, whose small vector part carries the ABSOLUTE rounding of numbers of size 1); noise of 2^-53 on r
alone moves numpy.linalg.solve to 1.8 - 2.4 on these cases. Next is the weak link, 2.35 at e_ref = 7.8e-4: the device
degrades no faster than the float64 references. Everywhere else the device is within the larger of nu 2^-52 and the
references' own error. The two switches that only move launches, and all three x 2^10 cases, returned their base case's X to
the bit; IROTAVG_BCR_NO_TOP16 and IROTAVG_BCR_NO_MIXED change the elimination order (ratio 0.13 and 0.55). No defect found:
nothing in bcr.hip changed.
"""
import numpy as np
import pytest

import band_cases as BC
from irotavg_amd import capi

pytestmark = pytest.mark.gpu

_X = {}          # case name -> X of its device solve (the twins and base cases of the bitwise comparisons)


def device_solve(c, monkeypatch):
    with monkeypatch.context() as mp:
        for k, v in c["env"].items():
            mp.setenv(k, v)                                    # (handle-scope switches, read at creation)
        with capi.Graph(c["I"], c["QQ"], c["n"], c["f"], band_direct=1) as G:
            G.set_rotations(c["Q0"])
            G.edge_residual()
            G.set_weights(c["w"])
            X = G.ls_solve()
            info, st = G.direct_info(), G.stats()
            res = G.direct_residual()
    _X[c["name"]] = X
    return X, info, st, res


def solution_of(name, monkeypatch):
    if name not in _X:
        device_solve(BC.CASE[name], monkeypatch)
    return _X[name]


@pytest.mark.parametrize("name", [c["name"] for c in BC.CASES])
def test_one_solve_matches_the_long_double_reference(name, monkeypatch):
    c = BC.CASE[name]
    X, info, st, res = device_solve(c, monkeypatch)
    levels = [(lv["blocks"], lv["chunks"], lv["reduced"]) for lv in info["levels"]]
    if c["route"] == "mixed":
        assert len(levels) > 1 and levels[1][2] < levels[1][0], \
            "no mixed level 1 on this device (the case is sized for 256 compute units): %s" % (levels,)
    assert info["block"] == c["B"] == st["band_block"], (info, c["B"])
    assert levels == c["levels"], (levels, c["levels"])
    assert info["closures"] == 0
    assert info["fused_assembly"] == (1 if c["B"] % 8 == 0 and "IROTAVG_BCR_NO_FUSED_ASM" not in c["env"] else 0), info
    ref = BC.references(c, block=info["block"], levels=levels, top16=c["top16"])
    r = BC.ratio(ref, X)
    print("band-solve %-20s %-6s levels %-22s ratio %6.2f  e_ref %.2e  floor %.2e  residual %.2e (x_bcr64 %.2e)"
          % (name, c["route"], [lv[0] for lv in levels], r, ref["e_ref"], ref["floor"], float(np.max(res)), ref["res_bcr64"]))
    assert st["direct_solves"] == 1 and st["pcg_solves"] == 0, st
    assert st["direct_up_fallbacks"] == 0 and st["direct_guarded"] == 0, st
    assert st["direct_dead_pivots"] == 0, st                   # (no closures: nobody counts, see the module docstring)
    assert np.isfinite(X).all()
    assert r < BC.BAR
    for row in c["isolated"]:
        assert np.all(X[row] == 0), (row, X[row])
    assert ref["ndead"] == len(c["isolated"])
    assert float(np.max(res)) <= 16.0 * ref["res_bcr64"]
    if c["twin"] is not None:
        np.testing.assert_array_equal(X, solution_of(c["twin"], monkeypatch))
    if c["system"] != name and ("IROTAVG_BCR_NO_FUSED_ASM" in c["env"] or "IROTAVG_BCR_UP_CAP" in c["env"]):
        np.testing.assert_array_equal(X, solution_of(c["system"], monkeypatch))
