"""The references of tests/band_cases.py checked against each other on the CPU -- what test_gpu_band_solve.py then holds the
banded direct solver (bcr.hip) to: the band-storage operator and Cholesky against their dense twins, the float64
restatement of the kernel's algorithm against LAPACK and the long-double solve on every case, the level shapes the cases are
named for, and what the bar of 16 can see: every mutant of the restatement is above it on the routes it concerns and changes
nothing on a route it cannot touch."""
import numpy as np
import pytest

import band_cases as BC
import pcg_cases as PC
from dense_cases import chol_solve_ld

LD = np.longdouble


def test_level_shapes_the_cases_are_named_for():
    shape = {c["name"]: ([lv[0] for lv in c["levels"]], c["top16"]) for c in BC.CASES}
    for c in BC.CASES:
        lev, nb0 = c["levels"], -(-c["nu"] // c["B"])
        assert lev[0][0] == nb0 and c["B"] == BC.block_size(c["bw"])
        if c["route"] == "one":
            assert len(lev) == 1 and nb0 <= 8 and not c["top16"]
        elif c["route"] == "two":
            assert len(lev) == 2 and 2 <= lev[1][0] <= 8 and c["top16"] == (c["B"] <= 24)
        elif c["route"] == "top16":
            assert len(lev) == 2 and 9 <= lev[1][0] <= 16 and c["top16"]
        elif c["route"] == "up":
            assert len(lev) in (3, 4) and c["B"] <= 24 and lev[1][1] <= 256 and c["top16"]     # bcr_wants_up
        elif c["route"] == "sep":
            assert len(lev) in (3, 4) and c["B"] >= 28 and not c["top16"]
        elif c["route"] == "mixed":
            assert len(lev) == 4 and lev[1][2] < lev[1][0] and lev[0][1] * 8 < nb0
    assert {c["B"] for c in BC.CASES if c["route"] == "one" and c["nu"] > 5} == {8, 12, 16, 20, 24, 28, 32}
    assert sorted(shape[n][0][1] for n in shape if n.startswith("top16-b8")) == [9, 9, 10, 16, 16]
    assert shape["up-b8-nb1025-u"] == ([1025, 129, 17, 3], True) and shape["sep-b32-nb513"] == ([513, 65, 9, 2], False)
    assert BC.CASE["mixed-b8"]["levels"] == [(4109, 512, 4109), (525, 66, 512), (66, 9, 66), (9, 2, 9)]
    assert BC.CASE["mixed-b32"]["levels"] == [(2053, 256, 2053), (261, 33, 256), (33, 5, 33), (5, 1, 5)]
    assert shape["switch-nomixed"] == ([4109, 514, 65, 9], True) and shape["switch-notop16"] == ([129, 17, 3], False)
    # the raw run of the B = 8 mixed level straddles a chunk boundary of level 1: blocks 512 ... 524, chunks 64 and 65
    assert 512 // 8 != 524 // 8
    for n in (2, 3, 8, 9, 10, 16):
        rounds, last = BC.top_schedule(n)
        done = [e[0] for r in rounds for e in r]
        assert sorted(done + [last]) == list(range(n)) and all(len(r) <= 4 for r in rounds)
    assert BC.top_schedule(10)[0][0] == [(0, -1, 1), (2, 1, 3), (4, 3, 5), (6, 5, 7)]


def test_band_operator_equals_the_dense_one():
    for name in ("two-b8-nb17", "dead-b8-sep", "one-b32-255-s"):
        c = BC.CASE[name]
        for dt in (np.float64, LD):
            L, b, _, _ = PC.operator(c, dt)
            S, bb = BC.band_operator(c, dt)
            Lb = BC.dense_from_band(S)
            tol = (2.0 ** -50 if dt is np.float64 else 2.0 ** -61) * np.abs(L).max()      # (the order of the sums differs)
            assert Lb.dtype == L.dtype and np.abs(Lb - L).max() <= tol
            assert np.abs(bb - b).max() <= (2.0 ** -50 if dt is np.float64 else 2.0 ** -61) * np.abs(b).max()
            np.testing.assert_array_equal(BC.dense_from_band(BC.band_from_dense(L, c["bw"])), L)
            X = np.asarray(np.random.default_rng(0).normal(size=(c["nu"], 3)), dtype=dt)
            assert np.abs(BC.band_matvec(S, X) - Lb @ X).max() <= 1e-13 * np.abs(Lb @ X).max()


def test_band_cholesky_equals_the_dense_one():
    """band_chol_solve against dense_cases.chol_solve_ld to 1e-17 relative, in long double."""
    for name in ("two-b8-nb17", "one-b32-255-s", "two-b16-nb17"):
        c = BC.CASE[name]
        L, b, _, _ = PC.operator(c, LD)
        Xd = chol_solve_ld(L, b, c["bw"])
        Xb = BC.band_chol_solve(BC.band_from_dense(L, c["bw"]), b)
        assert Xb.dtype == Xd.dtype == LD
        err = float(np.abs(Xb - Xd).max() / np.abs(Xd).max())
        print("band Cholesky %s: %.2e" % (name, err))
        assert err <= 1e-17


@pytest.mark.parametrize("name", [c["name"] for c in BC.CASES])
def test_references_agree_on_every_case(name):
    c = BC.CASE[name]
    ref = BC.references(c)
    print("band-ref %-20s nu %6d block %2d levels %s: e_lu %.2e e_bcr %.2e floor %.2e, residual of x_bcr64 %.2e, dead %d"
          % (name, c["nu"], c["B"], [lv[0] for lv in c["levels"]], ref["e_lu"], ref["e_bcr"], ref["floor"],
             ref["res_bcr64"], ref["ndead"]))
    assert np.isfinite(ref["x_ld"]).all() and np.isfinite(ref["x_bcr64"]).all()
    assert BC.ratio(ref, ref["x_lu64"]) <= 1.0 and BC.ratio(ref, ref["x_bcr64"]) <= 1.0
    # the restatement is as good as LAPACK: a plain float64 cyclic reduction measured 0.6 - 2.7 x the LU error
    assert ref["e_bcr"] <= 4.0 * max(ref["e_lu"], ref["floor"])
    # dead pivots: the planted rows and nothing else; their unknowns are exactly zero in every reference
    assert ref["ndead"] == len(c["isolated"]) and sorted(ref["dead"]) == sorted(c["isolated"])
    for x in (ref["x_ld"], ref["x_lu64"], ref["x_bcr64"]):
        assert np.all(x[list(c["isolated"])] == 0)
    if c["route"] == "weak":
        assert ref["e_ref"] > 1e4 * ref["floor"]               # the family is there for its conditioning


def test_large_pivot_cases_scale_their_twins_exactly():
    """All weights x 2^10: the float64 restatement returns the twin's solution to the bit (powers of two pass exactly
    through reciprocals and products, the dead-pivot limit is relative) -- what the GPU test asks of the kernel."""
    for c in BC.CASES:
        if c["route"] == "big":
            t = BC.CASE[c["twin"]]
            np.testing.assert_array_equal(c["w"], 1024.0 * t["w"])
            np.testing.assert_array_equal(BC.references(c)["x_bcr64"], BC.references(t)["x_bcr64"])
            assert BC.operator(c, np.float64)[0].max() > 1e11


def test_restatement_on_other_level_shapes():
    """Any level shape is the same solve: mixed levels and sixteen-block tops on small systems (shapes a device with two
    or four compute units would have), under the same bar as the references."""
    for name, ncu, kw in (("top16-b8-nb65", 2, {}), ("top16-b8-nb72", 2, {}), ("up-b8-nb129-s", 2, {}), ("sep-b32-nb65", 4, {}),
                          ("up-b24-nb129-u", 8, {}), ("dead-b8-last", 2, {}), ("top16-b24-nb121", 4, dict(no_top16=True))):
        c = BC.CASE[name]
        lev, top16 = BC.expected_levels(c["nu"], c["B"], ncu=ncu, **kw)
        if not kw:
            assert lev[1][2] < lev[1][0], (name, lev)                          # mixed
        ref = BC.references(c)
        S, b = BC.operator(c, np.float64)
        r = BC.ratio(ref, BC.bcr_solve64(S, b, c["B"], lev, top16))
        print("band-shape %s %s: ratio %.2f" % (name, lev, r))
        assert r < 4.0


# mutant -> (cases where it must be above the bar, cases it cannot touch)
SEEN = {
    "fill_dropped": (("two-b8-nb17", "top16-b8-nb73", "sep-b32-nb65", "mixed-b8"), ("one-b8-64-u", "one-b32-255-s")),
    "fill_scaled": (("two-b8-nb17", "top16-b8-nb73", "up-b24-nb129-s", "sep-b32-nb65"), ("one-b32-256-s",)),
    "pivot_row_formula": (("one-b32-256-s", "up-b8-nb129-s", "up-b24-nb129-s", "big-b8-nb129-s", "big-b24-nb129-s"), ()),
    "short_block_rhs": (("one-b8-63-u", "two-b16-nb64", "two-b32-nb64"), ("one-b8-64-u", "up-b8-nb129-u", "top16-b8-nb73")),
    "seam_neighbour": (("two-b8-nb9", "top16-b24-nb121", "sep-b32-nb65", "up-b8-nb129-u"), ("one-b8-63-u",)),
    "mixed_offset": (("mixed-b8",), ("two-b16-nb64", "up-b8-nb129-u")),
    "top_order": (("two-b16-nb64", "top16-b8-nb73", "top16-b24-nb121", "mixed-b8"),
                  ("one-b8-64-u", "sep-b32-nb65", "switch-notop16")),
    "dead_unclamped": (("dead-b8-row0", "dead-b8-sep", "dead-b8-last"), ("up-b8-nb129-u",)),
}


@pytest.mark.parametrize("mutant", BC.MUTANTS)
def test_the_bar_sees_every_mutant(mutant):
    seen, inert = SEEN[mutant]
    for name in seen:
        c = BC.CASE[name]
        r = BC.ratio(BC.references(c), BC.restated(c, mutant))
        print("band-mutant %s on %s: ratio %.3g" % (mutant, name, r))
        assert not r < BC.BAR                                  # (above the bar, or not a number)
    for name in inert:
        c = BC.CASE[name]
        ref = BC.references(c)
        x = BC.restated(c, mutant)
        np.testing.assert_array_equal(x, ref["x_bcr64"])
        assert BC.ratio(ref, x) <= 1.0


def test_mixed_offset_on_a_small_mixed_shape():
    c = BC.CASE["top16-b8-nb72"]
    lev, top16 = BC.expected_levels(c["nu"], c["B"], ncu=2)
    assert lev[1][2] < lev[1][0]
    S, b = BC.operator(c, np.float64)
    r = BC.ratio(BC.references(c), BC.bcr_solve64(S, b, c["B"], lev, top16, mutant="mixed_offset"))
    assert not r < BC.BAR
