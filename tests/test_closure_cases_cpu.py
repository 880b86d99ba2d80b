"""The references of tests/closure_cases.py checked against each other on the CPU -- what test_gpu_closure_solve.py then holds
the closure half of the banded direct solver (bcr.hip: bcr_solve_t) to: the classification of the extra edges and the level
shapes the cases are named for, the operator's parts against the whole operator, the long-double Woodbury reference
against the dense long-double Cholesky, the float64 Woodbury formula against LAPACK and the long-double solve on every
case, and what the bar of 16 can see: every mutant of the formula is above it on a named case."""
import numpy as np
import pytest

import band_cases as BC
import closure_cases as CC
import pcg_cases as PC
from dense_cases import chol_solve_ld

LD = np.longdouble


def blocks(c):
    return [lv[0] for lv in c["levels"]]


def test_cases_are_what_they_are_named_for():
    for c in CC.CASES:
        far = CC.classify(c["extra"], c["B"])
        assert int(far.sum()) == c["closures"] == int(c["far"].sum()), c["name"]
        assert c["B"] == BC.block_size(c["bw"]) and c["levels"][0][0] == -(-c["nu"] // c["B"])
        if c["closures"]:
            assert c["levels"] == BC.expected_levels(c["nu"], c["B"], no_top16=True)[0] and not c["top16"] and c["fused"] == 0
        # the band edges are make_case's: span <= bw, the span-1 edge of every view, three dropped edges onto fixed views
        ij = c["I"][:c["ext0"]].astype(np.int64) - c["f"]
        free = (ij[:, 0] >= 0) & (ij[:, 1] >= 0)
        assert np.abs(ij[free, 0] - ij[free, 1]).max() == c["bw"] <= 32
        assert int(((ij[:, 0] >= 0) & (ij[:, 1] < 0)).sum()) == 3 + (1 if c["anchor_late"] else 0)
    C = CC.CASE
    assert blocks(C["one-b8"]) == [8] and blocks(C["one-b8-61"]) == [8] and 60 in C["one-b8-61"]["extra"]
    assert C["one-b8"]["extra"].tolist() == [[3, 44], [60, 10], [0, 63]]
    for B in (8, 16, 24, 32):
        c = C["two-b%d-nb9" % B]
        assert blocks(c) == [9, 2] and c["closures"] == 7 and c["nu"] == 9 * B - 3
        blk = c["extra"] // B
        assert 8 in blk and 7 in blk and [0, c["nu"] - 1] in c["extra"].tolist()
        assert any(a // 8 == b // 8 and abs(a - b) >= 2 for a, b in blk.tolist())
    assert {c["B"] for c in CC.CASES if c["name"].startswith("up-b")} == {8, 12, 16, 20, 24, 28, 32}
    for c in CC.CASES:
        if c["name"].startswith("up-b") or c["name"] == "b24-s":
            B, nb0 = c["B"], c["levels"][0][0]
            assert len(c["levels"]) == 3 and c["closures"] == 30 and len({frozenset(e) for e in c["extra"].tolist()}) == 30
            chunk = c["extra"] // (8 * B)
            blk = c["extra"] // B
            assert any(a == b for a, b in chunk.tolist()) and any(abs(a - b) == 1 for a, b in chunk.tolist())
            assert 0 in chunk and nb0 // 8 in chunk and 7 in blk % 8 and [0, c["nu"] - 1] in c["extra"].tolist()
    assert blocks(C["up-b8-nb129"]) == [129, 17, 3] and blocks(C["up-b24-nb65"]) == [65, 9, 2]
    m = C["mixed-b8"]
    assert m["levels"] == [(4109, 512, 4109), (525, 66, 512), (66, 9, 66), (9, 2, 9), (2, 1, 2)] and m["closures"] == 6
    raw = m["extra"] >= 32768
    assert raw.all(1).sum() >= 2 and (raw.any(1) & ~raw.all(1)).sum() >= 2                    # raw - raw, raw - reduced
    assert any(max(e) // 64 == 511 and min(e) // 64 == 0 for e in m["extra"].tolist())       # the last reduced chunk -> the first
    for r in (8, 96, 97, 192, 193, 400, 401, 1024, 1025):
        c = C["count-r%d" % r]
        assert c["closures"] == r and c["nu"] == 1029 and blocks(c) == [129, 17, 3] and c["direct"] == (r <= 1024)
        assert len({frozenset(e) for e in c["extra"].tolist()}) == r
    for r in (256, 257):
        assert C["count-b32-r%d" % r]["closures"] == r and C["count-b32-r%d" % r]["B"] == 32
    for name in ("tiles-count-r8", "tiles-up-b8-nb129", "tiles-count-r96"):
        c, b = C[name], C[C[name]["system"]]
        assert c["env"] == {"IROTAVG_BCR_S_TILES": "1"} and c["closures"] in (8, 30, 96)
        for k in ("I", "QQ", "Q0", "w"):
            np.testing.assert_array_equal(c[k], b[k])
    d = C["dead"]
    wd = d["w"][d["ext0"]:]
    assert d["closures"] == 12 and int((wd == 0).sum()) == 4 and wd[11] == 0 and wd[0] > 0
    assert d["extra"][11].tolist() == d["extra"][0].tolist()[::-1]
    d = C["dup"]
    same = [k for k, e in enumerate(d["extra"].tolist()) if sorted(e) == [200, 700]]
    assert len(same) == 3 and len(set(d["w"][d["ext0"] + np.array(same)])) == 3 and [700, 200] in d["extra"].tolist()
    assert C["star"]["closures"] == 16 and all(517 in e for e in C["star"]["extra"].tolist())
    assert C["spread"]["fam"] == "s" and C["spread"]["closures"] == 30 and C["b24-s"]["fam"] == "s"
    w = C["spread"]["w"][C["spread"]["ext0"]:]
    assert w.min() < 1e-2 and w.max() > 1e2
    c = C["cancel"]
    link = (c["I"][:, 0] == c["f"] + 599) & (c["I"][:, 1] == c["f"] + 600)
    assert link.sum() == 1 and c["w"][link][0] == 1e-3 and c["extra"].tolist() == [[100, 900], [590, 640]]
    assert c["w"][c["ext0"]:].tolist() == [1.0, 2.0]
    ij = c["I"][:c["ext0"]].astype(np.int64) - c["f"]
    assert int(((ij[:, 0] < 600) & (ij[:, 0] >= 0) & (ij[:, 1] >= 600)).sum()) == 1           # the one link
    # wide in-band edges: more than 32 views, neighbouring blocks; no closure among them
    c = C["wide-b32"]
    assert c["closures"] == 0 and c["bwb"] == 62 and c["fused"] == 1 and (c["levels"], c["top16"]) == BC.expected_levels(541, 32)
    assert C["wide-b32-cl"]["closures"] == 1 and C["wide-b24-cl"]["closures"] == 1 and C["wide-b24-cl"]["B"] == 24
    for name in ("wide-b32", "wide-b32-cl", "wide-b24-cl"):
        c = C[name]
        wide = c["extra"][~c["far"]]
        assert len(wide) >= 2 and np.all(np.abs(wide[:, 0] - wide[:, 1]) > 32)
        assert np.all(np.abs(wide[:, 0] // c["B"] - wide[:, 1] // c["B"]) == 1)


def test_anchor_late_fails_the_cheap_rule_and_passes_the_exact_one():
    """bcr_plan's coverage rule (every row has a band edge to an earlier view or a kept edge from a fixed view) and the
    exact test behind it (bcr_band_part_anchored: union-find over the edges that are not closures), restated."""
    def rules(c):
        nu, f, B = c["nu"], c["f"], c["B"]
        ij = c["I"].astype(np.int64) - f
        ok = np.zeros(nu, dtype=bool)
        parent = list(range(nu))
        anch = np.zeros(nu, dtype=bool)

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x
        for i, j in ij.tolist():
            if i >= 0 and j >= 0:
                if i != j and abs(i - j) <= 32:
                    ok[max(i, j)] = True
                if i != j and not (abs(i - j) > 32 and abs(i // B - j // B) >= 2):
                    a, b = find(i), find(j)
                    parent[max(a, b)] = min(a, b)
            elif i < 0 <= j:
                ok[j] = anch[j] = True
        roots = {find(r) for r in range(nu) if anch[r]}
        return ok, all(find(r) in roots for r in range(nu))
    c = CC.CASE["anchor-late"]
    ok, exact = rules(c)
    assert np.nonzero(~ok)[0].tolist() == [0] and exact
    f = c["f"]
    assert not np.any((c["I"][:, 0] < f) & (c["I"][:, 1] == f))
    assert [f, 0] in c["I"].tolist() and [f - 1, f + 1] in c["I"].tolist() and c["closures"] == 30
    ok, exact = rules(CC.CASE["up-b8-nb129"])
    assert ok.all() and exact


def _band_storage_parts(monkeypatch, case, dtype):
    """parts() as the large systems get them: band storage, the closures' share of b added by hand."""
    with monkeypatch.context() as mp:
        mp.setattr(CC, "DENSE_MAX", 0)
        mp.setattr(CC, "DENSE64", 0)
        CC._parts.cache_clear()
        out = CC.parts(case, dtype)
    CC._parts.cache_clear()
    return out


def test_parts_add_up_to_the_whole_operator(monkeypatch):
    """A_b + V C V' = L and the right-hand side, in both storages and both precisions (to the order of the sums)."""
    for name in ("two-b8-nb9", "dead", "wide-b32-cl", "anchor-late"):
        c = CC.CASE[name]
        for dt in (np.float64, LD):
            tol = 2.0 ** -50 if dt is np.float64 else 2.0 ** -61
            L, b, _, _ = PC.operator(c, dt)
            _, ci, cj, w2 = CC.closure_rows(c, dt)
            V = CC.incidence(c["nu"], ci, cj, dt)
            for S, bb, Lp in (CC.parts(c, dt), _band_storage_parts(monkeypatch, c, dt)):
                assert S.dtype == L.dtype and S.shape[1] == 2 * c["bwb"] + 1
                assert np.abs(BC.dense_from_band(S) + (V * w2) @ V.T - L).max() <= tol * np.abs(L).max()
                assert np.abs(bb - b).max() <= tol * np.abs(b).max()
                assert Lp is None or np.array_equal(Lp, L)
            if dt is LD:
                X = np.asarray(np.random.default_rng(0).normal(size=(c["nu"], 3)), dtype=LD)
                assert np.abs(CC.full_matvec(c, X) - L @ X).max() <= 1e-17 * np.abs(L @ X).max()


def _fraction(v):
    """A long double as an exact rational (its 64-bit significand in two float64 pieces)."""
    from fractions import Fraction
    hi = float(v)
    return Fraction(hi) + Fraction(float(v - LD(hi)))


def test_twofold_residual_against_exact_rational_arithmetic(monkeypatch):
    """residual_twofold(b - L x in error-free transformations) against the same residual in exact rational arithmetic, at a
    random x and at the refined solution, where the residual is all cancellation."""
    c = CC.CASE["two-b8-nb9"]
    nu = c["nu"]
    with monkeypatch.context() as mp:
        mp.setattr(CC, "DENSE_MAX", 0)
        CC._parts.cache_clear()
        S, b, _ = CC.parts(c, LD)
        bw = S.shape[1] // 2
        _, ci, cj, w2 = CC.closure_rows(c, LD)
        for X in (np.asarray(np.random.default_rng(1).normal(size=(nu, 3)), dtype=LD), CC.woodbury_ld(c)[0]):
            r2 = CC.residual_twofold(c, X)
            for col in range(3):
                x = [_fraction(v) for v in X[:, col]]
                ex = [_fraction(v) for v in b[:, col]]
                mag = [abs(v) for v in ex]
                for row in range(nu):
                    for d in range(2 * bw + 1):
                        k = row + d - bw
                        if 0 <= k < nu and S[row, d] != 0:
                            t = _fraction(S[row, d]) * x[k]
                            ex[row] -= t
                            mag[row] += abs(t)
                for i, j, wq in zip(ci, cj, w2):
                    t = _fraction(wq) * (x[j] - x[i])
                    ex[j] -= t
                    ex[i] += t
                    mag[i] += abs(t)
                    mag[j] += abs(t)
                for row in range(nu):
                    assert abs(_fraction(r2[row, col]) - ex[row]) <= abs(ex[row]) / 2 ** 62 + mag[row] / 2 ** 120
    CC._parts.cache_clear()


def test_long_double_woodbury_equals_the_dense_cholesky(monkeypatch):
    """woodbury_ld (the reference of the systems above DENSE_MAX rows) against dense_cases.chol_solve_ld to 1e-17 relative, on
    systems small enough for the dense solve (refined on residuals in plain long double) to be that good itself: at 1029
    rows (`dup`) the two differ by 4e-17."""
    for name in ("two-b16-nb9", "two-b32-nb9", "wide-b24-cl"):
        c = CC.CASE[name]
        L, b, _, _ = PC.operator(c, LD)
        Xd = chol_solve_ld(L, b)
        with monkeypatch.context() as mp:
            mp.setattr(CC, "DENSE_MAX", 0)
            CC._parts.cache_clear()
            Xw, steps = CC.woodbury_ld(c)
        CC._parts.cache_clear()
        err = float(np.abs(Xw - Xd).max() / np.abs(Xd).max())
        print("long-double Woodbury %s: %.2e in %d steps" % (name, err, steps))
        assert Xw.dtype == LD and 1 <= steps <= 3 and err <= 1e-17


@pytest.mark.parametrize("name", CC.SOLVED)
def test_references_agree_on_every_case(name):
    c = CC.CASE[name]
    ref = CC.references(c)
    print("closure-ref %-18s nu %5d block %2d levels %-20s r %4d: e_lu %.2e e_wb %.2e floor %.2e, residuals %.2e %.2e, steps %d"
          % (name, c["nu"], c["B"], blocks(c), c["closures"], ref["e_lu"], ref["e_wb"], ref["floor"], ref["res_lu64"],
             ref["res_wb64"], ref["steps"]))
    assert np.isfinite(ref["x_ld"]).all() and np.isfinite(ref["x_wb64"]).all() and np.isfinite(ref["x_lu64"]).all()
    assert CC.ratio(ref, ref["x_lu64"]) <= 1.0 and CC.ratio(ref, ref["x_wb64"]) <= 1.0
    assert ref["ndead"] == 0                                   # bcr_solve64 meets no dead pivot in A_b
    assert ref["steps"] <= 3
    if name == "cancel":
        # A_b hangs on the weak link: Y = A_b^-1 b is far larger than the solution and the formula loses those digits
        assert 1e-11 < ref["e_wb"] < 1e-7
    else:
        # the formula's own cancellation does not loosen the bar
        assert ref["e_wb"] <= 8.0 * max(ref["e_lu"], ref["floor"])


# mutant -> the cases where it must be above the bar
SEEN = {
    "lambda_sign": ("one-b8", "up-b8-nb129", "count-r97", "wide-b24-cl"),
    "cinv_dropped": ("one-b8", "two-b24-nb9", "up-b16-nb65", "spread"),
    "dead_as_unit": ("dead",),
    "endpoint_off_by_one": ("one-b8-61", "two-b8-nb9", "up-b12-nb65", "star"),
    "dup_once": ("dup",),
    "wide_dropped": ("wide-b32", "wide-b32-cl", "wide-b24-cl"),
    "wide_as_far_only": ("wide-b32", "wide-b32-cl", "wide-b24-cl"),
}


@pytest.mark.parametrize("mutant", CC.MUTANTS)
def test_the_bar_sees_every_mutant(mutant):
    for name in SEEN[mutant]:
        c = CC.CASE[name]
        r = CC.ratio(CC.references(c), CC.woodbury64(c, mutant=mutant))
        print("closure-mutant %s on %s: ratio %.3g" % (mutant, name, r))
        assert not r < CC.BAR                                  # (above the bar, or not a number)
    # a mutant that cannot touch a case changes nothing there
    for name, inert in (("up-b8-nb129", ("dead_as_unit", "dup_once")), ("wide-b32", ("lambda_sign", "cinv_dropped", "dup_once"))):
        if mutant in inert:
            c = CC.CASE[name]
            np.testing.assert_array_equal(CC.woodbury64(c, mutant=mutant), CC.references(c)["x_wb64"])
