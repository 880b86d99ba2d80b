"""The cases of tests/variance_cases.py on the CPU -- what test_gpu_variance_edges.py then holds the variance query and the edge
diagnostics to: every case reaches the block size, block count, closure count and route its table row claims (by the planner's
rule restated in Python: this guards the generator, not the library); the block references (band_reference,
band_edge_reference) agree with the dense inverse on every band-route case small enough for one; and the comparison of the GPU
file, at the GPU file's tolerance, rejects a reference with one wrong index at a block edge.

Measured here, block reference against dense inverse, worst relative difference over marginals, pairs, edge_var, leverage
and chi2 of a case:
    b8_257 7.0e-13, b16_129 2.9e-14, b28_74 6.5e-14, b32_65 2.1e-14, b32_span 3.4e-14, b8_span33 2.4e-13, b8_fixed3 3.0e-14
(the blocks of 8 rows lose most: their recurrences are the longest). The bar is 1e-11: a margin of 14 at the worst case, and a
hundred times below the 1e-9 the device is held to. The three wrong references (on b8_257, b16_129 and b8_span33, the one case all three
can act on) are off by 4e-4 ... 0.99. No GPU."""
import numpy as np
import pytest

import test_edge_diagnostics_cpu as ED
import test_rotation_variance_cpu as RV
import variance_cases as VC
from test_gpu_variance_edges import RTOL, check_edges, check_variance, worst

REF_RTOL = 1e-11

# name: (B of the handle, blocks, closures, route of the queries) -- the table of the issue, twins and the k = 0 variant included
TABLE = {
    "b8_257": (8, 257, 0, "band"), "b8_511": (8, 511, 0, "band"), "b8_512": (8, 512, 0, "band"), "b8_513": (8, 513, 0, "band"),
    "b12_256": (12, 256, 5, "band"), "b12_256_k0": (12, 256, 5, "band"), "b16_129": (16, 129, 64, "band"),
    "b20_128": (20, 128, 63, "band"), "b20_128_k63": (20, 128, 63, "band"), "b24_128": (24, 128, 65, "band"),
    "b24_128_k65": (24, 128, 65, "band"), "b28_74": (28, 74, 1, "band"), "b32_65": (32, 65, 0, "band"),
    "b32_127": (32, 127, 0, "band"), "b32_128": (32, 128, 0, "band"), "b32_span": (32, 65, 30, "band"),
    "b8_span33": (8, 257, 10, "band"), "b8_fixed3": (8, 257, 0, "band"), "lim_1024": (12, 250, 1024, "band"),
    "lim_1024_k1024": (12, 250, 1024, "band"), "lim_1025": (0, 0, 0, "pcg"),
    "d_1": (0, 0, 0, "dense"), "d_2": (0, 0, 0, "dense"), "d_63": (0, 0, 0, "dense"), "d_64": (0, 0, 0, "dense"),
    "d_65": (0, 0, 0, "dense"), "d_2048": (0, 0, 0, "dense"), "d_2048_direct": (8, 256, 0, "dense"),
}
SIZES = {"b8_257": (2049, 1), "b8_511": (4088, 1), "b8_512": (4096, 1), "b8_513": (4097, 1), "b12_256": (3072, 1),
         "b16_129": (2064, 1), "b20_128": (2560, 2), "b24_128": (3072, 1), "b28_74": (2072, 1), "b32_65": (2049, 1),
         "b32_127": (4064, 1), "b32_128": (4096, 1), "b32_span": (2080, 1), "b8_span33": (2049, 1), "b8_fixed3": (2056, 3),
         "lim_1024": (3000, 1), "lim_1025": (3000, 1), "d_1": (1, 1), "d_2": (2, 1), "d_63": (63, 1), "d_64": (64, 1),
         "d_65": (65, 1), "d_2048": (2048, 1), "d_2048_direct": (2048, 1)}


# ---- 1. the generator ---------------------------------------------------------------------------------------------------------
def test_every_case_reaches_what_its_table_row_claims():
    assert set(TABLE) == set(VC.CASE)
    for name, c in VC.CASE.items():
        got = (c["B"], c["nb"], c["closures"], c["route"])
        assert got == TABLE[name], (name, got)
        assert got == tuple(c["claim"][k] for k in ("B", "nb", "closures", "route")), name
        P = VC.plan(c["I"], c["n"], c["f"], c["opts"].get("band_direct", 0))       # (from the finished edge list, once more)
        assert (P["B"], P["nb"], len(P["closures"]), P["route"]) == got
        if name in SIZES:
            assert (c["nu"], c["f"]) == SIZES[name]
        d = c["d"]
        assert d.shape == (len(c["I"]),) and np.all((d == 0) | ((d >= 0.1) & (d <= 3.0)))
        assert np.all(d[np.setdiff1d(np.arange(len(d)), c["far"])] > 0)             # only closures are ever dead
        assert c["I"].dtype == np.int32 and c["I"].min() >= 0 and c["I"].max() == c["n"] - 1
        np.testing.assert_allclose(np.linalg.norm(c["Q"], axis=1), 1.0, rtol=1e-14)
        if c["route"] != "dense":
            assert c["plan_band"] == c["band"] == (c["B"] or 12)                   # exactly B predecessors give that B
        assert len(c["pairs"]) == (1025 if name in VC.MANY_PAIRS else 12 if name in ("d_1", "d_2") else 60)
        assert VC.zero_pairs(c).sum() >= 2
    assert VC.BAND == [n for n in TABLE if TABLE[n][3] == "band"] and len(VC.DENSE) == 7


def test_the_edges_each_case_is_named_for():
    C = VC.CASE
    # block counts next to a power of two; the last block's padding; the 64-row tiles
    assert [C[n]["nb"] for n in ("b8_257", "b8_511", "b8_512", "b8_513", "b32_65", "b32_127", "b32_128")] == \
        [257, 511, 512, 513, 65, 127, 128]
    assert C["b8_257"]["nb"] * 8 - C["b8_257"]["nu"] == 7 and C["b8_513"]["nb"] * 8 - C["b8_513"]["nu"] == 7
    for n in ("b8_512", "b32_128"):
        assert C[n]["nu"] % C[n]["B"] == 0 and C[n]["nu"] % 64 == 0                # no pad row, no pad tile
    assert C["b8_511"]["nu"] % 8 == 0 and C["b8_511"]["nu"] % 64 != 0
    for n in ("b12_256", "b16_129", "b20_128", "b24_128", "b28_74", "b32_127"):
        assert C[n]["nu"] == C[n]["nb"] * C[n]["B"]                                # an exact fit of the last block
    assert 64 // 12 == 5 and 256 % 5 == 1 and 64 // 28 == 2 and 74 % 2 == 0       # windows of k_ed_wband: a short / a full last one
    assert {C[n]["B"] for n in VC.BAND} == {8, 12, 16, 20, 24, 28, 32}
    # closure counts: the columns of Z, the order of S
    live = {n: (C[n]["live"], C[n]["ldZ"]) for n in VC.BAND}
    assert live["b16_129"] == (64, 64) and live["b20_128_k63"] == (63, 64) and live["b24_128_k65"] == (65, 128)
    assert live["b20_128"] == (57, 64) and live["b24_128"] == (59, 64) and live["b28_74"] == (1, 64)
    assert live["lim_1024"] == (922, 960) and live["lim_1024_k1024"] == (1024, 1024)
    assert live["b12_256"] == (5, 64) and live["b12_256_k0"] == (0, 64) and C["b12_256_k0"]["closures"] == 5
    assert live["b32_span"] == (27, 64) and live["b8_span33"] == (9, 64)
    assert C["lim_1024"]["nfar"] == 1024 and C["lim_1025"]["nfar"] == 1025 and C["lim_1025"]["nu"] < 8192
    np.testing.assert_array_equal(C["b12_256"]["I"], C["b12_256_k0"]["I"])
    for n in VC.BAND:
        c = C[n]
        ij = c["I"][c["far"]].astype(np.int64) - c["f"]
        if n not in ("b32_span", "b8_span33"):
            assert np.all(np.abs(ij[:, 0] - ij[:, 1]) >= 2 * c["B"] + 64)
        assert len({frozenset(e) for e in ij.tolist()}) == len(ij)
        if len(ij) > 1:
            assert (ij[:, 0] > ij[:, 1]).any() and (ij[:, 0] < ij[:, 1]).any()     # both orientations
    # spans of 33 ... 63 views
    c = C["b32_span"]
    ij = c["I"][c["m_band"]:].astype(np.int64) - 1
    lo = ij.min(1)
    assert len(ij) == 60 and np.all(np.abs(ij[:, 0] - ij[:, 1]) == 40)
    assert int((lo % 32 < 24).sum()) == 30 and np.all((ij.max(1) // 32 - lo // 32 == 1) == (lo % 32 < 24))
    np.testing.assert_array_equal(np.sort(c["far"]) - c["m_band"], np.flatnonzero(lo % 32 >= 24))
    c = C["b8_span33"]
    ij = c["I"][c["far"]].astype(np.int64)
    assert len(ij) == 10 and np.all(np.abs(ij[:, 0] - ij[:, 1]) == 33)
    # boundary slots, the quirk, multiplicity
    c = C["b8_fixed3"]
    f = c["f"]
    X = c["I"][c["m_band"]:]
    for v in range(3):
        assert int(((X[:, 0] == v) & (X[:, 1] >= f)).sum()) == 2 and int(((X[:, 1] == v) & (X[:, 0] >= f)).sum()) == 2
    assert int(((X[:, 0] < f) & (X[:, 1] < f)).sum()) == 1 and int((X[:, 0] == X[:, 1]).sum()) == 1
    band = {tuple(e) for e in c["I"][:c["m_band"]].tolist()}
    free = X[(X[:, 0] >= f) & (X[:, 1] >= f) & (X[:, 0] != X[:, 1])]
    assert sum(tuple(e) in band for e in free.tolist()) == 20 and sum(tuple(e[::-1]) in band for e in free.tolist()) == 20
    assert C["b20_128"]["f"] == 2
    # the pairs
    for n, c in C.items():
        rows = c["pairs"].astype(np.int64) - c["f"]
        have = {tuple(p) for p in rows.tolist()}
        unit = c["B"] if c["route"] == "band" else 64
        assert (c["nu"] - 1, 0) in have and (0, min(unit, c["nu"]) - 1) in have
        assert ((c["nu"] - 1) // unit * unit, c["nu"] - 1) in have
        s = unit
        while s < c["nu"]:
            assert (s - 1, s) in have
            s *= 2
        ij = c["I"][c["far"]].astype(np.int64) - c["f"]
        assert all(tuple(e) in have for e in ij[:3].tolist())
    assert VC.PAIR_CHUNK + 1 == 1025


# ---- 2. the block references against the dense inverse -------------------------------------------------------------------------
def residuals_of(c):
    return np.random.default_rng(len(c["I"])).normal(scale=0.01, size=(len(c["I"]), 3))


SMALL_BAND = [n for n in VC.BAND if VC.CASE[n]["nu"] <= VC.BOTH_REFS_MAX]


@pytest.mark.parametrize("name", SMALL_BAND)
def test_block_references_agree_with_the_dense_inverse(name):
    c = VC.CASE[name]
    pairs = VC.pairs_of(c)
    var, pv, _ = RV.band_reference(c["I"], c["n"], c["f"], c["d"], c["B"], pairs)
    vd, pd = RV.dense_reference(c["I"], c["n"], c["f"], c["d"], pairs)
    z = VC.zero_pairs(c)
    assert np.all(pv[z] == 0) and np.all(pd[z] == 0) and np.all(var[:c["f"]] == 0)
    res = residuals_of(c)
    eb = ED.band_edge_reference(c["I"], c["n"], c["f"], c["d"], c["B"], res)
    ed = ED.edge_reference(c["I"], c["n"], c["f"], c["d"], res)
    errs = dict(var=worst(var[c["f"]:], vd[c["f"]:]), pairs=worst(pv[~z], pd[~z]))
    for k in ("edge_var", "leverage", "chi2"):
        np.testing.assert_array_equal(eb[k] == 0, ed[k] == 0)
        errs[k] = worst(eb[k], ed[k])
    print("reference to reference, %s: %s" % (name, ", ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) < REF_RTOL
    assert eb["scale"] == ed["scale"]


def test_the_cases_above_the_dense_limit_are_left_to_the_block_reference():
    assert SMALL_BAND == ["b8_257", "b16_129", "b28_74", "b32_65", "b32_span", "b8_span33", "b8_fixed3"]


# ---- 3. what the tolerance can see ----------------------------------------------------------------------------------------------
MUTANTS = ("pad_coupled", "last_uncoupled", "closure_left_out")
_split_band = RV.split_band


def mutated_split(mutant):
    """split_band with one defect at a block edge: the pad rows of the last block tied to the row before them (an edge of
    weight one each, as if the sequence went on), the coupling into the last block missing, the last live closure missing."""
    def split(p, q, w, nu, B):
        D, U, (cp, cq, cw) = _split_band(p, q, w, nu, B)
        nb = len(D)
        if mutant == "pad_coupled":
            for r in range(nu, nb * B):
                kb, rr = divmod(r, B)
                assert rr > 0                                                        # (the row before lies in the same block)
                D[kb, rr, rr] += 1.0
                D[kb, rr - 1, rr - 1] += 1.0
                D[kb, rr, rr - 1] -= 1.0
                D[kb, rr - 1, rr] -= 1.0
        elif mutant == "last_uncoupled":
            U[nb - 2] = 0.0
        elif mutant == "closure_left_out":
            live = np.flatnonzero(cw != 0)
            keep = np.ones(len(cw), dtype=bool)
            keep[live[-1:]] = False
            cp, cq, cw = cp[keep], cq[keep], cw[keep]
        return D, U, (cp, cq, cw)
    return split


def references(c, res):
    var, pv, _ = RV.band_reference(c["I"], c["n"], c["f"], c["d"], c["B"], VC.pairs_of(c))
    return var, pv, ED.band_edge_reference(c["I"], c["n"], c["f"], c["d"], c["B"], res)


# case -> the mutants that cannot touch it (b8_257 has no closure, the last block of b16_129 no pad row; b8_span33 has seven
# pad rows and nine live closures: all three mutants act on it)
INERT = {"b8_257": ("closure_left_out",), "b16_129": ("pad_coupled",), "b8_span33": ()}


@pytest.mark.parametrize("name", ["b8_257", "b16_129", "b8_span33"])
def test_the_comparison_rejects_a_wrong_index_at_a_block_edge(name, monkeypatch):
    c = VC.CASE[name]
    res = residuals_of(c)
    var, pv, edge = references(c, res)
    check_variance(dict(var=var, pair_var=pv), var, pv, c, rtol=RTOL)              # the helper accepts the reference itself
    check_edges(edge, edge, c)
    for mutant in MUTANTS:
        with monkeypatch.context() as mp:
            mp.setattr(RV, "split_band", mutated_split(mutant))
            mp.setattr(ED, "split_band", mutated_split(mutant))
            mvar, mpv, medge = references(c, res)
        if mutant in INERT[name]:
            np.testing.assert_array_equal(mvar, var)
            np.testing.assert_array_equal(mpv, pv)
            for k in ("edge_var", "leverage", "chi2"):
                np.testing.assert_array_equal(medge[k], edge[k])
            continue
        f, z = c["f"], VC.zero_pairs(c)
        seen = dict(var=worst(mvar[f:], var[f:]), pairs=worst(mpv[~z], pv[~z]), edge_var=worst(medge["edge_var"], edge["edge_var"]))
        print("mutant %s on %s: %s" % (mutant, name, ", ".join("%s %.2e" % kv for kv in seen.items())))
        # every output is off by far more than the tolerance ...
        assert min(seen.values()) > 1e3 * RTOL
        # ... and the helpers of the GPU file say so, each on its own
        with pytest.raises(AssertionError):
            check_variance(dict(var=mvar, pair_var=pv), var, pv, c, rtol=RTOL)
        with pytest.raises(AssertionError):
            check_variance(dict(var=var, pair_var=mpv), var, pv, c, rtol=RTOL)
        with pytest.raises(AssertionError):
            check_edges(medge, edge, c)
