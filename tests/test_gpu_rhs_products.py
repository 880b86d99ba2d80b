"""The right-hand sides of the banded direct solver run as SMALL matrix-core products (bcr.hip, BcrRs: four 4 x 4 x 4 fp64
blocks per instruction instead of a 16-column tile that holds three columns and thirteen of zeros).

1. An exact-answer probe of the device functions themselves (capi.bcr_rhs_products: one wave, W_R = D^-1 R,
   R_c -= Q' W_R, R_a -= P W_R): integer matrices, so every product and sum is exact in fp64 and the comparison with NumPy's
   integer matmul is for EQUALITY. A permuted lane layout, a wrong row group, a block of the instruction that is only
   partly filled (B = 8: two row groups; B = 24: four and two) or an update that is not skipped show as a wrong integer.
2. The routes end to end: irls on a view sequence against the oracle by the bars of test_gpu_band_direct.py (identical
   iteration counts, rotations 1e-9 rad, weights 1e-7), and a second irls on the same handle -- served from the kept
   unit-weight factor, i.e. by the right-hand-side-only pass -- bit for bit what the full solve gives
   (IROTAVG_BCR_NO_UNIT_FACTOR=1). Block size, level shape and the fused level-0 assembly are asserted from direct_info().
   The mixed level 1 of blocks of 24 needs 512 chunks of 192 rows at level 0: that case cannot be smaller than 98 614 views.
"""
import os

import numpy as np
import pytest

from irotavg_amd import capi, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
SIG = 5 * np.pi / 180
SWITCH = "IROTAVG_BCR_NO_UNIT_FACTOR"


# ---- 1. the probe ---------------------------------------------------------------------------------------------------
def small_ints(B, seed):
    rng = np.random.default_rng([B, seed])
    D = rng.integers(-64, 65, size=(B, B))
    D = np.triu(D) + np.triu(D, 1).T
    P, Q = rng.integers(-64, 65, size=(2, B, B))
    R, Ra, Rc = rng.integers(-64, 65, size=(3, B, 3))
    return D, P, Q, R, Ra, Rc


def distinct_ints(B, seed):
    """every entry of D^-1 (up to its symmetry), P, Q and R another integer"""
    rng = np.random.default_rng([B, seed, 7])
    nt = B * (B + 1) // 2
    pool = rng.permutation(np.arange(1, nt + 2 * B * B + 3 * B + 1)) * rng.choice([-1, 1], size=nt + 2 * B * B + 3 * B)
    D = np.zeros((B, B), dtype=np.int64)
    D[np.triu_indices(B)] = pool[:nt]
    D = D + np.triu(D, 1).T
    P = pool[nt:nt + B * B].reshape(B, B)
    Q = pool[nt + B * B:nt + 2 * B * B].reshape(B, B)
    R = pool[nt + 2 * B * B:].reshape(B, 3)
    assert len(set(np.concatenate([D[np.triu_indices(B)], P.ravel(), Q.ravel(), R.ravel()]).tolist())) == len(pool)
    Ra, Rc = rng.integers(-64, 65, size=(2, B, 3))
    return D, P, Q, R, Ra, Rc


def run_probe(M, hasP=True, hasQ=True):
    D, P, Q, R, Ra, Rc = M
    out = capi.bcr_rhs_products(D, P, Q, R, hasP, hasQ, Ra=Ra, Rc=Rc)
    WR = D @ R
    assert np.abs(P @ WR).max() < 2 ** 53 and np.abs(Q.T @ WR).max() < 2 ** 53    # exact in fp64
    assert np.array_equal(out["WR"], WR.astype(np.float64))
    assert np.array_equal(out["Ra"], (Ra - P @ WR if hasP else Ra).astype(np.float64))
    assert np.array_equal(out["Rc"], (Rc - Q.T @ WR if hasQ else Rc).astype(np.float64))


@pytest.mark.parametrize("B", [8, 16, 24, 32])
def test_probe_small_integers(B):
    for seed in range(3):
        run_probe(small_ints(B, seed))


@pytest.mark.parametrize("B", [8, 16, 24, 32])
def test_probe_distinct_entries(B):
    run_probe(distinct_ints(B, 1))


@pytest.mark.parametrize("B", [8, 16, 24, 32])
def test_probe_skipped_updates_leave_their_targets(B):
    M = small_ints(B, 11)
    run_probe(M, hasP=False)
    run_probe(M, hasQ=False)
    run_probe(M, hasP=False, hasQ=False)


def test_probe_refuses_other_block_sizes():
    for B in (4, 12, 20, 28, 40):
        D = np.eye(B)
        with pytest.raises(capi.IrotavgError):
            capi.bcr_rhs_products(D, D, D, np.zeros((B, 3)))


# ---- 2. the routes --------------------------------------------------------------------------------------------------
def mst_init(S, n, f=1):
    Q = np.zeros((n, 4)); Q[:, 3] = 1; Q[:f] = S["Qgt"][:f]
    rc, Qm = O.init_mst(Q, S["QQ"], S["I"], f)
    assert rc == 0
    return Qm


def perturbed(Qa, f=1, seed=99):
    rng = np.random.default_rng(seed)
    Qb = Qa.copy()
    Qb[f:] = synth.qmul(Qa[f:], synth.qexp(0.05 * rng.standard_normal((len(Qa) - f, 3))))
    return Qb


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def two_calls(S, n, Qa, Qb, off):
    if off:
        os.environ[SWITCH] = "1"
    try:
        with capi.Graph(S["I"], S["QQ"], n, 1, band_direct=1) as G:
            recs = []
            for Q0 in (Qa, Qb):
                G.set_rotations(Q0)
                b = G.irls(4, SIG, 100, 1e-3)
                recs.append(dict(iters=b["iters"], scores=np.asarray(b["scores"])[:b["iters"]], Q=G.get_rotations(),
                                 w=G.get_weights(), info=G.direct_info(), stats=G.stats()))
            return recs
    finally:
        os.environ.pop(SWITCH, None)


def route(n, m, seed, block, levels, kept, mixed=False):
    S = synth.make_graph(n, m, 0.0, seed=seed, p_band_out=0.02)
    Qa = mst_init(S, n)
    Qb = perturbed(Qa)
    on, off = two_calls(S, n, Qa, Qb, False), two_calls(S, n, Qa, Qb, True)
    for r in on + off:
        info = r["info"]
        assert info["block"] == block and info["closures"] == 0 and info["fused_assembly"] == 1, info
        assert [lv["blocks"] for lv in info["levels"]] == levels, info
        lv1 = info["levels"][1]
        assert (lv1["reduced"] < lv1["blocks"]) == mixed, info
        assert r["stats"]["pcg_solves"] == 0 and r["stats"]["direct_solves"] > 0
    # the second call of the handle that keeps the factor is served from it: the right-hand-side-only pass
    assert [r["info"]["unit_factor"] for r in on] == [kept, kept], on[1]["info"]
    assert [r["info"]["unit_factor_solves"] for r in on] == [0, kept], on[1]["info"]
    assert [r["info"]["unit_factor"] for r in off] == [0, 0] and off[1]["info"]["unit_factor_solves"] == 0
    for a, b in zip(on, off):
        assert a["iters"] == b["iters"] and a["iters"] >= 2
        for k in ("scores", "Q", "w"):
            same_bits(a[k], b[k])
    ro = O.irls(S["QQ"], S["I"], Qa, 1, 4, SIG, 100, 1e-3)
    assert on[0]["iters"] == ro["iters"]
    assert synth.angular_distance(on[0]["Q"], ro["Q"]).max() < 1e-9
    np.testing.assert_allclose(on[0]["w"], ro["weights"], rtol=1e-7)


# 129 blocks at level 0 is the fewest that gives three levels (17 separators are more than the single-workgroup top of
# sixteen takes): n = 128 B + 2 views, one of them fixed -> 129 -> 17 -> 3 blocks, the top in one workgroup
@pytest.mark.parametrize("n,m,block", [(128 * 8 + 2, 3 * (128 * 8 + 2) - 6, 8), (128 * 16 + 2, 15 * (128 * 16 + 2), 16),
                                       (128 * 24 + 2, 21 * (128 * 24 + 2), 24)])
def test_three_levels_single_workgroup_top(n, m, block):
    route(n, m, 5, block, [129, 17, 3], 1)


def test_mixed_level_one_blocks_of_24():
    """512 chunks of eight blocks fill the device at level 0 (two workgroups on each of 256 compute units); the 13 blocks
    behind them enter level 1 raw, next to the 512 separators (band_cases.py: "mixed")"""
    nb0 = 512 * 8 + 13
    n = nb0 * 24 - 3 + 1
    route(n, 21 * n, 6, 24, [nb0, 512 + 13, 66, 9], 1, mixed=True)


def test_two_levels_launch_by_launch():
    """65 blocks -> a top of nine: the level-0 launch and the single-workgroup top as a launch of its own; no factor is kept"""
    n = 64 * 24 + 2
    route(n, 21 * n, 7, 24, [65, 9], 0)
