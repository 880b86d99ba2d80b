"""The eight-row tile of a 24-row (or 8-row) block of the banded direct solver runs as 4 x 4 x 4 fp64 matrix-core products
that share their A-operand over the four column groups of a 16-column tile (bcr.hip, BcrAop), not as a 16-row tile that is
half zeros.

1. An exact-answer probe (capi.bcr_block_products): one elimination's wide products through the member functions of
   BcrElim that the reduction kernels call -- W = D^-1 [P' | Q | R], D_c -= Q' W_Q, D_a -= P W_P, fill = -P W_Q -- by one
   workgroup of 1, 2 and 4 waves (how the column tiles are dealt). Integer matrices with distinct entries: every product
   and sum is exact in fp64, the comparison with NumPy's integer matmul is for EQUALITY. A wrong row group, a transposed
   A-operand, an accumulator register that is not the one the stores and the next product read show as a wrong integer.
   Matrices whose only non-zeros lie in the last eight rows or columns isolate the small tile as a producer and as a k-range.
2. The routes end to end at their smallest shapes (those of test_gpu_rhs_products.py, other seeds): irls against the oracle
   (identical iteration counts, rotations 1e-9 rad, weights 1e-7) and the kept unit-weight factor against
   IROTAVG_BCR_NO_UNIT_FACTOR=1 bit for bit. No kernel is instantiated with the closures' nineteen right-hand-side columns,
   so there is no route of that kind to run; closures on blocks of 24 are test_gpu_band_direct.py's.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from irotavg_amd import capi  # noqa: E402
from test_gpu_rhs_products import route  # noqa: E402

pytestmark = pytest.mark.gpu
SERVED = [(24, 1), (24, 2), (24, 4), (8, 1), (8, 2)]


# ---- 1. the probe ---------------------------------------------------------------------------------------------------
def distinct_ints(B, seed):
    """every entry of D^-1 (up to its symmetry), P, Q and R another non-zero integer; D_c, D_a small integers"""
    rng = np.random.default_rng([B, seed, 24])
    nt = B * (B + 1) // 2
    total = nt + 2 * B * B + 3 * B
    pool = rng.permutation(np.arange(1, total + 1)) * rng.choice([-1, 1], size=total)
    D = np.zeros((B, B), dtype=np.int64)
    D[np.triu_indices(B)] = pool[:nt]
    D = D + np.triu(D, 1).T
    P = pool[nt:nt + B * B].reshape(B, B)
    Q = pool[nt + B * B:nt + 2 * B * B].reshape(B, B)
    R = pool[nt + 2 * B * B:].reshape(B, 3)
    assert len(set(np.abs(np.concatenate([D[np.triu_indices(B)], P.ravel(), Q.ravel(), R.ravel()])).tolist())) == total
    Dc, Da = rng.integers(-64, 65, size=(2, B, B))
    return D, P, Q, R, Dc, Da


def run_probe(M, wpe, hasP=True, hasQ=True):
    D, P, Q, R, Dc, Da = M
    B = len(D)
    out = capi.bcr_block_products(D, P, Q, R, wpe, hasP, hasQ, Dc=Dc, Da=Da)
    Z = np.zeros((B, B), dtype=np.int64)
    W = D @ np.hstack([P.T if hasP else Z, Q if hasQ else Z, R])
    WP, WQ = W[:, :B], W[:, B:2 * B]
    assert max(np.abs(P @ WP).max(), np.abs(P @ WQ).max(), np.abs(Q.T @ WQ).max()) < 2 ** 52    # exact in fp64
    assert np.array_equal(out["W"], W.astype(np.float64))
    assert np.array_equal(out["Dc"], (Dc - Q.T @ WQ if hasQ else Dc).astype(np.float64))
    assert np.array_equal(out["Da"], (Da - P @ WP if hasP else Da).astype(np.float64))
    assert np.array_equal(out["fill"], (-(P @ WQ) if hasP else P).astype(np.float64))


@pytest.mark.parametrize("B,wpe", SERVED)
def test_probe_distinct_entries(B, wpe):
    for seed in range(2):
        run_probe(distinct_ints(B, seed), wpe)


@pytest.mark.parametrize("B,wpe", SERVED)
def test_probe_skipped_updates_leave_their_targets(B, wpe):
    M = distinct_ints(B, 11)
    run_probe(M, wpe, hasP=False)
    run_probe(M, wpe, hasQ=False)
    run_probe(M, wpe, hasP=False, hasQ=False)


@pytest.mark.parametrize("B,wpe", SERVED)
@pytest.mark.parametrize("which", ["rows", "cols"])
def test_probe_only_the_last_eight_rows_or_columns(B, wpe, which):
    """non-zeros only in rows (or only in columns) B - 8 ... B - 1 of P and Q: as rows they are the small tile's
    A-operands alone, as columns its k-steps (and, through W, its accumulators as the next product's B-operand) alone.
    D^-1 is symmetric, so rows and columns at once: its last 8 x 8 block."""
    D, P, Q, R, Dc, Da = distinct_ints(B, 5)
    keep = np.zeros((B, B), dtype=np.int64)
    if which == "rows":
        keep[B - 8:, :] = 1
    else:
        keep[:, B - 8:] = 1
    run_probe((D * keep * keep.T, P * keep, Q * keep, R, Dc, Da), wpe)


def test_probe_refuses_what_it_does_not_serve():
    for B, wpe in [(4, 1), (12, 1), (16, 1), (20, 2), (28, 1), (32, 4), (40, 1), (24, 3), (24, 8), (24, 0), (8, 4)]:
        D = np.eye(B)
        with pytest.raises(capi.IrotavgError):
            capi.bcr_block_products(D, D, D, np.zeros((B, 3)), wpe)


# ---- 2. the routes --------------------------------------------------------------------------------------------------
def test_three_levels_single_workgroup_top_blocks_of_24():
    """129 -> 17 -> 3 blocks: the single-launch upper reduction and the one-workgroup top"""
    n = 128 * 24 + 2
    route(n, 21 * n, 15, 24, [129, 17, 3], 1)


def test_two_levels_launch_by_launch_blocks_of_24():
    """65 -> 9 blocks: the level-0 launch and the top as a launch of its own; no factor is kept"""
    n = 64 * 24 + 2
    route(n, 21 * n, 17, 24, [65, 9], 0)


def test_mixed_level_one_blocks_of_24():
    """512 chunks at level 0, thirteen raw blocks next to their separators at level 1"""
    nb0 = 512 * 8 + 13
    n = nb0 * 24 - 3 + 1
    route(n, 21 * n, 16, 24, [nb0, 512 + 13, 66, 9], 1, mixed=True)
