"""The level-0 reduction of the banded direct solver assembles level 0 itself (bcr.hip, k_bcr_reduce<..., ASM = true>: the
workgroup of a chunk runs K3's body -- asm0w.hpp -- for the chunk's own 64-row slices and then reduces the chunk; extra
workgroups assemble the slices under no chunk) instead of a launch of k_assemble0w in front of the solve.

The arithmetic is the same instructions on the same inputs, so the fused form is held against the two-launch form
(IROTAVG_BCR_NO_FUSED_ASM=1) BITWISE: iteration count, score trace, rotations, weights. `direct_info()["fused_assembly"]`
says which form the handle's last assembly + solve took.
"""
import os

import numpy as np
import pytest

from irotavg_amd import capi, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
SIG = 5 * np.pi / 180


def mst_init(I, QQ, Qgt, n, f=1):
    Q = np.zeros((n, 4)); Q[:, 3] = 1; Q[:f] = Qgt[:f]
    rc, Qm = O.init_mst(Q, QQ, I, f)
    assert rc == 0
    return Qm


def run(I, QQ, n, f, Qm, fused, l1=0):
    """irls (after l1ra(l1) if asked) from Qm on a fresh handle, in the fused or in the two-launch form"""
    if not fused:
        os.environ["IROTAVG_BCR_NO_FUSED_ASM"] = "1"
    try:
        with capi.Graph(I, QQ, n, f, band_direct=1) as G:
            before = G.direct_info()
            G.set_rotations(Qm)
            out = dict(before=before)
            if l1:
                a = G.l1ra(l1, 1e-3)
                out.update(l1_iters=a["iters"], l1_scores=np.asarray(a["scores"]), l1_Q=G.get_rotations())
            b = G.irls(4, SIG, 30, 1e-3)
            out.update(iters=b["iters"], scores=np.asarray(b["scores"]), Q=G.get_rotations(), w=G.get_weights(),
                       info=G.direct_info(), stats=G.stats())
            return out
    finally:
        os.environ.pop("IROTAVG_BCR_NO_FUSED_ASM", None)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def fused_equals_two_launch(I, QQ, n, f, Qm, block, l1=0):
    r1 = run(I, QQ, n, f, Qm, True, l1)
    r0 = run(I, QQ, n, f, Qm, False, l1)
    for r in (r0, r1):
        assert r["info"]["block"] == block, r["info"]
        assert r["before"]["fused_assembly"] == 0                  # nothing assembled yet
        assert r["stats"]["direct_solves"] > 0 and r["stats"]["pcg_solves"] == 0, r["stats"]
    assert r1["info"]["fused_assembly"] == 1 and r0["info"]["fused_assembly"] == 0
    assert r1["iters"] == r0["iters"] and r1["iters"] >= 1
    same_bits(r1["scores"], r0["scores"])
    same_bits(r1["Q"], r0["Q"])
    same_bits(r1["w"], r0["w"])
    assert np.array_equal(r1["Q"], r0["Q"]) and np.array_equal(r1["w"], r0["w"])
    assert np.isfinite(r1["Q"]).all() and np.isfinite(r1["scores"]).all()
    if l1:
        assert r1["l1_iters"] == r0["l1_iters"]
        same_bits(r1["l1_scores"], r0["l1_scores"])
        same_bits(r1["l1_Q"], r0["l1_Q"])
    return r1, r0


# blocks of 8 (band 3, ONE slice per chunk): one chunk + one block (the eight-wave workgroups, whose upper four waves only
# keep K3's barriers company), a partial last slice and a partial last chunk at two and three levels;
# 16 (band 15, two slices per chunk), 3001 rows: no multiple of 128; 24 (band 21, three slices), 3001: no multiple of 192;
# 32 (band 29, four slices per chunk, one workgroup per CU)
@pytest.mark.parametrize("n,m,block", [(65, 3 * 65 - 6, 8), (520, 3 * 520 - 6, 8), (4100, 3 * 4100 - 6, 8),
                                       (3001, 15 * 3001, 16), (3001, 21 * 3001, 24), (2511, 74830, 32)])
def test_fused_assembly_is_bitwise_the_two_launch_form(n, m, block):
    S = synth.make_graph(n, m, 0.0, seed=n, p_band_out=0.02)
    Qm = mst_init(S["I"], S["QQ"], S["Qgt"], n)
    fused_equals_two_launch(S["I"], S["QQ"], n, 1, Qm, block)


def test_mixed_level_one_slices_are_assembled_by_the_extra_workgroups():
    """36000 views in blocks of 8 = 563 chunks on 512 resident slots: the rows of the 51 surplus chunks' blocks lie under
    no level-0 chunk -- their slices are assembled by the workgroups behind the chunks' and gathered at level 1."""
    n, m = 36000, 4 * 36000 - 10
    S = synth.make_graph(n, m, 0.0, seed=12, p_band_out=0.01)
    Qm = mst_init(S["I"], S["QQ"], S["Qgt"], n)
    r1, _ = fused_equals_two_launch(S["I"], S["QQ"], n, 1, Qm, 8)
    lev = r1["info"]["levels"]
    assert lev[1]["reduced"] < lev[1]["blocks"] and 8 * lev[0]["chunks"] < lev[0]["blocks"], lev


def test_fixed_views_and_duplicate_edges():
    """f = 3 fixed views, 30 % of the edges given as (j, i), 80 duplicates: the boundary-slot walk (edges to fixed views
    reach the diagonal, the right-hand side and bval only) inside the fused form."""
    n, f = 1500, 3
    S = synth.make_graph(n, 4 * n, 0.0, seed=13, p_band_out=0.02)
    rng = np.random.default_rng(5)
    I, QQ = S["I"].copy(), S["QQ"].copy()
    flip = rng.random(len(I)) < 0.3
    I[flip] = I[flip][:, ::-1]
    QQ[flip] = synth.qconj(QQ[flip])
    I = np.concatenate([I, I[:80]]).astype(np.int32)
    QQ = np.concatenate([QQ, QQ[:80]])
    assert ((I[:, 1] < f) & (I[:, 0] >= f)).sum() > 0 and ((I[:, 0] < f) & (I[:, 1] >= f)).sum() > 0
    Qm = mst_init(I, QQ, S["Qgt"], n, f)
    r1, _ = fused_equals_two_launch(I, QQ, n, f, Qm, 8)
    np.testing.assert_array_equal(r1["Q"][:f], Qm[:f])


@pytest.mark.parametrize("m,block", [(33000, 12), (57000, 20)])
def test_other_block_sizes_keep_the_two_launches_and_match_the_oracle(m, block):
    """chunks of 96 / 160 rows are no whole slices"""
    n = 3000
    S = synth.make_graph(n, m, 0.0, seed=3, p_band_out=0.02)
    Qm = mst_init(S["I"], S["QQ"], S["Qgt"], n)
    r = run(S["I"], S["QQ"], n, 1, Qm, True)
    assert r["info"]["block"] == block and r["info"]["fused_assembly"] == 0, r["info"]
    ro = O.irls(S["QQ"], S["I"], Qm, 1, 4, SIG, 30, 1e-3)
    assert r["iters"] == ro["iters"]
    np.testing.assert_allclose(r["scores"], ro["scores"], rtol=1e-7)
    assert synth.angular_distance(r["Q"], ro["Q"]).max() < 1e-9
    np.testing.assert_allclose(r["w"], ro["weights"], rtol=1e-7)


def test_closures_keep_the_two_launches():
    n = 3000
    S = synth.closure_graph(n, 12000, 5, 7, 1)
    Qm = mst_init(S["I"], S["QQ"], S["Qgt"], n)
    r = run(S["I"], S["QQ"], n, 1, Qm, True)
    assert r["info"]["block"] == 8 and r["info"]["closures"] == 5 and r["info"]["fused_assembly"] == 0, r["info"]
    assert r["stats"]["direct_solves"] > 0 and np.isfinite(r["Q"]).all()


def test_l1ra_then_irls_on_one_handle():
    """l1ra's assemblies (the primal-dual Hessian: launches of k_assemble0w, other modes) alternate with the fused IRLS
    assembly on ONE handle and its level-0 arrays"""
    n = 3001
    S = synth.make_graph(n, 21 * n, 0.0, seed=4, p_band_out=0.02)
    Qm = mst_init(S["I"], S["QQ"], S["Qgt"], n)
    fused_equals_two_launch(S["I"], S["QQ"], n, 1, Qm, 24, l1=3)
