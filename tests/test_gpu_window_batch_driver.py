"""The host driver the batched calls on device arrays share (irotavg_amd/csrc/batchdev.hpp: the pinned block of records
and descriptors, the sequence number, the wait): window_init_mst_batch, window_solve_batch, window_uncertainty_batch and
window_gate_batch interleaved in one process while their batches grow and shrink.

What the driver itself can get wrong is a block that has to grow (records and descriptors move, the device pointer is
new) and a sequence number or record left over from another call or another kind of call. So every problem goes through
the four calls alone (nb = 1) first, and then batches of copies of those problems, at nb = 1, 3, 70, 2, 200, must give the
same bytes: the kernels and the inputs are the same, there is no tolerance. Each step up is more than the half a block
is given as headroom, so a process that starts with this module allocates the block of every family at least three
times; behind modules that ran larger batches the blocks are there already and the sequence numbers are what is checked."""
import numpy as np
import pytest
import torch

from irotavg_amd import torch_api

pytestmark = pytest.mark.gpu
MARK = -7.25  # free rows of Q on the way into the initialisation
KINDS = ("init", "solve", "uncertainty", "gate")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def t64(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev())


def unit(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def problem(name, nv, f, I, cand, seed):
    """a random unit measurement per edge and per candidate, random fixed rows, marked free rows"""
    I, cand = np.array(I, dtype=np.int32).reshape(-1, 2), np.array(cand, dtype=np.int32).reshape(-1, 2)
    rng = np.random.default_rng([seed, nv, f, len(I)])
    Q0 = np.full((nv, 4), MARK)
    Q0[:f] = unit(rng, f)
    return dict(name=name, nv=nv, f=f, ne=len(I), nc=len(cand), I=I, QQ=unit(rng, len(I)), Q0=Q0, cand=cand,
                cand_QQ=unit(rng, len(cand)))


# triangles (nv = 3, f = 1, ne = 3), and twelve views each linked to its four predecessors so that descriptors differ
PROBLEMS = [problem("triangle-%d" % s, 3, 1, [(0, 1), (1, 2), (0, 2)], [(0, 2), (2, 1)], s) for s in range(3)]
PROBLEMS.append(problem("twelve", 12, 2, [(p, v) for v in range(1, 12) for p in range(max(0, v - 4), v)],
                        [(0, 11), (9, 3), (5, 2)], 7))


def call(kind, cases, ref):
    """One batched call of `kind` on `cases`. Its inputs are the nb = 1 outputs of the call before it (ref[name][kind]),
    so every call stands alone. Returns, per problem, {output name: its rows}."""
    cat = lambda rows: np.concatenate(list(rows))
    ends = lambda key: np.concatenate([[0], np.cumsum([c[key] for c in cases])])
    sizes = np.array([(c["nv"], c["f"], c["ne"]) for c in cases], dtype=np.int32)
    ei = torch.tensor(cat(c["I"] for c in cases), dtype=torch.int32, device=dev())
    QQ = t64(cat(c["QQ"] for c in cases))
    if kind == "init":
        Q = t64(cat(c["Q0"] for c in cases))
        r = torch_api.window_init_mst_batch(sizes, ei, QQ, Q)
        outs = [("Q", Q, "nv")]
    elif kind == "solve":
        Q = t64(cat(ref[c["name"]]["init"]["Q"] for c in cases))
        r = torch_api.window_solve_batch(sizes, ei, QQ, Q)
        outs = [("Q", Q, "nv"), ("weights", r["weights"], "ne"), ("l1_iters", r["l1_iters"], None),
                ("irls_iters", r["irls_iters"], None), ("kernel", r["kernel"], None)]
    else:
        Q = t64(cat(ref[c["name"]]["solve"]["Q"] for c in cases))
        w = t64(cat(ref[c["name"]]["solve"]["weights"] for c in cases))
        if kind == "uncertainty":
            r = torch_api.window_uncertainty_batch(sizes, ei, QQ, Q, weights=w)
            outs = [("var", r["var"], "nv"), ("edge_var", r["edge_var"], "ne"), ("leverage", r["leverage"], "ne"),
                    ("chi2", r["chi2"], "ne"), ("scale", r["scale"], None)]
        else:
            ci = torch.tensor(cat(c["cand"] for c in cases), dtype=torch.int32, device=dev())
            r = torch_api.window_gate_batch(sizes, ei, QQ, Q, ci, t64(cat(c["cand_QQ"] for c in cases)),
                                            np.array([c["nc"] for c in cases], dtype=np.int32), weights=w)
            outs = [("angle", r["angle"], "nc"), ("pair_var", r["pair_var"], "nc"), ("chi2", r["chi2"], "nc"),
                    ("scale", r["scale"], None)]
    torch.cuda.synchronize()
    assert r["rc"] == 0 and (r["status"] == 0).all(), (kind, len(cases), r["rc"], r["status"])
    per = [dict() for _ in cases]
    for name, a, key in outs:
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        e = np.arange(len(cases) + 1) if key is None else ends(key)
        for b in range(len(cases)):
            per[b][name] = np.ascontiguousarray(a[e[b]:e[b + 1]])
    return per


@pytest.fixture(scope="module")
def ref():
    """every problem through the four calls alone: {problem: {kind: {output: rows}}}, computed once"""
    out = {p["name"]: {} for p in PROBLEMS}
    for kind in KINDS:
        for p in PROBLEMS:
            out[p["name"]][kind] = call(kind, [p], out)[0]
    for p in PROBLEMS:  # the references are results, not the inputs handed through
        assert not (out[p["name"]]["init"]["Q"] == MARK).any() and np.isfinite(out[p["name"]]["solve"]["Q"]).all(), p["name"]
        assert np.isfinite(out[p["name"]]["uncertainty"]["var"]).all() and np.isfinite(out[p["name"]]["gate"]["chi2"]).all(), p["name"]
    return out


def test_mixed_calls_while_the_blocks_grow_and_shrink(ref):
    for nb in (1, 3, 70, 2, 200):
        cases = [PROBLEMS[b % len(PROBLEMS)] for b in range(nb)]
        for kind in KINDS:
            for b, got in enumerate(call(kind, cases, ref)):
                want = ref[cases[b]["name"]][kind]
                assert got.keys() == want.keys()
                for name in want:
                    assert got[name].tobytes() == want[name].tobytes(), (kind, nb, b, cases[b]["name"], name)
