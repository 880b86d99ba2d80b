"""irotavg_components / irotavg_components_dev (irotavg_amd/csrc/components.hip, components.hpp, devapi.hip;
torch_api.components, extract_component, scatter_component; docs/components.md) on the device.

The reference is a union-find written here (reference): labels = least id, sizes, the selection with its tie rule, the
order-preserving maps. Everything is an integer, so every comparison is exact and there is no tolerance. Each case is held
to it in the device form with sentinel-filled outputs (the entries past n' / m' stay as they were), a second call gives the
same bytes, and the host form gives the device form's arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from irotavg_amd import capi, torch_api

pytestmark = pytest.mark.gpu
OUTS = ("label", "view_map", "edge_map", "views", "edges", "I_out")
SENTINEL = -77


def t32(a):
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.int32, device=torch.device("cuda", torch.cuda.current_device()))


def reference(I, n, f, rank, which):
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    usable = np.array([(rank is None or rank[k] >= 0) and a != b for k, (a, b) in enumerate(I)])
    for a, b in I[usable]:
        ra, rb = find(a), find(b)
        parent[max(ra, rb)] = min(ra, rb)
    label = np.array([find(v) for v in range(n)])
    sizes = np.bincount(label, minlength=n)
    sel = int(np.argmax(sizes)) if which else 0                    # argmax: the first, so the smallest label of a tie
    views = np.flatnonzero(label == sel)
    edges = np.flatnonzero(usable & (label[I[:, 0]] == sel))
    view_map, edge_map = np.full(n, -1), np.full(len(I), -1)
    view_map[views], edge_map[edges] = np.arange(len(views)), np.arange(len(edges))
    info = [len(np.unique(label)), len(views), len(edges), int((views < f).sum()), sel, int(sizes.max())]
    return dict(label=label, view_map=view_map, edge_map=edge_map, views=views, edges=edges, I_out=view_map[I[edges]], info=info)


def run_dev(I, n, f, rank, which, skip=(), info=True):
    """the device form with sentinel-filled outputs of full capacity; the outputs named in `skip` are passed as NULL"""
    m = len(I)
    out = {k: torch.full(s, SENTINEL, dtype=torch.int32, device=t32([0]).device)
           for k, s in zip(OUTS, ((n,), (n,), (m,), (n,), (m,), (m, 2)))}
    ei, rk = t32(I), None if rank is None else t32(rank)
    s = (C.c_int64 * 6)(*([SENTINEL] * 6))
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = capi.lib().irotavg_components_dev(m, n, f, ptr(ei), ptr(rk), which, *[None if k in skip else ptr(out[k]) for k in OUTS],
                                           s if info else None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return dict({k: v.cpu().numpy() for k, v in out.items()}, rc=rc, info=list(s))


def held_to_reference(got, want, skip=()):
    assert got["rc"] == capi.OK and got["info"] == want["info"]
    n1, m1 = want["info"][1], want["info"][2]
    for k, count in zip(OUTS, (None, None, None, n1, m1, m1)):
        if k in skip:
            assert (got[k] == SENTINEL).all(), k
            continue
        np.testing.assert_array_equal(got[k][:count], want[k], err_msg=k)
        assert count is None or (got[k][count:] == SENTINEL).all(), k


def chain(n, down=False):
    I = np.array([(i, i + 1) for i in range(n - 1)] or [(0, 0)], dtype=np.int32)
    return (I[::-1].copy() if down else I), n, None


def band_cut():
    """4096 views, span <= 8; every edge of every 97th view is forbidden: many components, chunks across workgroups"""
    rng = np.random.default_rng(5)
    I = np.array([(i, i + d) for i in range(4096) for d in rng.choice(np.arange(1, 9), 3, replace=False) if i + d < 4096], dtype=np.int32)
    return I, 4096, np.where(((I % 97) == 0).any(axis=1), -1, 0).astype(np.int32)


def arr(*pairs):
    return np.array(pairs, dtype=np.int32)


CASES = {"chain%d%s" % (n, "down" if down else ""): chain(n, down)
         for n in (1, 2, 63, 64, 65, 255, 256, 257, 1025) for down in (False, True)}
CASES.update({
    "star_high_centre": (arr(*[(299, i) for i in range(299)]), 300, None),
    "star_centre_0": (arr(*[(i, 0) for i in range(1, 300)]), 300, None),
    # 0 alone, {1, 2, 3} and {4, 5, 6} tie: the largest is label 1, the anchor's is smaller, fixed views 1 and 2 lie outside it
    "tie_and_small_anchor": (arr((1, 2), (2, 3), (4, 5), (6, 5)), 7, None),
    # isolated 3 and 7, self loops, a parallel and a reversed duplicate
    "edge_kinds": (arr((0, 1), (1, 1), (0, 1), (1, 0), (2, 2), (4, 5), (5, 6), (6, 4), (3, 3)), 8, None),
    # rank < 0 on the only edge that joins 0..4 with 5..9, and on a chord inside each part (dropped; the views stay)
    "rank_cut": (arr(*[(i, i + 1) for i in range(9)], (0, 3), (9, 6)), 10, np.array([0, 1, 0, 2, -1, 0, 0, 5, 0, -2, -1], dtype=np.int32)),
    "band_cut": band_cut(),
})
WANT = {}  # (case, which, f) -> the reference, computed once


@pytest.mark.parametrize("f", [1, 3])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_components_equal_the_union_find(case, which, f):
    I, n, rank = CASES[case]
    f = min(f, n)
    want = WANT.setdefault((case, which, f), reference(I, n, f, rank, which))
    got = run_dev(I, n, f, rank, which)
    held_to_reference(got, want)
    again = run_dev(I, n, f, rank, which)
    assert all(got[k].tobytes() == again[k].tobytes() for k in OUTS) and got["info"] == again["info"]
    host = capi.components(I, n, f, rank, which)
    n1, m1 = want["info"][1], want["info"][2]
    for k, hk, count in zip(OUTS, ("label", "view_map", "edge_map", "views", "edges", "I"), (n, n, len(I), n1, m1, m1)):
        np.testing.assert_array_equal(host[hk], got[k][:count], err_msg=k)
    assert list(host["info"].values()) == got["info"]


def test_a_bad_id_is_refused_and_nothing_is_written():
    I, n, _ = CASES["chain257"]
    for bad, at in ((-1, (0, 0)), (257, (255, 1)), (2 ** 31 - 1, (100, 0))):
        Ib = I.copy()
        Ib[at] = bad
        got = run_dev(Ib, n, 1, None, 1)
        assert got["rc"] == capi.ERR_BAD_ARG and got["info"] == [SENTINEL] * 6
        assert all((got[k] == SENTINEL).all() for k in OUTS)
    assert torch_api.components(t32(Ib).long() * 2 ** 20, n, allow_rc=(capi.ERR_BAD_ARG,))["label"] is None   # narrowed to -1


@pytest.mark.parametrize("skip", [(k,) for k in OUTS] + [OUTS])
def test_every_output_may_be_null(skip):
    I, n, rank = CASES["band_cut"]
    want = WANT.setdefault(("band_cut", 1, 3), reference(I, n, 3, rank, 1))
    held_to_reference(run_dev(I, n, 3, rank, 1, skip), want, skip)
    assert run_dev(I, n, 3, rank, 1, skip, info=False)["rc"] == capi.OK


def test_inputs_in_flight_and_outputs_consumed_on_a_side_stream():
    I, n, rank = CASES["band_cut"]
    want = WANT.setdefault(("band_cut", 1, 1), reference(I, n, 1, rank, 1))
    half, rk = t32(I // 2), t32(rank)
    odd = t32(I % 2)
    big = torch.ones(1 << 25, dtype=torch.float64, device=half.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(16):                                       # keeps the stream busy while the call is made
            big = big * 1.5
        c = torch_api.components(half * 2 + odd, n, 1, rk, "largest")   # the inputs are produced on the stream
        doubled = c["views"] * 2                                  # consumed right behind the call, no synchronise
    side.synchronize()
    assert list(c["info"].values()) == want["info"] and (c["n_total"], c["m"], c["f"]) == tuple(want["info"][1:4])
    np.testing.assert_array_equal(doubled.cpu().numpy(), 2 * want["views"])
    np.testing.assert_array_equal(c["edge_index"].cpu().numpy(), want["I_out"])


def test_end_to_end_a_cut_graph_is_extracted_initialised_and_scattered_back():
    rng = np.random.default_rng(11)
    I = arr(*[(i, i + d) for i in range(48) for d in (1, 2, 3) if i + d < 48])
    QQ = rng.normal(size=(len(I), 4))
    QQ /= np.linalg.norm(QQ, axis=1, keepdims=True)
    rank = np.where((I[:, 0] < 30) & (I[:, 1] >= 30), -1, 0).astype(np.int32)   # nothing usable joins 0..29 with 30..47
    ei, rk = t32(I), t32(rank)
    qq = torch.tensor(QQ, dtype=torch.float64, device=ei.device)
    Q = torch.full((48, 4), -9.0, dtype=torch.float64, device=ei.device)
    Q[0] = torch.tensor([0, 0, 0, 1.0])
    whole = torch_api.init_tree(ei, qq, 48, Q.clone(), rank=rk, allow_rc=(capi.ERR_NOT_SPANNING,))
    assert whole["rc"] == capi.ERR_NOT_SPANNING and whole["info"]["components"] == 2
    c = torch_api.components(ei, 48, 1, rk)
    x = torch_api.extract_component(c, qq, Q, rk)
    assert (x["n_total"], x["f"]) == (30, 1) and c["views"].tolist() == list(range(30)) and (x["rank"] >= 0).all()
    sub = torch_api.init_tree(x["edge_index"], x["QQ"], x["n_total"], x["Q"], x["f"], x["rank"])
    assert sub["rc"] == capi.OK and sub["info"]["components"] == 1
    before = Q.cpu().numpy().copy()
    torch_api.scatter_component(c, Q, sub["Q"])
    after = Q.cpu().numpy()
    assert after[:30].tobytes() == sub["Q"].cpu().numpy().tobytes() and not (after[1:30] == -9.0).any()
    assert after[30:].tobytes() == before[30:].tobytes()
