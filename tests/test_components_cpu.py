"""irotavg_components, irotavg_components_dev and the torch front-end (docs/components.md) without a GPU: the symbols, the
argument checks that run before any device is touched, the front-end's own checks, and extract_component /
scatter_component on a hand-made component on CPU tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

from irotavg_amd import capi, torch_api

HOST, DEV = "irotavg_components", "irotavg_components_dev"
# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE = [C.c_void_p(0x10000 * (k + 1)) for k in range(8)]
NAMES = ("I", "rank", "label", "view_map", "edge_map", "views", "edges", "I_out")
M, N = 6, 5
INFO = [-1, -2, -3, -4, -5, -6]


def host_call(m=M, n_total=N, f=1, which=0, I=True, rank=True):
    """the host form on real arrays with sentinel-filled outputs, which must come back untouched"""
    Ia = np.array([(0, 1), (1, 2), (2, 0), (2, 3), (3, 0), (3, 4)], dtype=np.int32)
    rk = np.zeros(M, dtype=np.int32)
    outs = [np.full(k, -7, dtype=np.int32) for k in (N, N, M, N, M, 2 * M)]
    s = (C.c_int64 * 6)(*INFO)
    label, view_map, edge_map, views, edges, I_out = (capi._i(o) for o in outs)
    rc = capi.lib().irotavg_components(m, n_total, f, capi._i(Ia) if I else None, capi._i(rk) if rank else None, which, label,
                                       view_map, edge_map, views, edges, I_out, s)
    assert all((o == -7).all() for o in outs) and list(s) == INFO
    return rc


def dev_call(m=M, n_total=N, f=1, which=0, **ptr):
    p = dict(zip(NAMES, FAKE), **ptr)
    s = (C.c_int64 * 6)(*INFO)
    rc = capi.lib().irotavg_components_dev(m, n_total, f, p["I"], p["rank"], which, p["label"], p["view_map"], p["edge_map"],
                                           p["views"], p["edges"], p["I_out"], s, None)
    assert list(s) == INFO
    return rc


def test_the_symbols_are_listed_with_their_argument_counts():
    for name, nargs in ((HOST, 13), (DEV, 14)):
        assert name in capi.SYMBOLS and len(getattr(capi.lib(), name).argtypes) == nargs
    assert callable(torch_api.TorchGraph.components)


SIZES = [dict(m=0), dict(m=-1), dict(m=0x80000000), dict(n_total=0), dict(n_total=-3), dict(n_total=0x80000000), dict(f=0),
         dict(f=-1), dict(f=N + 1), dict(which=-1), dict(which=2)]


@pytest.mark.parametrize("kw", [dict(I=False)] + SIZES)
def test_the_host_form_refuses_before_any_device_work(kw):
    assert host_call(**kw) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [dict(I=None), dict(I=C.c_void_p(0x10004)), dict(I_out=C.c_void_p(0x80004))] + SIZES +
                         [{name: C.c_void_p(0x90002)} for name in NAMES[1:7]])
def test_the_device_form_refuses_before_any_device_work(kw):
    assert dev_call(**kw) == capi.ERR_BAD_ARG


def test_no_device_arrives_after_the_checks():
    """every well-formed call, the limits themselves included, gets as far as the device"""
    no_device = capi.ERR_NO_DEVICE if capi.lib().irotavg_device_count() <= 0 else capi.ERR_BAD_ARG  # (the made-up addresses)
    if capi.lib().irotavg_device_count() <= 0:
        assert host_call() == host_call(rank=False, f=N, which=1) == capi.ERR_NO_DEVICE
        out = capi.components([(0, 1)], 2, allow_rc=(capi.ERR_NO_DEVICE,))
        assert out["rc"] == capi.ERR_NO_DEVICE and out["label"] is None and out["info"] is None
    for kw in (dict(), dict(m=0x7fffffff), dict(n_total=0x7fffffff), dict(f=N, which=1), dict(rank=C.c_void_p(0x20004)),
               dict(zip(NAMES[1:], [None] * 7))):
        assert dev_call(**kw) == no_device


def test_the_host_wrapper_checks_its_arguments():
    with pytest.raises(ValueError, match="rank"):
        capi.components([(0, 1), (1, 2)], 3, rank=[0, 0, 0])
    with pytest.raises(ValueError, match="which"):
        capi.components([(0, 1), (1, 2)], 3, which="smallest")


def test_the_torch_wrapper_refuses_before_the_c_call(monkeypatch):
    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    ei, rank = torch.zeros((9, 2), dtype=torch.int32), torch.zeros(9, dtype=torch.int32)
    for args, kw, err, match in (((ei, 5), {}, TypeError, "ROCm device"),
                                 ((ei.numpy(), 5), {}, TypeError, "torch.Tensor"),
                                 ((ei.to(torch.int16), 5), {}, TypeError, "edge_index"),
                                 ((ei.t(), 5), {}, ValueError, "edge_index"),
                                 ((ei[:0], 5), {}, ValueError, "at least one row"),
                                 ((ei, 5), dict(rank=rank.long()), TypeError, "rank"),
                                 ((ei, 5), dict(rank=rank[:8]), ValueError, "rank"),
                                 ((ei, 0), {}, ValueError, "n_total"),
                                 ((ei, 2 ** 31), {}, ValueError, "n_total"),
                                 ((ei, 5), dict(f=0), ValueError, "f must"),
                                 ((ei, 5), dict(f=6), ValueError, "f must"),
                                 ((ei, 5), dict(which="smallest"), ValueError, "which")):
        with pytest.raises(err, match=match):
            torch_api.components(*args, **kw)


def hand_made():
    """views 1, 3, 4 of five and edges 0, 2 of four, as components would return them"""
    t = lambda a: torch.tensor(a, dtype=torch.int32)
    return dict(view_map=t([-1, 0, -1, 1, 2]), edge_map=t([0, -1, 1, -1]), views=t([1, 3, 4]), edges=t([0, 2]),
                edge_index=t([(0, 1), (2, 1)]), n_total=3, m=2, f=1)


def test_extract_component_gathers_the_rows_of_the_selection():
    c = hand_made()
    QQ, Q = torch.arange(16.0, dtype=torch.float64).reshape(4, 4), torch.arange(20.0, dtype=torch.float64).reshape(5, 4)
    rank, w = torch.tensor([3, 2, 1, 0], dtype=torch.int32), torch.tensor([0.5, 0.25, 2.0, 4.0], dtype=torch.float64)
    x = torch_api.extract_component(c, QQ, Q, rank, w)
    assert torch.equal(x["QQ"], QQ[[0, 2]]) and torch.equal(x["Q"], Q[[1, 3, 4]])
    assert x["rank"].tolist() == [3, 1] and x["w"].tolist() == [0.5, 2.0]
    assert x["edge_index"] is c["edge_index"] and (x["n_total"], x["m"], x["f"]) == (3, 2, 1)
    bare = torch_api.extract_component(c, QQ)
    assert bare["Q"] is None and bare["rank"] is None and bare["w"] is None
    with pytest.raises(ValueError, match="QQ"):
        torch_api.extract_component(c, QQ[:3])
    with pytest.raises(ValueError, match="Q must"):
        torch_api.extract_component(c, QQ, Q[:4])
    with pytest.raises(TypeError, match="rank"):
        torch_api.extract_component(c, QQ, rank=rank.long())


def test_scatter_component_writes_the_selected_rows_and_no_other():
    c = hand_made()
    full = torch.full((5, 4), -9.0, dtype=torch.float64)
    sub = torch.arange(12.0, dtype=torch.float64).reshape(3, 4)
    assert torch_api.scatter_component(c, full, sub) is full
    assert torch.equal(full[[1, 3, 4]], sub) and (full[[0, 2]] == -9.0).all()
    with pytest.raises(ValueError, match="Q_sub"):
        torch_api.scatter_component(c, full, sub[:2])
    with pytest.raises(ValueError, match="Q_full"):
        torch_api.scatter_component(c, full[:4], sub)
