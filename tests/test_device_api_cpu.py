"""Device-pointer handle API (irotavg_graph_*_dev, irotavg_amd/torch_api.py) without a GPU: the symbols, the argument
checks that run before any device is touched, and the Python front-end's own checks and stride arithmetic."""
import ctypes as C

import pytest
import torch

from irotavg_amd import capi

DEV_SYMBOLS = ["irotavg_graph_create_dev", "irotavg_graph_set_rotations_dev", "irotavg_graph_get_rotations_dev",
               "irotavg_graph_set_weights_dev", "irotavg_graph_get_weights_dev", "irotavg_graph_get_residuals_dev",
               "irotavg_graph_rotation_variance_dev", "irotavg_graph_edge_diagnostics_dev"]

# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE_I, FAKE_QQ = C.c_void_p(0x10000), C.c_void_p(0x20000)


def create_dev(m, n_total, f, I, QQ, rs, cs, h=None):
    h = C.c_void_p(0xdead) if h is None else h
    rc = capi.lib().irotavg_graph_create_dev(C.byref(h), m, n_total, f, I, QQ, rs, cs, None, None)
    return rc, h


def test_every_new_symbol_is_exported_and_declared():
    L = capi.lib()
    for s in DEV_SYMBOLS:
        assert s in capi.SYMBOLS
        assert hasattr(L, s), "missing export: " + s
        assert getattr(L, s).argtypes is not None


def test_create_dev_null_pointers_and_sizes_are_bad_arguments():
    assert capi.lib().irotavg_graph_create_dev(None, 10, 5, 1, FAKE_I, FAKE_QQ, 4, 1, None, None) == capi.ERR_BAD_ARG
    for I, QQ in ((None, FAKE_QQ), (FAKE_I, None), (None, None)):
        rc, h = create_dev(10, 5, 1, I, QQ, 4, 1)
        assert rc == capi.ERR_BAD_ARG and not h.value          # the handle pointer is cleared
    for m in (0, -3):
        rc, h = create_dev(m, 5, 1, FAKE_I, FAKE_QQ, 4, 1)
        assert rc == capi.ERR_BAD_ARG and not h.value
    for n_total, f in ((0, 0), (5, -1), (5, 5), (2 ** 31, 1)):
        assert create_dev(10, n_total, f, FAKE_I, FAKE_QQ, 4, 1)[0] == capi.ERR_BAD_ARG
    assert create_dev(10, 5, 1, C.c_void_p(0x10004), FAKE_QQ, 4, 1)[0] == capi.ERR_BAD_ARG   # pairs not 8-byte aligned


@pytest.mark.parametrize("rs,cs", [(0, 0), (0, 1), (4, 0), (1, 1), (2, 1), (3, 1), (1, 2), (1, 99), (3, 99), (-2, 1),
                                   (1, -99), (2, 3), (2 ** 40, 1)])
def test_create_dev_rejects_strides_that_alias(rs, cs):
    """m = 100 rows of 4: accepted are |rs| >= 4 |cs| or |cs| >= 100 |rs| (include/irotavg_hip.h), nothing else."""
    rc, h = create_dev(100, 50, 1, FAKE_I, FAKE_QQ, rs, cs)
    assert rc == capi.ERR_BAD_ARG and not h.value


@pytest.mark.parametrize("rs,cs", [(4, 1), (1, 100), (1, 128), (6, 1), (16, 2), (-4, 1), (1, -100), (3, 300), (4, -1)])
def test_create_dev_valid_arguments_need_a_device(rs, cs):
    """Strides that cannot alias pass the argument checks; without a HIP device the answer is NO_DEVICE. (With one,
    the made-up addresses are then refused by the pointer check, still before any kernel.)"""
    rc, h = create_dev(100, 50, 1, FAKE_I, FAKE_QQ, rs, cs)
    expected = capi.ERR_NO_DEVICE if capi.lib().irotavg_device_count() <= 0 else capi.ERR_BAD_ARG
    assert rc == expected and not h.value


def test_handle_calls_reject_a_null_handle():
    L = capi.lib()
    assert L.irotavg_graph_set_rotations_dev(None, FAKE_QQ, 4, 1, None) == capi.ERR_BAD_ARG
    assert L.irotavg_graph_get_rotations_dev(None, FAKE_QQ, 4, 1, None) == capi.ERR_BAD_ARG
    assert L.irotavg_graph_set_weights_dev(None, FAKE_QQ, None) == capi.ERR_BAD_ARG
    assert L.irotavg_graph_get_weights_dev(None, FAKE_QQ, None) == capi.ERR_BAD_ARG
    assert L.irotavg_graph_get_residuals_dev(None, FAKE_QQ, 1, 100, None) == capi.ERR_BAD_ARG
    assert L.irotavg_graph_rotation_variance_dev(None, FAKE_QQ, None, None) == capi.ERR_BAD_ARG
    assert L.irotavg_graph_edge_diagnostics_dev(None, FAKE_QQ, None, None, None, None) == capi.ERR_BAD_ARG


# ---- the torch front-end -------------------------------------------------------------------------------------------------
@pytest.fixture
def no_c_calls(monkeypatch):
    """Any use of the C library from here on is an error."""
    from irotavg_amd import torch_api

    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    return torch_api


def test_torchgraph_rejects_cpu_tensors_before_the_c_call(no_c_calls):
    ei = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32)
    QQ = torch.tensor([[0, 0, 0, 1.0]] * 2, dtype=torch.float64)
    with pytest.raises(TypeError, match="ROCm device"):
        no_c_calls.TorchGraph(ei, QQ, 3, 1)
    with pytest.raises(TypeError, match="ROCm device"):
        no_c_calls.TorchGraph(ei.to(torch.int64), QQ, 3, 1)
    with pytest.raises(TypeError):
        no_c_calls.TorchGraph(ei.numpy(), QQ, 3, 1)             # not a tensor at all


def test_torchgraph_rejects_float32_before_the_c_call(no_c_calls):
    ei = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32)
    with pytest.raises(TypeError, match="float64"):
        no_c_calls.TorchGraph(ei, torch.zeros((2, 4), dtype=torch.float32), 3, 1)
    with pytest.raises(TypeError, match="int32"):
        no_c_calls.TorchGraph(ei.to(torch.int16), torch.zeros((2, 4), dtype=torch.float64), 3, 1)


def test_torchgraph_rejects_wrong_shapes_before_the_c_call(no_c_calls):
    QQ = torch.zeros((4, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match="edge_index"):
        no_c_calls.TorchGraph(torch.zeros(4, dtype=torch.int32), QQ, 3, 1)            # 1-D
    with pytest.raises(ValueError, match="edge_index"):
        no_c_calls.TorchGraph(torch.zeros((2, 4), dtype=torch.int32), QQ, 3, 1)       # (2, m)
    with pytest.raises(ValueError, match="QQ"):
        no_c_calls.TorchGraph(torch.zeros((4, 2), dtype=torch.int32), QQ[:3], 3, 1)   # m differs
    with pytest.raises(ValueError, match="QQ"):
        no_c_calls.TorchGraph(torch.zeros((4, 2), dtype=torch.int32), QQ.t()[:, :3], 3, 1)


def test_stride_tuples():
    from irotavg_amd import torch_api
    m = 10
    assert torch_api.matrix_strides(torch.zeros((m, 4), dtype=torch.float64)) == (4, 1)           # contiguous: AoS
    assert torch_api.matrix_strides(torch.zeros((4, m + 6), dtype=torch.float64)[:, :m].t()) == (1, m + 6)  # planes, ld > m
    assert torch_api.matrix_strides(torch.zeros((m, 6), dtype=torch.float64)[:, 1:5]) == (6, 1)   # a column slice
    assert torch_api.matrix_strides(torch.zeros((2 * m, 8), dtype=torch.float64)[::2, 2:6]) == (16, 1)
    with pytest.raises(ValueError):
        torch_api.matrix_strides(torch.zeros(4, dtype=torch.float64))
