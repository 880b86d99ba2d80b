"""irotavg_window_solve_batch_dev and torch_api.window_solve_batch without a GPU: the symbol, the argument checks that run
before any device is touched, the front-end's own checks, and the packing offsets it derives from `sizes`."""
import ctypes as C

import numpy as np
import pytest
import torch

from irotavg_amd import capi

NAME = "irotavg_window_solve_batch_dev"
# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE_I, FAKE_QQ, FAKE_Q, FAKE_W = (C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000))
GOOD = [(12, 2, 40), (320, 256, 640), (2, 1, 1)]


def call(sizes, nb=None, I=FAKE_I, QQ=FAKE_QQ, qq=(4, 1), Q=FAKE_Q, q=(4, 1), cost=4, kernel=0, w=FAKE_W, null_sizes=False):
    s = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 3)
    res = np.full((max(len(s), 1), 4), -99, dtype=np.int32)
    rc = capi.lib().irotavg_window_solve_batch_dev(
        len(s) if nb is None else nb, None if null_sizes else s.ctypes.data_as(C.POINTER(C.c_int32)), I, QQ, qq[0], qq[1],
        Q, q[0], q[1], cost, 0.1, 5, 5, 1e-3, w, res.ctypes.data_as(C.POINTER(C.c_int32)), kernel, None)
    assert (res == -99).all()
    return rc


def test_the_symbol_is_exported_and_listed():
    assert NAME in capi.SYMBOLS
    assert hasattr(capi.lib(), NAME) and getattr(capi.lib(), NAME).argtypes is not None


@pytest.mark.parametrize("bad", [(66, 1, 100), (321, 300, 100), (70, 6, 641), (20, 20, 30), (20, 1, 0), (20, -1, 30),
                                 (0, 0, 5), (-3, 0, 5), (20, 21, 30), (2 ** 31 - 1, 2 ** 31 - 2, 5), (5, 1, -2)])
def test_a_problem_outside_the_limits_is_a_bad_argument(bad):
    assert call(GOOD[:2] + [bad] + GOOD[2:]) == capi.ERR_BAD_ARG


def test_counts_kernels_costs_and_pointers():
    assert call(GOOD, nb=0) == capi.ERR_BAD_ARG
    assert call(GOOD, nb=-1) == capi.ERR_BAD_ARG
    assert call(GOOD, nb=262145) == capi.ERR_BAD_ARG           # above the documented cap (sizes is not read)
    assert call(GOOD, null_sizes=True) == capi.ERR_BAD_ARG
    assert call(GOOD, kernel=3) == capi.ERR_BAD_ARG
    assert call(GOOD, kernel=-1) == capi.ERR_BAD_ARG
    assert call(GOOD, kernel=2) == capi.ERR_BAD_ARG            # (320, 256, 640) does not fit the wave kernel
    assert call([(18, 1, 40)], kernel=2) == capi.ERR_BAD_ARG   # 17 free views
    assert call(GOOD, cost=14) == capi.ERR_UNKNOWN_COST
    assert call(GOOD, cost=-1) == capi.ERR_UNKNOWN_COST
    for kw in (dict(I=None), dict(QQ=None), dict(Q=None)):
        assert call(GOOD, **kw) == capi.ERR_BAD_ARG
    for kw in (dict(I=C.c_void_p(0x10004)), dict(QQ=C.c_void_p(0x20004)), dict(Q=C.c_void_p(0x30004)),
               dict(w=C.c_void_p(0x40004))):
        assert call(GOOD, **kw) == capi.ERR_BAD_ARG            # not 8-byte aligned


@pytest.mark.parametrize("rs,cs", [(0, 0), (0, 1), (4, 0), (1, 1), (2, 1), (3, 1), (1, 2), (1, 99), (-2, 1), (2, 3),
                                   (2 ** 40, 1), (-2 ** 63, 1), (1, -2 ** 63)])
def test_strides_that_alias_are_bad_arguments(rs, cs):
    """sum m = 681 rows of QQ, sum n_total = 334 rows of Q"""
    assert call(GOOD, qq=(rs, cs)) == capi.ERR_BAD_ARG
    assert call(GOOD, q=(rs, cs)) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kernel,sizes", [(0, GOOD), (1, GOOD), (2, [GOOD[0], GOOD[2]])])
@pytest.mark.parametrize("rs,cs", [(4, 1), (1, 681), (6, 1), (-4, 1), (1, -700), (4, -1), (2 ** 31, 1)])
def test_a_well_formed_call_needs_a_device(kernel, sizes, rs, cs):
    """the pattern of test_compute_entry_points_fail_loudly_without_a_device: where a device exists the made-up addresses
    are the next thing to be refused, which the GPU suite covers"""
    if capi.lib().irotavg_device_count() > 0:
        pytest.skip("a HIP device exists")
    assert call(sizes, kernel=kernel, qq=(rs, cs), q=(rs, cs)) == capi.ERR_NO_DEVICE
    assert call(sizes, kernel=kernel, qq=(rs, cs), q=(rs, cs), w=None) == capi.ERR_NO_DEVICE


# ---- the torch front-end -------------------------------------------------------------------------------------------------
@pytest.fixture
def no_c_calls(monkeypatch):
    """Any use of the C library from here on is an error."""
    from irotavg_amd import torch_api

    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    return torch_api


def tensors(m=41, n=14):
    return (torch.zeros((m, 2), dtype=torch.int32), torch.zeros((m, 4), dtype=torch.float64),
            torch.zeros((n, 4), dtype=torch.float64))


SIZES = np.array([(12, 2, 40), (2, 1, 1)])


def test_wrapper_rejects_cpu_tensors_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    with pytest.raises(TypeError, match="ROCm device"):
        no_c_calls.window_solve_batch(SIZES, ei, QQ, Q)
    with pytest.raises(TypeError):
        no_c_calls.window_solve_batch(SIZES, ei.numpy(), QQ, Q)


def test_wrapper_rejects_wrong_dtypes_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    with pytest.raises(TypeError, match="float64"):
        no_c_calls.window_solve_batch(SIZES, ei, QQ.float(), Q)
    with pytest.raises(TypeError, match="float64"):
        no_c_calls.window_solve_batch(SIZES, ei, QQ, Q.float())
    with pytest.raises(TypeError, match="int32"):
        no_c_calls.window_solve_batch(SIZES, ei.to(torch.int16), QQ, Q)
    with pytest.raises(TypeError, match="integers"):
        no_c_calls.window_solve_batch(SIZES.astype(np.float64), ei, QQ, Q)


def test_wrapper_rejects_wrong_shapes_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    with pytest.raises(ValueError, match="sizes"):
        no_c_calls.window_solve_batch(SIZES.ravel(), ei, QQ, Q)
    with pytest.raises(ValueError, match="sizes"):
        no_c_calls.window_solve_batch(SIZES[:, :2], ei, QQ, Q)
    with pytest.raises(ValueError, match="edge_index"):
        no_c_calls.window_solve_batch(SIZES, ei[:-1], QQ, Q)                 # sum m differs
    with pytest.raises(ValueError, match="edge_index"):
        no_c_calls.window_solve_batch(SIZES, ei.t(), QQ, Q)
    with pytest.raises(ValueError, match="QQ"):
        no_c_calls.window_solve_batch(SIZES, ei, QQ[:, :3], Q)
    with pytest.raises(ValueError, match="Q must"):
        no_c_calls.window_solve_batch(SIZES, ei, QQ, Q[:-1])                 # sum n_total differs


def test_offsets_are_the_cumulative_sums_of_sizes():
    from irotavg_amd import torch_api
    rng = np.random.default_rng(5)
    nv = rng.integers(2, 321, size=500)
    sizes = np.stack([nv, rng.integers(0, nv), rng.integers(1, 641, size=500)], 1)
    s32, eoff, voff, sum_m, sum_n = torch_api.batch_offsets(sizes)
    assert s32.dtype == np.int32 and s32.flags.c_contiguous and (s32 == sizes).all()
    np.testing.assert_array_equal(eoff, np.cumsum(sizes[:, 2]) - sizes[:, 2])
    np.testing.assert_array_equal(voff, np.cumsum(sizes[:, 0]) - sizes[:, 0])
    assert (sum_m, sum_n) == (sizes[:, 2].sum(), sizes[:, 0].sum())
    assert (eoff[0], voff[0]) == (0, 0)
    # int64 sums: 262144 problems at the limits do not fit the int32 the sizes themselves travel in
    big = np.tile(np.array([[320, 256, 640]], dtype=np.int32), (262144, 1))
    _, eo, vo, sm, sn = torch_api.batch_offsets(big)
    assert sm == 262144 * 640 and sn == 262144 * 320 and eo[-1] == 262143 * 640 and eo.dtype == np.int64
    _, eo, vo, sm, sn = torch_api.batch_offsets(torch.tensor(sizes))         # a host tensor is a host array
    assert sm == sum_m and vo[-1] == voff[-1]
