"""irotavg_window_init_mst_batch_dev and torch_api.window_init_mst_batch (docs/window_init_batch.md) without a GPU: the
symbol, the argument checks that run before any device is touched, the front-end's own checks, and the stand-alone program
that holds the parallel restatement of the sweep (irotavg_amd/csrc/winmst.hpp) against the sequential one under
AddressSanitizer and UndefinedBehaviorSanitizer. Nothing is preloaded and nothing sanitized is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from irotavg_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "irotavg_window_init_mst_batch_dev"
# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE_I, FAKE_QQ, FAKE_Q = (C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000))
GOOD = [(12, 2, 40), (320, 256, 640), (2, 1, 1)]


def call(sizes, nb=None, I=FAKE_I, QQ=FAKE_QQ, qq=(4, 1), Q=FAKE_Q, q=(4, 1), null_sizes=False):
    s = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 3)
    res = np.full(max(len(s), 1), -99, dtype=np.int32)
    rc = capi.lib().irotavg_window_init_mst_batch_dev(
        len(s) if nb is None else nb, None if null_sizes else s.ctypes.data_as(C.POINTER(C.c_int32)), I, QQ, qq[0], qq[1],
        Q, q[0], q[1], res.ctypes.data_as(C.POINTER(C.c_int32)), None)
    assert (res == -99).all()                                      # refused before any problem ran
    return rc


def no_device():
    """with a device the made-up addresses are the next thing to be refused, still before any kernel"""
    return capi.ERR_NO_DEVICE if capi.lib().irotavg_device_count() <= 0 else capi.ERR_BAD_ARG


def test_the_symbol_is_exported_listed_and_declared():
    assert NAME in capi.SYMBOLS
    assert hasattr(capi.lib(), NAME) and getattr(capi.lib(), NAME).argtypes is not None
    assert len(getattr(capi.lib(), NAME).argtypes) == 11
    header = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)


def test_counts_and_pointers():
    assert call(GOOD, nb=0) == capi.ERR_BAD_ARG
    assert call(GOOD, nb=-1) == capi.ERR_BAD_ARG
    assert call(GOOD, nb=262145) == capi.ERR_BAD_ARG               # above the documented cap (sizes is not read)
    assert call(GOOD, null_sizes=True) == capi.ERR_BAD_ARG
    for kw in (dict(I=None), dict(QQ=None), dict(Q=None)):
        assert call(GOOD, **kw) == capi.ERR_BAD_ARG
    for kw in (dict(I=C.c_void_p(0x10004)), dict(QQ=C.c_void_p(0x20004)), dict(Q=C.c_void_p(0x30004))):
        assert call(GOOD, **kw) == capi.ERR_BAD_ARG                # not 8-byte aligned


@pytest.mark.parametrize("bad", [(12, 0, 40),                      # f = 0: view 0 is the anchor and must be fixed
                                 (12, 12, 40),                     # f = n_total: nothing to initialise
                                 (12, 13, 40), (12, -1, 40),
                                 (66, 1, 100),                     # 65 free views
                                 (321, 300, 100),                  # 321 views
                                 (70, 6, 641),                     # 641 edges
                                 (20, 1, 0), (0, 0, 5), (-3, 1, 5), (5, 1, -2), (2 ** 31 - 1, 2 ** 31 - 2, 5)])
def test_a_problem_outside_the_limits_is_a_bad_argument(bad):
    assert call([bad]) == capi.ERR_BAD_ARG
    assert call(GOOD[:2] + [bad] + GOOD[2:]) == capi.ERR_BAD_ARG


def test_f_of_one_and_the_limits_themselves_are_accepted():
    assert call([(2, 1, 1)]) == no_device()
    assert call([(65, 1, 640)]) == no_device()                     # 64 free views
    assert call([(320, 256, 640)]) == no_device()
    assert call([(320, 319, 1)]) == no_device()


@pytest.mark.parametrize("rs,cs", [(0, 0), (0, 1), (4, 0), (1, 1), (2, 1), (3, 1), (1, 2), (1, 99), (-2, 1), (2, 3),
                                   (2 ** 40, 1), (-2 ** 63, 1), (1, -2 ** 63)])
def test_strides_that_alias_are_bad_arguments(rs, cs):
    """sum m = 681 rows of QQ, sum n_total = 334 rows of Q"""
    assert call(GOOD, qq=(rs, cs)) == capi.ERR_BAD_ARG
    assert call(GOOD, q=(rs, cs)) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("rs,cs", [(4, 1), (1, 681), (6, 1), (-4, 1), (1, -700), (4, -1), (2 ** 31, 1)])
def test_a_well_formed_call_needs_a_device(rs, cs):
    assert call(GOOD, qq=(rs, cs), q=(rs, cs)) == no_device()
    assert call(GOOD, qq=(rs, cs), q=(4, 1)) == no_device()


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
        no_c_calls.window_init_mst_batch(SIZES, ei, QQ, Q)
    with pytest.raises(TypeError):
        no_c_calls.window_init_mst_batch(SIZES, ei.numpy(), QQ, Q)


def test_wrapper_rejects_wrong_dtypes_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    with pytest.raises(TypeError, match="float64"):
        no_c_calls.window_init_mst_batch(SIZES, ei, QQ.float(), Q)
    with pytest.raises(TypeError, match="float64"):
        no_c_calls.window_init_mst_batch(SIZES, ei, QQ, Q.float())
    with pytest.raises(TypeError, match="int32"):
        no_c_calls.window_init_mst_batch(SIZES, ei.to(torch.int16), QQ, Q)
    with pytest.raises(TypeError, match="integers"):
        no_c_calls.window_init_mst_batch(SIZES.astype(np.float64), ei, QQ, Q)


def test_wrapper_rejects_wrong_shapes_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    with pytest.raises(ValueError, match="sizes"):
        no_c_calls.window_init_mst_batch(SIZES.ravel(), ei, QQ, Q)
    with pytest.raises(ValueError, match="sizes"):
        no_c_calls.window_init_mst_batch(SIZES[:, :2], ei, QQ, Q)
    with pytest.raises(ValueError, match="edge_index"):
        no_c_calls.window_init_mst_batch(SIZES, ei[:-1], QQ, Q)                 # sum m differs
    with pytest.raises(ValueError, match="edge_index"):
        no_c_calls.window_init_mst_batch(SIZES, ei.t(), QQ, Q)
    with pytest.raises(ValueError, match="QQ"):
        no_c_calls.window_init_mst_batch(SIZES, ei, QQ[:, :3], Q)
    with pytest.raises(ValueError, match="Q must"):
        no_c_calls.window_init_mst_batch(SIZES, ei, QQ, Q[:-1])                 # sum n_total differs


# ---- the restatement against the sweep, under sanitizers, as a child process ---------------------------------------------
FLAGS = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "irotavg_amd", "csrc")]


def test_winmst_host_check_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "winmst_host_check")
    r = subprocess.run(["g++", *FLAGS, os.path.join(ROOT, "tools", "winmst_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "winmst host check ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)


def test_the_host_sweep_it_must_match_is_the_library_s():
    """the four-edge ordering trap through the library's own irotavg_init_mst: view 3 takes the later duplicate (edge 3,
    sweep 0), which shows in its rotation because the two copies of (2, 3) carry different measurements"""
    I = np.array([(2, 3), (0, 1), (1, 2), (2, 3)], dtype=np.int32)
    rng = np.random.default_rng(3)
    QQ = rng.standard_normal((4, 4))
    QQ /= np.linalg.norm(QQ, axis=1, keepdims=True)
    Q = np.zeros((4, 4))
    Q[0] = (0, 0, 0, 1)

    def qmul(a, b):
        return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                         a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                         a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                         a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])
    Qf, QQf = capi.fmat(Q), capi.fmat(QQ)
    assert capi.lib().irotavg_init_mst(4, 4, capi._d(Qf), 4, capi._d(QQf), 4, capi._i(I), 1) == capi.OK
    want = qmul(QQ[3], qmul(QQ[2], qmul(QQ[1], Q[0])))
    other = qmul(QQ[0], qmul(QQ[2], qmul(QQ[1], Q[0])))
    assert (Qf[3] == want).all() and not (Qf[3] == other).all()
