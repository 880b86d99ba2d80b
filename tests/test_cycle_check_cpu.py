"""irotavg_cycle_check, irotavg_cycle_check_dev and torch_api.cycle_check (docs/cycle_check.md) without a GPU: the symbols,
the argument checks that run before any device is touched, the front-end's own checks, and the stand-alone program that
holds the pieces the kernels run (irotavg_amd/csrc/cycles.hpp) against a brute-force loop over all edge triples under
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
HOST, DEV, GROUP = "irotavg_cycle_check", "irotavg_cycle_check_dev", "irotavg_cycle_check_group"
# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE = [C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000)]
M = 6


def no_device():
    """with a device the made-up addresses are the next thing to be refused, still before any kernel"""
    return capi.ERR_NO_DEVICE if capi.lib().irotavg_device_count() <= 0 else capi.ERR_BAD_ARG


def host_call(m=M, n_total=5, I=True, QQ=True, ldqq=None, threshold=0.1):
    """the host form on real arrays with sentinel-filled outputs, which must come back untouched"""
    Ia = np.array([(0, 1), (1, 2), (2, 0), (2, 3), (3, 0), (3, 4)], dtype=np.int32)
    Qa = capi.fmat(np.tile([0, 0, 0, 1.0], (M, 1)))
    cnt, ok = np.full(M, -7, dtype=np.int32), np.full(M, -8, dtype=np.int32)
    mn = np.full(M, -9.0)
    s = (C.c_int64 * 4)(-1, -2, -3, -4)
    rc = capi.lib().irotavg_cycle_check(m, n_total, capi._i(Ia) if I else None, capi._d(Qa) if QQ else None,
                                        M if ldqq is None else ldqq, threshold, capi._i(cnt), capi._i(ok), capi._d(mn), s)
    assert (cnt == -7).all() and (ok == -8).all() and (mn == -9.0).all() and list(s) == [-1, -2, -3, -4]
    return rc


def dev_call(m=M, n_total=5, I=FAKE[0], QQ=FAKE[1], qq=(4, 1), threshold=0.1, cnt=FAKE[2], ok=FAKE[3], mn=FAKE[4]):
    s = (C.c_int64 * 4)(-1, -2, -3, -4)
    rc = capi.lib().irotavg_cycle_check_dev(m, n_total, I, QQ, qq[0], qq[1], threshold, cnt, ok, mn, s, None)
    assert list(s) == [-1, -2, -3, -4]
    return rc


def test_the_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    for name, nargs in ((HOST, 10), (DEV, 12), (GROUP, 1)):
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name) and len(getattr(capi.lib(), name).argtypes) == nargs
        assert re.search(r"\bint\s+%s\s*\(" % name, header)


@pytest.mark.parametrize("kw", [dict(I=False), dict(QQ=False), dict(m=0), dict(m=-1), dict(m=0x40000000), dict(n_total=0),
                                dict(n_total=-3), dict(n_total=0x80000000), dict(threshold=float("nan")),
                                dict(threshold=-1e-300), dict(threshold=-float("inf")), dict(ldqq=M - 1), dict(ldqq=0)])
def test_the_host_form_refuses_before_any_device_work(kw):
    assert host_call(**kw) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [dict(I=None), dict(QQ=None), dict(m=0), dict(m=-1), dict(m=0x40000000), dict(n_total=0),
                                dict(n_total=0x80000000), dict(threshold=float("nan")), dict(threshold=-0.5),
                                dict(I=C.c_void_p(0x10004)), dict(QQ=C.c_void_p(0x20004)), dict(mn=C.c_void_p(0x50004)),
                                dict(cnt=C.c_void_p(0x30002)), dict(ok=C.c_void_p(0x40001))])
def test_the_device_form_refuses_before_any_device_work(kw):
    assert dev_call(**kw) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("rs,cs", [(0, 0), (0, 1), (4, 0), (1, 1), (2, 1), (3, 1), (1, 2), (1, M - 1), (-2, 1), (2, 3),
                                   (2 ** 40, 1), (-2 ** 63, 1), (1, -2 ** 63)])
def test_strides_that_alias_are_bad_arguments(rs, cs):
    assert dev_call(qq=(rs, cs)) == capi.ERR_BAD_ARG


def test_no_device_arrives_after_the_checks():
    """every well-formed call, the limits themselves included, gets as far as the device"""
    if capi.lib().irotavg_device_count() <= 0:
        assert host_call() == capi.ERR_NO_DEVICE
        assert host_call(threshold=float("inf")) == capi.ERR_NO_DEVICE
        assert host_call(threshold=0.0, ldqq=M + 3) == capi.ERR_NO_DEVICE
    for kw in (dict(), dict(threshold=float("inf")), dict(threshold=0.0), dict(m=0x3fffffff, qq=(4, 1)),
               dict(n_total=0x7fffffff), dict(cnt=None, ok=None, mn=None), dict(cnt=C.c_void_p(0x30004)),
               dict(qq=(1, M)), dict(qq=(6, 1)), dict(qq=(-4, 1)), dict(qq=(1, -700)), dict(qq=(4, -1)), dict(qq=(2 ** 31, 1))):
        assert dev_call(**kw) == no_device()


def test_the_group_width_is_one_of_four():
    L = capi.lib()
    default = L.irotavg_cycle_check_group(0)
    try:
        assert L.irotavg_cycle_check_group(0) == 8             # the default, given back by 0
        for bad in (-1, 1, 4, 12, 24, 128):
            assert L.irotavg_cycle_check_group(bad) == capi.ERR_BAD_ARG
        assert L.irotavg_cycle_check_group(0) == 8             # a refused value changes nothing
        for g in (8, 16, 32, 64):
            capi.cycle_check_group(g)
            assert capi.cycle_check_group(g) == g
    finally:
        L.irotavg_cycle_check_group(default)


# ---- the torch front-end -------------------------------------------------------------------------------------------------
@pytest.fixture
def no_c_calls(monkeypatch):
    """Any use of the C library from here on is an error."""
    from irotavg_amd import torch_api

    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    return torch_api


def tensors(m=9):
    return torch.zeros((m, 2), dtype=torch.int32), torch.zeros((m, 4), dtype=torch.float64)


def test_wrapper_rejects_cpu_tensors_before_the_c_call(no_c_calls):
    ei, QQ = tensors()
    with pytest.raises(TypeError, match="ROCm device"):
        no_c_calls.cycle_check(ei, QQ, 5)
    with pytest.raises(TypeError):
        no_c_calls.cycle_check(ei.numpy(), QQ, 5)
    with pytest.raises(TypeError):
        no_c_calls.cycle_check(ei, QQ.numpy(), 5)


def test_wrapper_rejects_wrong_dtypes_before_the_c_call(no_c_calls):
    ei, QQ = tensors()
    with pytest.raises(TypeError, match="float64"):
        no_c_calls.cycle_check(ei, QQ.float(), 5)
    with pytest.raises(TypeError, match="int32"):
        no_c_calls.cycle_check(ei.to(torch.int16), QQ, 5)
    with pytest.raises(TypeError, match="int32"):
        no_c_calls.cycle_check(ei, QQ, 5, count=torch.zeros(9, dtype=torch.int64))
    with pytest.raises(TypeError, match="float64"):
        no_c_calls.cycle_check(ei, QQ, 5, min_err=torch.zeros(9, dtype=torch.float32))


def test_wrapper_rejects_wrong_shapes_and_values_before_the_c_call(no_c_calls):
    ei, QQ = tensors()
    with pytest.raises(ValueError, match="edge_index"):
        no_c_calls.cycle_check(ei.t(), QQ, 5)
    with pytest.raises(ValueError, match="edge_index"):
        no_c_calls.cycle_check(ei[:0], QQ[:0], 5)
    with pytest.raises(ValueError, match="QQ"):
        no_c_calls.cycle_check(ei, QQ[:-1], 5)
    with pytest.raises(ValueError, match="QQ"):
        no_c_calls.cycle_check(ei, QQ[:, :3], 5)
    with pytest.raises(ValueError, match="ok"):
        no_c_calls.cycle_check(ei, QQ, 5, ok=torch.zeros(8, dtype=torch.int32))
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match="n_total"):
            no_c_calls.cycle_check(ei, QQ, bad)
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            no_c_calls.cycle_check(ei, QQ, 5, threshold=bad)


# ---- the kernels' pieces against the brute force, under sanitizers, as a child process -------------------------------------
FLAGS = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "irotavg_amd", "csrc")]


def test_cycles_host_check_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "cycles_host_check")
    r = subprocess.run(["g++", *FLAGS, os.path.join(ROOT, "tools", "cycles_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cycles host check ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
