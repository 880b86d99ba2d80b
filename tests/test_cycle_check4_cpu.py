"""irotavg_cycle_check4, irotavg_cycle_check4_dev and torch_api.cycle_check4 (docs/cycle_check.md, "Four-cycles") without a
GPU: the symbols, the argument checks that run before any device is touched, the front-end's own checks, and the
stand-alone program that holds the pieces the kernels run (irotavg_amd/csrc/cycles4.hpp) against the literal reference
under AddressSanitizer and UndefinedBehaviorSanitizer. Nothing is preloaded and nothing sanitized is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from irotavg_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE = [C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000)]
M = 6


def host_call(m=M, n_total=5, I=True, QQ=True, ldqq=M, threshold=0.1, ne=3, edges=True):
    """the host form on real arrays with sentinel-filled outputs, which must come back untouched"""
    Ia = np.array([(0, 1), (1, 2), (2, 3), (3, 0), (3, 4), (4, 0)], dtype=np.int32)
    Qa = capi.fmat(np.tile([0, 0, 0, 1.0], (M, 1)))
    sub = np.array([4, 0, 4], dtype=np.int32)
    cnt, ok, mn = np.full(M, -7, dtype=np.int32), np.full(M, -8, dtype=np.int32), np.full(M, -9.0)
    s = (C.c_int64 * 4)(-1, -2, -3, -4)
    rc = capi.lib().irotavg_cycle_check4(m, n_total, capi._i(Ia) if I else None, capi._d(Qa) if QQ else None, ldqq, threshold,
                                         ne, capi._i(sub) if edges else None, capi._i(cnt), capi._i(ok), capi._d(mn), s)
    assert (cnt == -7).all() and (ok == -8).all() and (mn == -9.0).all() and list(s) == [-1, -2, -3, -4]
    return rc


def dev_call(m=M, n_total=5, I=FAKE[0], QQ=FAKE[1], qq=(4, 1), threshold=0.1, ne=3, edges=FAKE[5], cnt=FAKE[2], ok=FAKE[3],
             mn=FAKE[4]):
    s = (C.c_int64 * 4)(-1, -2, -3, -4)
    rc = capi.lib().irotavg_cycle_check4_dev(m, n_total, I, QQ, qq[0], qq[1], threshold, ne, edges, cnt, ok, mn, s, None)
    assert list(s) == [-1, -2, -3, -4]
    return rc


def test_the_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    for name, nargs in (("irotavg_cycle_check4", 12), ("irotavg_cycle_check4_dev", 14), ("irotavg_cycle_check4_group", 1)):
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name) and len(getattr(capi.lib(), name).argtypes) == nargs
        assert re.search(r"\bint\s+%s\s*\(" % name, header)


SIZES = [dict(m=0), dict(m=0x40000000), dict(n_total=0), dict(n_total=0x80000000), dict(threshold=float("nan")),
         dict(threshold=-1e-300), dict(ne=-1), dict(ne=0x80000000), dict(ne=3, edges=None), dict(ne=M + 1, edges=None)]


@pytest.mark.parametrize("kw", SIZES + [dict(I=False), dict(QQ=False), dict(ldqq=M - 1)])
def test_the_host_form_refuses_before_any_device_work(kw):
    assert host_call(**kw) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", SIZES + [dict(I=None), dict(QQ=None), dict(qq=(1, 1)), dict(qq=(0, 1)),
                                        dict(I=C.c_void_p(0x10004)), dict(QQ=C.c_void_p(0x20004)), dict(mn=C.c_void_p(0x50004)),
                                        dict(cnt=C.c_void_p(0x30002)), dict(ok=C.c_void_p(0x40001)), dict(edges=C.c_void_p(0x60002))])
def test_the_device_form_refuses_before_any_device_work(kw):
    assert dev_call(**kw) == capi.ERR_BAD_ARG


def test_no_device_arrives_after_the_checks():
    """every well-formed call, the limits themselves included, gets as far as the device"""
    have = capi.lib().irotavg_device_count() > 0
    if not have:
        assert host_call() == capi.ERR_NO_DEVICE
        assert host_call(ne=M, edges=False, threshold=float("inf")) == capi.ERR_NO_DEVICE
    for kw in (dict(), dict(ne=M, edges=None), dict(ne=0x7fffffff), dict(ne=0), dict(edges=C.c_void_p(0x60004)),
               dict(cnt=None, ok=None, mn=None), dict(qq=(1, M)), dict(threshold=0.0)):
        assert dev_call(**kw) == (capi.ERR_BAD_ARG if have else capi.ERR_NO_DEVICE)   # (made-up addresses are refused next)


def test_the_group_width_is_one_of_four():
    L = capi.lib()
    default = L.irotavg_cycle_check4_group(0)
    try:
        for bad in (-1, 1, 4, 12, 128):
            assert L.irotavg_cycle_check4_group(bad) == capi.ERR_BAD_ARG
        assert L.irotavg_cycle_check4_group(0) == default            # a refused value changes nothing
        for g in (8, 16, 32, 64):
            capi.cycle_check4_group(g)
            assert capi.cycle_check4_group(g) == g
    finally:
        L.irotavg_cycle_check4_group(default)


def test_the_torch_wrapper_refuses_before_the_c_call(monkeypatch):
    from irotavg_amd import torch_api

    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    ei, QQ = torch.zeros((9, 2), dtype=torch.int32), torch.zeros((9, 4), dtype=torch.float64)
    sub = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(TypeError, match="ROCm device"):
        torch_api.cycle_check4(ei, QQ, 5, edges=sub)
    for kw, exc, what in ((dict(edges=sub.to(torch.int16)), TypeError, "int32"), (dict(edges=sub.numpy()), TypeError, "edges"),
                          (dict(edges=sub.view(3, 1)), ValueError, "edges"), (dict(edges=sub[:0]), ValueError, "edges"),
                          (dict(edges=sub, ok=torch.zeros(9, dtype=torch.int32)), ValueError, "ok"),
                          (dict(count=torch.zeros(9, dtype=torch.int64)), TypeError, "int32"),
                          (dict(min_err=torch.zeros(3)), TypeError, "float64"), (dict(threshold=-0.1), ValueError, "threshold")):
        with pytest.raises(exc, match=what):
            torch_api.cycle_check4(ei, QQ, 5, **kw)
    with pytest.raises(ValueError, match="QQ"):
        torch_api.cycle_check4(ei, QQ[:-1], 5)
    with pytest.raises(ValueError, match="n_total"):
        torch_api.cycle_check4(ei, QQ, 2 ** 31)


def test_cycles4_host_check_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "cycles4_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "irotavg_amd", "csrc"), os.path.join(ROOT, "tools", "cycles4_host_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cycles4 host check ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
