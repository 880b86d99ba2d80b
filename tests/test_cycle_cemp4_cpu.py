"""irotavg_cycle_cemp4, irotavg_cycle_cemp4_dev and torch_api.cycle_cemp4 (docs/cycle_check.md, "Corruption estimates over
four-cycles") without a GPU: the symbols, the argument checks that run before any device is touched, the front-end's own
checks and its default subset, and the stand-alone program that holds the pieces the kernels run
(irotavg_amd/csrc/cemp4.hpp) against the definition in long double under AddressSanitizer and UndefinedBehaviorSanitizer.
Nothing is preloaded and nothing sanitized is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from irotavg_amd import capi, torch_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = [C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000)]   # nothing dereferences them
M = 6
BETA = np.array([1.0, 2.0, 4.0])


def dev_call(m=M, n_total=5, I=FAKE[0], QQ=FAKE[1], qq=(4, 1), s_in=FAKE[2], ne=2, edges=FAKE[3], iters=3, beta=BETA,
             max_records=0, s4=FAKE[4], used=FAKE[5]):
    h = (C.c_int64 * 2)(-1, -2)
    b = None if beta is None else capi._d(np.ascontiguousarray(beta, dtype=np.float64))
    rc = capi.lib().irotavg_cycle_cemp4_dev(m, n_total, I, QQ, qq[0], qq[1], s_in, ne, edges, iters, b, max_records, s4, used,
                                            h, None)
    assert list(h) == [-1, -2]
    return rc


def host_call(m=M, n_total=5, ldqq=M, s_in=True, ne=2, edges=True, iters=3, beta=BETA, max_records=0, I=True):
    Ia = np.array([(0, 1), (1, 2), (2, 0), (2, 3), (3, 0), (3, 4)], dtype=np.int32)
    Qa, sa, ea = capi.fmat(np.tile([0, 0, 0, 1.0], (M, 1))), np.zeros(M), np.array([3, 4], dtype=np.int32)
    s4, used, h = np.full(M, -9.0), np.full(M, -7, dtype=np.int32), (C.c_int64 * 2)(-1, -2)
    b = None if beta is None else capi._d(np.ascontiguousarray(beta, dtype=np.float64))
    rc = capi.lib().irotavg_cycle_cemp4(m, n_total, capi._i(Ia) if I else None, capi._d(Qa), ldqq, capi._d(sa) if s_in else None,
                                        ne, capi._i(ea) if edges else None, iters, b, max_records, capi._d(s4), capi._i(used), h)
    assert (s4 == -9.0).all() and (used == -7).all() and list(h) == [-1, -2]
    return rc


def test_the_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    for name, nargs in (("irotavg_cycle_cemp4", 14), ("irotavg_cycle_cemp4_dev", 16)):
        assert name in capi.SYMBOLS and len(getattr(capi.lib(), name).argtypes) == nargs
        assert re.search(r"\bint\s+%s\s*\(" % name, header)


BAD = [dict(m=0), dict(m=0x40000000), dict(n_total=0), dict(n_total=0x80000000), dict(iters=-1), dict(iters=65),
       dict(beta=None), dict(beta=[1.0, float("nan"), 1.0]), dict(beta=[1.0, 1.0, float("inf")]), dict(beta=[-1e-300, 1.0, 1.0]),
       dict(max_records=-1), dict(ne=-1), dict(ne=0x80000000)]


@pytest.mark.parametrize("kw", BAD + [dict(I=False), dict(ldqq=M - 1), dict(s_in=False), dict(edges=False, ne=M - 1)])
def test_the_host_form_refuses_before_any_device_work(kw):
    assert host_call(**kw) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", BAD + [dict(I=None), dict(QQ=None), dict(qq=(1, 1)), dict(I=C.c_void_p(0x10004)), dict(s_in=None),
                                      dict(edges=None), dict(s_in=C.c_void_p(0x30004)), dict(edges=C.c_void_p(0x40002)),
                                      dict(s4=C.c_void_p(0x50004)), dict(used=C.c_void_p(0x60002))])
def test_the_device_form_refuses_before_any_device_work(kw):
    assert dev_call(**kw) == capi.ERR_BAD_ARG


def test_no_device_arrives_after_the_checks():
    """every well-formed call, the limits themselves included, gets as far as the device"""
    none = capi.lib().irotavg_device_count() <= 0
    if none:
        assert host_call() == host_call(iters=0, beta=None) == host_call(s_in=False, edges=False, ne=M) == capi.ERR_NO_DEVICE
    for kw in (dict(), dict(iters=0, beta=None), dict(iters=64, beta=np.zeros(64)), dict(s4=None, used=None), dict(qq=(1, M)),
               dict(ne=0), dict(s_in=None, edges=None, ne=M)):
        assert dev_call(**kw) == (capi.ERR_NO_DEVICE if none else capi.ERR_BAD_ARG)   # (a device refuses the made-up addresses)


def test_the_wrapper_refuses_before_the_c_call_and_lists_the_nan_edges(monkeypatch):
    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    ei, QQ = torch.zeros((9, 2), dtype=torch.int32), torch.zeros((9, 4), dtype=torch.float64)
    s, e = torch.zeros(9, dtype=torch.float64), torch.tensor([1, 2])
    for bad in (dict(QQ=QQ.float()), dict(s=s.float()), dict(edges=e.float()), dict(s4=torch.zeros(2, dtype=torch.float32)),
                dict(used=torch.zeros(2, dtype=torch.int64)), dict()):
        with pytest.raises(TypeError):                              # (the last one: CPU tensors)
            torch_api.cycle_cemp4(ei, bad.pop("QQ", QQ), 5, bad.pop("s", s), bad.pop("edges", e), **bad)
    for bad in (dict(QQ=QQ[:-1]), dict(n_total=0), dict(s=s[:-1]), dict(edges=e[:0]), dict(edges=e[None]), dict(beta=[1.0] * 65),
                dict(beta=[float("nan")]), dict(beta=[-1.0]), dict(max_records=-1), dict(s4=torch.zeros(3, dtype=torch.float64))):
        with pytest.raises(ValueError):
            torch_api.cycle_cemp4(ei, bad.pop("QQ", QQ), bad.pop("n_total", 5), bad.pop("s", s), bad.pop("edges", e), **bad)
    # edges=None lists the NaN entries of s: none of them is an empty list, two of them fit an s4 of two entries
    with pytest.raises(ValueError, match="at least one entry"):
        torch_api.cycle_cemp4(ei, QQ, 5, s)
    s[[3, 7]] = float("nan")
    with pytest.raises(ValueError, match="s4"):
        torch_api.cycle_cemp4(ei, QQ, 5, s, s4=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(TypeError, match="ROCm device"):
        torch_api.cycle_cemp4(ei, QQ, 5, s, s4=torch.zeros(2, dtype=torch.float64))


def test_cemp4_host_check_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "cemp4_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "irotavg_amd", "csrc"), os.path.join(ROOT, "tools", "cemp4_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cemp4 host check ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
