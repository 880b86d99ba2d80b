"""irotavg_cycle_cemp, irotavg_cycle_cemp_dev and torch_api.cycle_cemp (docs/cycle_check.md, "Corruption estimates") without
a GPU: the symbols, the argument checks that run before any device is touched, the front-end's own checks and helpers, and
the stand-alone program that holds the pieces the kernels run (irotavg_amd/csrc/cemp.hpp) against the definition in sequence
under AddressSanitizer and UndefinedBehaviorSanitizer. Nothing is preloaded and nothing sanitized is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from irotavg_amd import capi, torch_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = [C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000)]   # look like arrays; nothing dereferences them
M = 6
BETA = np.array([1.0, 2.0, 4.0])


def dev_call(m=M, n_total=5, I=FAKE[0], QQ=FAKE[1], qq=(4, 1), iters=3, beta=BETA, max_records=0, s=FAKE[2], used=FAKE[3]):
    h = (C.c_int64 * 2)(-1, -2)
    b = None if beta is None else capi._d(np.ascontiguousarray(beta, dtype=np.float64))
    rc = capi.lib().irotavg_cycle_cemp_dev(m, n_total, I, QQ, qq[0], qq[1], iters, b, max_records, s, used, h, None)
    assert list(h) == [-1, -2]
    return rc


def host_call(m=M, n_total=5, ldqq=M, iters=3, beta=BETA, max_records=0, I=True):
    Ia = np.array([(0, 1), (1, 2), (2, 0), (2, 3), (3, 0), (3, 4)], dtype=np.int32)
    Qa = capi.fmat(np.tile([0, 0, 0, 1.0], (M, 1)))
    s, used, h = np.full(M, -9.0), np.full(M, -7, dtype=np.int32), (C.c_int64 * 2)(-1, -2)
    b = None if beta is None else capi._d(np.ascontiguousarray(beta, dtype=np.float64))
    rc = capi.lib().irotavg_cycle_cemp(m, n_total, capi._i(Ia) if I else None, capi._d(Qa), ldqq, iters, b, max_records,
                                       capi._d(s), capi._i(used), h)
    assert (s == -9.0).all() and (used == -7).all() and list(h) == [-1, -2]
    return rc


def test_the_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    for name, nargs in (("irotavg_cycle_cemp", 11), ("irotavg_cycle_cemp_dev", 13)):
        assert name in capi.SYMBOLS and len(getattr(capi.lib(), name).argtypes) == nargs
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert capi.CEMP_SUMMARY_FIELDS == ("records", "untested")


BAD = [dict(m=0), dict(m=0x40000000), dict(n_total=0), dict(n_total=0x80000000), dict(iters=-1), dict(iters=65),
       dict(beta=None), dict(beta=[1.0, float("nan"), 1.0]), dict(beta=[1.0, 1.0, float("inf")]), dict(beta=[-1e-300, 1.0, 1.0]),
       dict(max_records=-1)]


@pytest.mark.parametrize("kw", BAD + [dict(I=False), dict(ldqq=M - 1)])
def test_the_host_form_refuses_before_any_device_work(kw):
    assert host_call(**kw) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", BAD + [dict(I=None), dict(QQ=None), dict(qq=(1, 1)), dict(I=C.c_void_p(0x10004)),
                                      dict(s=C.c_void_p(0x30004)), dict(used=C.c_void_p(0x40002))])
def test_the_device_form_refuses_before_any_device_work(kw):
    assert dev_call(**kw) == capi.ERR_BAD_ARG


def test_no_device_arrives_after_the_checks():
    """every well-formed call, the limits themselves included, gets as far as the device"""
    none = capi.lib().irotavg_device_count() <= 0
    if none:
        assert host_call() == host_call(iters=0, beta=None) == host_call(max_records=1) == capi.ERR_NO_DEVICE
    for kw in (dict(), dict(iters=0, beta=None), dict(iters=64, beta=np.zeros(64)), dict(s=None, used=None), dict(qq=(1, M))):
        assert dev_call(**kw) == (capi.ERR_NO_DEVICE if none else capi.ERR_BAD_ARG)   # (a device refuses the made-up addresses)


def test_the_schedule_and_the_rank_against_hand_values():
    assert torch_api.cemp_beta(0) == [] and len(torch_api.cemp_beta()) == 6
    assert np.allclose(torch_api.cemp_beta(3), [8 / np.pi, 16 / np.pi, 32 / np.pi], rtol=1e-15)
    assert np.allclose(torch_api.cemp_beta(3, 1.0, 3.0), [1 / np.pi, 3 / np.pi, 9 / np.pi], rtol=1e-15)
    with pytest.raises(ValueError, match="iters"):
        torch_api.cemp_beta(65)
    s = torch.tensor([0.0, 0.2, 0.2000001, float("nan"), 3.0], dtype=torch.float64)
    rank = torch_api.rank_from_cemp(s, 0.2)
    assert rank.dtype == torch.int32 and rank.tolist() == [0, 0, 2, 1, 2]
    with pytest.raises(TypeError, match="float64"):
        torch_api.rank_from_cemp(s.float(), 0.2)


def test_the_wrapper_refuses_before_the_c_call(monkeypatch):
    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    ei, QQ = torch.zeros((9, 2), dtype=torch.int32), torch.zeros((9, 4), dtype=torch.float64)
    for bad in (dict(QQ=QQ.float()), dict(s=torch.zeros(9, dtype=torch.float32)), dict(used=torch.zeros(9, dtype=torch.int64)), dict()):
        with pytest.raises(TypeError):                              # (the last one: CPU tensors)
            torch_api.cycle_cemp(ei, bad.pop("QQ", QQ), 5, **bad)
    for bad in (dict(QQ=QQ[:-1]), dict(n_total=0), dict(beta=[1.0] * 65), dict(beta=[float("nan")]), dict(beta=[-1.0]),
                dict(beta=[[1.0]]), dict(max_records=-1), dict(s=torch.zeros(8, dtype=torch.float64))):
        with pytest.raises(ValueError):
            torch_api.cycle_cemp(ei, bad.pop("QQ", QQ), bad.pop("n_total", 5), **bad)


def test_cemp_host_check_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "cemp_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "irotavg_amd", "csrc"), os.path.join(ROOT, "tools", "cemp_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "cemp host check ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
