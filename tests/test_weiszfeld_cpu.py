"""irotavg_weiszfeld, irotavg_weiszfeld_dev and torch_api.weiszfeld (docs/local_sweeps.md) without a GPU: the symbols, the
argument checks that run before any device is touched, the front-end's own checks, weights_from_cemp, and the stand-alone
program that holds the pieces the kernel runs (irotavg_amd/csrc/sweep.hpp) against the definition in sequence under
AddressSanitizer and UndefinedBehaviorSanitizer. Nothing is preloaded and nothing sanitized is loaded into Python."""
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
M, N = 6, 5


def dev_call(m=M, n_total=N, f=1, I=FAKE[0], QQ=FAKE[1], qq=(4, 1), Q=FAKE[2], q=(4, 1), w=FAKE[3], cost=1, sweeps=2, inner=1,
             floor=1e-6):
    step, info = (C.c_double * 2)(-1.0, -2.0), (C.c_int64 * 2)(-1, -2)
    rc = capi.lib().irotavg_weiszfeld_dev(m, n_total, f, I, QQ, qq[0], qq[1], Q, q[0], q[1], w, cost, sweeps, inner, floor, step,
                                          info, None)
    assert list(step) == [-1.0, -2.0] and list(info) == [-1, -2]
    return rc


def host_call(m=M, n_total=N, f=1, ldqq=M, ldq=N, cost=1, sweeps=2, inner=1, floor=1e-6, I=True):
    Ia = np.array([(0, 1), (1, 2), (2, 0), (2, 3), (3, 0), (3, 4)], dtype=np.int32)
    Qa, Q = capi.fmat(np.tile([0, 0, 0, 1.0], (M, 1))), capi.fmat(np.tile([0, 0, 0, 1.0], (N, 1)))
    Q0, step, info = Q.copy(), (C.c_double * 2)(-1.0, -2.0), (C.c_int64 * 2)(-1, -2)
    rc = capi.lib().irotavg_weiszfeld(m, n_total, f, capi._i(Ia) if I else None, capi._d(Qa), ldqq, capi._d(Q), ldq, None, cost,
                                      sweeps, inner, floor, step, info)
    assert (Q == Q0).all() and list(step) == [-1.0, -2.0] and list(info) == [-1, -2]
    return rc


def test_the_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    for name, nargs in (("irotavg_weiszfeld", 15), ("irotavg_weiszfeld_dev", 18)):
        assert name in capi.SYMBOLS and len(getattr(capi.lib(), name).argtypes) == nargs
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
    assert capi.SWEEP_INFO_FIELDS == ("half_edges", "empty_rows")


BAD = [dict(m=0), dict(m=0x40000000), dict(n_total=0), dict(n_total=0x80000000), dict(f=0), dict(f=N + 1), dict(cost=2), dict(cost=-1),
       dict(sweeps=-1), dict(sweeps=1025), dict(inner=0), dict(inner=17), dict(floor=0.0), dict(floor=-1e-6),
       dict(floor=float("nan")), dict(floor=float("inf"))]


@pytest.mark.parametrize("kw", BAD + [dict(I=False), dict(ldqq=M - 1), dict(ldq=N - 1)])
def test_the_host_form_refuses_before_any_device_work(kw):
    assert host_call(**kw) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", BAD + [dict(I=None), dict(QQ=None), dict(Q=None), dict(qq=(1, 1)), dict(q=(1, 1)),
                                      dict(I=C.c_void_p(0x10004)), dict(Q=C.c_void_p(0x30004)), dict(w=C.c_void_p(0x40004))])
def test_the_device_form_refuses_before_any_device_work(kw):
    assert dev_call(**kw) == capi.ERR_BAD_ARG


def test_no_device_arrives_after_the_checks():
    """every well-formed call, the limits themselves included, gets as far as the device"""
    none = capi.lib().irotavg_device_count() <= 0
    if none:
        assert host_call() == host_call(sweeps=0) == host_call(f=N, cost=0, inner=16) == capi.ERR_NO_DEVICE
    for kw in (dict(), dict(sweeps=0), dict(sweeps=2, inner=16, cost=0), dict(w=None), dict(f=N), dict(q=(1, N), qq=(1, M))):
        assert dev_call(**kw) == (capi.ERR_NO_DEVICE if none else capi.ERR_BAD_ARG)   # (a device refuses the made-up addresses)


def test_weights_from_cemp_against_hand_values():
    s = torch.tensor([0.0, 0.5, float("nan"), 2.0], dtype=torch.float64)
    w = torch_api.weights_from_cemp(s, 2.0)
    assert w.dtype == torch.float64 and np.allclose(w.numpy(), [1.0, np.exp(-1.0), 1.0, np.exp(-4.0)], rtol=1e-15)
    with pytest.raises(TypeError, match="float64"):
        torch_api.weights_from_cemp(s.float(), 2.0)
    with pytest.raises(ValueError, match="beta"):
        torch_api.weights_from_cemp(s, -1.0)


def test_the_wrapper_refuses_before_the_c_call(monkeypatch):
    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    ei, QQ, Q = torch.zeros((9, 2), dtype=torch.int32), torch.zeros((9, 4), dtype=torch.float64), torch.zeros((5, 4), dtype=torch.float64)
    for bad in (dict(QQ=QQ.float()), dict(Q=Q.float()), dict(w=torch.zeros(9, dtype=torch.float32)), dict()):
        with pytest.raises(TypeError):                              # (the last one: CPU tensors)
            torch_api.weiszfeld(ei, bad.pop("QQ", QQ), 5, bad.pop("Q", Q), **bad)
    for bad in (dict(QQ=QQ[:-1]), dict(Q=Q[:-1]), dict(n_total=0), dict(f=0), dict(f=6), dict(w=torch.zeros(8, dtype=torch.float64)),
                dict(cost="l05"), dict(sweeps=1025), dict(sweeps=-1), dict(inner=0), dict(inner=17), dict(floor=0.0),
                dict(floor=float("nan"))):
        with pytest.raises(ValueError):
            torch_api.weiszfeld(ei, bad.pop("QQ", QQ), bad.pop("n_total", 5), bad.pop("Q", Q), **bad)


def test_sweep_host_check_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "sweep_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "irotavg_amd", "csrc"), os.path.join(ROOT, "tools", "sweep_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sweep host check ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
