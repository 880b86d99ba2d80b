"""irotavg_window_cemp_batch_dev and torch_api.window_cemp_batch (docs/window_cemp_batch.md) without a GPU: the symbol, the
argument checks that run before any device is touched, the front-end's own checks, and the stand-alone program that holds
the kernel's index math (irotavg_amd/csrc/wincemp.hpp) against a literal triple loop under AddressSanitizer and
UndefinedBehaviorSanitizer. Nothing is preloaded and nothing sanitized is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from irotavg_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "irotavg_window_cemp_batch_dev"
# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE_I, FAKE_QQ, FAKE_S, FAKE_U = (C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000))
GOOD = [(12, 2, 40), (320, 256, 640), (2, 1, 1)]
BETA = [2.5, 5.0]


def call(sizes, nb=None, I=FAKE_I, QQ=FAKE_QQ, qq=(4, 1), iters=None, beta=BETA, s=FAKE_S, used=FAKE_U, null_sizes=False):
    sz = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 3)
    res = np.full(3 * max(len(sz), 1), -99, dtype=np.int32)
    b = None if beta is None else np.array(beta, dtype=np.float64)
    rc = capi.lib().irotavg_window_cemp_batch_dev(
        len(sz) if nb is None else nb, None if null_sizes else sz.ctypes.data_as(C.POINTER(C.c_int32)), I, QQ, qq[0], qq[1],
        (0 if b is None else len(b)) if iters is None else iters, None if b is None else capi._d(b), s, used,
        res.ctypes.data_as(C.POINTER(C.c_int32)), None)
    assert (res == -99).all()                                      # refused before any problem ran
    return rc


def no_device():  # (with a device the made-up addresses are the next thing to be refused, still before any kernel)
    return capi.ERR_NO_DEVICE if capi.lib().irotavg_device_count() <= 0 else capi.ERR_BAD_ARG


def test_the_symbol_is_exported_listed_and_declared():
    assert NAME in capi.SYMBOLS
    assert hasattr(capi.lib(), NAME) and len(getattr(capi.lib(), NAME).argtypes) == 12
    header = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)


BAD = [dict(nb=0), dict(nb=-1), dict(nb=262145), dict(null_sizes=True), dict(I=None), dict(QQ=None),
       dict(I=C.c_void_p(0x10004)), dict(QQ=C.c_void_p(0x20004)), dict(s=C.c_void_p(0x30004)), dict(used=C.c_void_p(0x40002)),
       dict(iters=-1), dict(iters=65, beta=[1.0] * 65), dict(iters=2, beta=None), dict(beta=[1.0, float("nan")]),
       dict(beta=[float("inf")]), dict(beta=[1.0, -1e-300])]
BAD += [dict(qq=q) for q in ((0, 0), (0, 1), (4, 0), (1, 1), (2, 1), (3, 1), (1, 99), (-2, 1), (2 ** 40, 1), (1, -2 ** 63))]
# a problem outside the limits, alone and in the middle of a batch
BAD += [dict(sizes=pre + [z] + GOOD[2:]) for z in ((12, 12, 40), (12, -1, 40), (66, 1, 100), (321, 300, 100), (70, 6, 641),
                                                  (20, 1, 0), (0, 0, 5), (-3, 1, 5), (5, 1, -2)) for pre in ([], GOOD[:2])]


@pytest.mark.parametrize("kw", BAD, ids=repr)
def test_counts_pointers_alignment_schedule_strides_and_limits_are_refused_on_the_host(kw):
    assert call(kw.get("sizes", GOOD), **{k: v for k, v in kw.items() if k != "sizes"}) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [dict(), dict(qq=(1, 681)), dict(qq=(6, 1)), dict(qq=(-4, 1)), dict(s=None), dict(used=None),
                                dict(s=None, used=None), dict(beta=[]), dict(beta=None), dict(beta=[0.0] * 64),
                                dict(sizes=[(65, 1, 640)]), dict(sizes=[(12, 0, 40)])])
def test_a_well_formed_call_needs_a_device(kw):
    assert call(kw.get("sizes", GOOD), **{k: v for k, v in kw.items() if k != "sizes"}) == no_device()


# ---- the torch front-end -------------------------------------------------------------------------------------------------
@pytest.fixture
def no_c_calls(monkeypatch):
    """Any use of the C library from here on is an error."""
    from irotavg_amd import torch_api

    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    return torch_api


SIZES = np.array([(12, 2, 40), (2, 1, 1)])


def test_the_wrapper_refuses_before_the_c_call(no_c_calls):
    f = no_c_calls.window_cemp_batch
    ei, QQ = torch.zeros((41, 2), dtype=torch.int32), torch.zeros((41, 4), dtype=torch.float64)
    for kind, match, args, kw in (
            (TypeError, "ROCm device", (SIZES, ei, QQ), {}),
            (TypeError, "torch.Tensor", (SIZES, ei.numpy(), QQ), {}),
            (TypeError, "float64", (SIZES, ei, QQ.float()), {}),
            (TypeError, "int32", (SIZES, ei.to(torch.int16), QQ), {}),
            (TypeError, "integers", (SIZES.astype(np.float64), ei, QQ), {}),
            (TypeError, "float64", (SIZES, ei, QQ), dict(s=torch.zeros(41))),
            (TypeError, "int32", (SIZES, ei, QQ), dict(used=torch.zeros(41, dtype=torch.int64))),
            (ValueError, "sizes", (SIZES.ravel(), ei, QQ), {}),
            (ValueError, "edge_index", (SIZES, ei[:-1], QQ), {}),
            (ValueError, "QQ", (SIZES, ei, QQ[:, :3]), {}),
            (ValueError, "s must", (SIZES, ei, QQ), dict(s=torch.zeros(40, dtype=torch.float64))),
            (ValueError, "beta", (SIZES, ei, QQ), dict(beta=[1.0] * 65)),
            (ValueError, "beta", (SIZES, ei, QQ), dict(beta=[-1.0])),
            (ValueError, "beta", (SIZES, ei, QQ), dict(beta=[float("nan")]))):
        with pytest.raises(kind, match=match):
            f(*args, **kw)


# ---- the index math against the triple loop, under sanitizers, as a child process --------------------------------------------
FLAGS = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "irotavg_amd", "csrc")]


def test_wincemp_host_check_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "wincemp_host_check")
    r = subprocess.run(["g++", *FLAGS, os.path.join(ROOT, "tools", "wincemp_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wincemp host check ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
