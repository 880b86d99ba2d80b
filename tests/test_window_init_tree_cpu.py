"""irotavg_window_init_tree_batch_dev and torch_api.window_init_tree_batch (docs/window_init_tree_batch.md) without a GPU:
the symbol, the argument checks in front of any device work, the front-end's own checks, and the stand-alone program that
holds the one-thread form of the kernel (wintree.hpp) against Kruskal under ASan and UBSan, as a child process."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from irotavg_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE = dict(I=0x10000, QQ=0x20000, rank=0x30000, Q=0x40000, in_tree=0x50000)
GOOD = [(12, 2, 40), (320, 256, 640), (2, 1, 1)]


def call(sizes, nb=None, qq=(4, 1), q=(4, 1), null_sizes=False, **ptr):
    s = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 3)
    res = np.full(4 * max(len(s), 1), -99, dtype=np.int32)
    p = {k: (None if ptr.get(k, v) is None else C.c_void_p(ptr.get(k, v))) for k, v in FAKE.items()}
    rc = capi.lib().irotavg_window_init_tree_batch_dev(
        len(s) if nb is None else nb, None if null_sizes else s.ctypes.data_as(C.POINTER(C.c_int32)), p["I"], p["QQ"], qq[0],
        qq[1], p["rank"], p["Q"], q[0], q[1], p["in_tree"], res.ctypes.data_as(C.POINTER(C.c_int32)), None)
    assert (res == -99).all()                                      # refused before any problem ran
    return rc


def test_the_symbol_is_listed_and_takes_13_arguments():
    assert "irotavg_window_init_tree_batch_dev" in capi.SYMBOLS          # (tests/test_abi.py holds SYMBOLS to the header)
    assert len(capi.lib().irotavg_window_init_tree_batch_dev.argtypes) == 13


@pytest.mark.parametrize("kw", [dict(nb=0), dict(nb=-1), dict(nb=262145), dict(null_sizes=True),
                                dict(I=None), dict(QQ=None), dict(Q=None),
                                dict(I=0x10004), dict(QQ=0x20004), dict(Q=0x40004),          # not 8-byte aligned
                                dict(rank=0x30002), dict(in_tree=0x50001)])                  # not 4-byte aligned
def test_counts_pointers_and_alignment(kw):
    assert call(GOOD, **kw) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("bad", [(12, 0, 40), (12, 12, 40), (12, 13, 40), (12, -1, 40),   # f = 0: no root; f >= n_total
                                 (66, 1, 100), (321, 300, 100), (70, 6, 641),             # 65 free views, 321 views, 641 edges
                                 (20, 1, 0), (0, 0, 5), (-3, 1, 5), (5, 1, -2)])
def test_a_problem_outside_the_limits_is_a_bad_argument(bad):
    assert call([bad]) == capi.ERR_BAD_ARG
    assert call(GOOD[:2] + [bad] + GOOD[2:]) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("rs,cs", [(0, 0), (4, 0), (1, 1), (3, 1), (1, 99), (-2, 1), (2 ** 40, 1), (-2 ** 63, 1)])
def test_strides_that_alias_are_bad_arguments(rs, cs):
    """sum m = 681 rows of QQ, sum n_total = 334 rows of Q"""
    assert call(GOOD, qq=(rs, cs)) == capi.ERR_BAD_ARG
    assert call(GOOD, q=(rs, cs)) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [dict(), dict(rank=None), dict(in_tree=None), dict(rank=0x30004, in_tree=0x50004),
                                dict(qq=(1, 681), q=(1, -700)), dict(qq=(-4, 1), q=(6, 1))])
def test_a_well_formed_call_needs_a_device(kw):
    """NO_DEVICE comes behind every host-side check, at the limits themselves too (with a device the made-up addresses
    are the next thing to be refused, still before any kernel)"""
    want = capi.ERR_NO_DEVICE if capi.lib().irotavg_device_count() <= 0 else capi.ERR_BAD_ARG
    assert call(GOOD, **kw) == want and call([(65, 1, 640), (320, 319, 1)]) == want


# ---- the torch front-end -------------------------------------------------------------------------------------------------
@pytest.fixture
def api(monkeypatch):
    """torch_api with any use of the C library an error"""
    from irotavg_amd import torch_api

    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    return torch_api


SIZES = np.array([(12, 2, 40), (2, 1, 1)])
EI, QQ, Q = torch.zeros((41, 2), dtype=torch.int32), torch.zeros((41, 4), dtype=torch.float64), torch.zeros((14, 4), dtype=torch.float64)
RANK, TREE = torch.zeros(41, dtype=torch.int32), torch.zeros(41, dtype=torch.int32)


@pytest.mark.parametrize("exc,match,args,kw", [
    (TypeError, "ROCm device", (SIZES, EI, QQ, Q), {}),
    (TypeError, "torch.Tensor", (SIZES, EI.numpy(), QQ, Q), {}),
    (TypeError, "float64", (SIZES, EI, QQ.float(), Q), {}),
    (TypeError, "int32", (SIZES, EI.to(torch.int16), QQ, Q), {}),
    (TypeError, "integers", (SIZES.astype(np.float64), EI, QQ, Q), {}),
    (TypeError, "rank must be", (SIZES, EI, QQ, Q), dict(rank=RANK.double())),
    (TypeError, "in_tree must be", (SIZES, EI, QQ, Q), dict(in_tree=TREE.long())),
    (ValueError, "sizes", (SIZES[:, :2], EI, QQ, Q), {}),
    (ValueError, "edge_index", (SIZES, EI[:-1], QQ, Q), {}),
    (ValueError, "QQ", (SIZES, EI, QQ[:, :3], Q), {}),
    (ValueError, "Q must", (SIZES, EI, QQ, Q[:-1]), {}),
    (ValueError, "rank must have", (SIZES, EI, QQ, Q), dict(rank=RANK.long()[:-1])),
    (ValueError, "in_tree must have", (SIZES, EI, QQ, Q), dict(in_tree=TREE[:-1])),
])
def test_wrapper_checks_come_before_the_c_call(api, exc, match, args, kw):
    with pytest.raises(exc, match=match):
        api.window_init_tree_batch(*args, **kw)


def test_wintree_host_check_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "wintree_host_check")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                        os.path.join(ROOT, "irotavg_amd", "csrc"), os.path.join(ROOT, "tools", "wintree_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "wintree host check ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
