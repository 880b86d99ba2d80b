"""irotavg_init_tree, irotavg_init_tree_dev and the torch front-end (docs/init_tree.md) without a GPU: the symbols, the
argument checks that run before any device is touched, the front-end's own checks, rank_from_cycle_check on a hand-written
table, and the stand-alone program that holds the steps the kernels run (irotavg_amd/csrc/treeinit.hpp) against Kruskal
and a long-double propagation under AddressSanitizer and UndefinedBehaviorSanitizer. Nothing is preloaded and nothing
sanitized is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from irotavg_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEV, COUNTERS = "irotavg_init_tree", "irotavg_init_tree_dev", "irotavg_init_tree_counters"
# addresses that look like arrays (8-byte aligned, non-NULL); nothing dereferences them before the device check
FAKE = [C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000)]
M, N = 6, 5
INFO = [-1, -2, -3, -4]


def no_device():
    """with a device the made-up addresses are the next thing to be refused, still before any kernel"""
    return capi.ERR_NO_DEVICE if capi.lib().irotavg_device_count() <= 0 else capi.ERR_BAD_ARG


def host_call(m=M, n_total=N, f=1, I=True, QQ=True, ldqq=None, rank=True, Q=True, ldq=None, tree=True):
    """the host form on real arrays with sentinel-filled outputs, which must come back untouched"""
    Ia = np.array([(0, 1), (1, 2), (2, 0), (2, 3), (3, 0), (3, 4)], dtype=np.int32)
    Qa = capi.fmat(np.tile([0, 0, 0, 1.0], (M, 1)))
    rk = np.zeros(M, dtype=np.int32)
    Qv = capi.fmat(np.full((N, 4), -9.0))
    tr = np.full(M, -7, dtype=np.int32)
    s = (C.c_int64 * 4)(*INFO)
    rc = capi.lib().irotavg_init_tree(m, n_total, f, capi._i(Ia) if I else None, capi._d(Qa) if QQ else None,
                                      M if ldqq is None else ldqq, capi._i(rk) if rank else None, capi._d(Qv) if Q else None,
                                      N if ldq is None else ldq, capi._i(tr) if tree else None, s)
    assert (Qv == -9.0).all() and (tr == -7).all() and list(s) == INFO
    return rc


def dev_call(m=M, n_total=N, f=1, I=FAKE[0], QQ=FAKE[1], qq=(4, 1), rank=FAKE[2], Q=FAKE[3], q=(4, 1), tree=FAKE[4]):
    s = (C.c_int64 * 4)(*INFO)
    rc = capi.lib().irotavg_init_tree_dev(m, n_total, f, I, QQ, qq[0], qq[1], rank, Q, q[0], q[1], tree, s, None)
    assert list(s) == INFO
    return rc


def test_the_symbols_are_exported_listed_and_declared():
    header = open(os.path.join(ROOT, "include", "irotavg_hip.h")).read()
    for name, nargs, ret in ((HOST, 11, "int"), (DEV, 14, "int"), (COUNTERS, 1, "void")):
        assert name in capi.SYMBOLS
        assert hasattr(capi.lib(), name) and len(getattr(capi.lib(), name).argtypes) == nargs
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), header)
    from irotavg_amd import torch_api
    assert callable(capi.init_tree) and callable(torch_api.init_tree) and callable(torch_api.rank_from_cycle_check)
    assert callable(torch_api.TorchGraph.init_tree)


@pytest.mark.parametrize("kw", [dict(I=False), dict(QQ=False), dict(Q=False), dict(m=0), dict(m=-1), dict(m=0x80000000),
                                dict(n_total=0), dict(n_total=-3), dict(n_total=0x80000000), dict(f=0), dict(f=-1),
                                dict(f=N + 1), dict(ldqq=M - 1), dict(ldqq=0), dict(ldq=N - 1), dict(ldq=0)])
def test_the_host_form_refuses_before_any_device_work(kw):
    assert host_call(**kw) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("kw", [dict(I=None), dict(QQ=None), dict(Q=None), dict(m=0), dict(m=-1), dict(m=0x80000000),
                                dict(n_total=0), dict(n_total=0x80000000), dict(f=0), dict(f=-2), dict(f=N + 1),
                                dict(I=C.c_void_p(0x10004)), dict(QQ=C.c_void_p(0x20004)), dict(Q=C.c_void_p(0x40004)),
                                dict(rank=C.c_void_p(0x30002)), dict(tree=C.c_void_p(0x50001))])
def test_the_device_form_refuses_before_any_device_work(kw):
    assert dev_call(**kw) == capi.ERR_BAD_ARG


@pytest.mark.parametrize("which", ["qq", "q"])
@pytest.mark.parametrize("rs,cs", [(0, 0), (0, 1), (4, 0), (1, 1), (2, 1), (3, 1), (1, 2), (1, N - 2), (-2, 1), (2, 3),
                                   (2 ** 40, 1), (-2 ** 63, 1), (1, -2 ** 63)])
def test_strides_that_alias_are_bad_arguments(which, rs, cs):
    assert dev_call(**{which: (rs, cs)}) == capi.ERR_BAD_ARG


def test_no_device_arrives_after_the_checks():
    """every well-formed call, the limits themselves included, gets as far as the device"""
    if capi.lib().irotavg_device_count() <= 0:
        assert host_call() == capi.ERR_NO_DEVICE
        assert host_call(rank=False, tree=False, f=N) == capi.ERR_NO_DEVICE
        assert host_call(ldqq=M + 3, ldq=N + 1) == capi.ERR_NO_DEVICE
    for kw in (dict(), dict(m=0x7fffffff), dict(n_total=0x7fffffff), dict(f=N), dict(rank=None, tree=None),
               dict(rank=C.c_void_p(0x30004)), dict(qq=(1, M)), dict(q=(1, N)), dict(qq=(6, 1)), dict(q=(-4, 1)),
               dict(qq=(1, -700)), dict(q=(4, -1)), dict(qq=(2 ** 31, 1))):
        assert dev_call(**kw) == no_device()


def test_the_counters_can_be_read_without_a_device():
    assert capi.init_tree_counters() == (0, 0) or capi.lib().irotavg_device_count() > 0
    capi.lib().irotavg_init_tree_counters(None)  # NULL is ignored


def test_the_host_wrapper_checks_its_shapes():
    I = np.array([(0, 1), (1, 2)], dtype=np.int32)
    QQ, Q = np.tile([0, 0, 0, 1.0], (2, 1)), np.tile([0, 0, 0, 1.0], (3, 1))
    with pytest.raises(ValueError, match="QQ"):
        capi.init_tree(I, QQ[:1], 3, Q)
    with pytest.raises(ValueError, match="Q must"):
        capi.init_tree(I, QQ, 4, Q)
    with pytest.raises(ValueError, match="rank"):
        capi.init_tree(I, QQ, 3, Q, rank=[0, 0, 0])
    if capi.lib().irotavg_device_count() <= 0:
        out = capi.init_tree(I, QQ, 3, Q, allow_rc=(capi.ERR_NO_DEVICE,))
        assert out["rc"] == capi.ERR_NO_DEVICE and out["info"] is None and (out["in_tree"] == -1).all()


# ---- the torch front-end -------------------------------------------------------------------------------------------------
@pytest.fixture
def no_c_calls(monkeypatch):
    """Any use of the C library from here on is an error."""
    from irotavg_amd import torch_api

    def boom():
        raise AssertionError("the C library was reached")
    monkeypatch.setattr(capi, "lib", boom)
    return torch_api


def tensors(m=9, n=5):
    return (torch.zeros((m, 2), dtype=torch.int32), torch.zeros((m, 4), dtype=torch.float64),
            torch.zeros((n, 4), dtype=torch.float64))


def test_wrapper_rejects_cpu_tensors_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    with pytest.raises(TypeError, match="ROCm device"):
        no_c_calls.init_tree(ei, QQ, 5, Q)
    with pytest.raises(TypeError):
        no_c_calls.init_tree(ei.numpy(), QQ, 5, Q)
    with pytest.raises(TypeError):
        no_c_calls.init_tree(ei, QQ.numpy(), 5, Q)
    with pytest.raises(TypeError):
        no_c_calls.init_tree(ei, QQ, 5, Q.numpy())


def test_wrapper_rejects_wrong_dtypes_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    with pytest.raises(TypeError, match="float64"):
        no_c_calls.init_tree(ei, QQ.float(), 5, Q)
    with pytest.raises(TypeError, match="float64"):
        no_c_calls.init_tree(ei, QQ, 5, Q.float())
    with pytest.raises(TypeError, match="int32"):
        no_c_calls.init_tree(ei.to(torch.int16), QQ, 5, Q)
    with pytest.raises(TypeError, match="int32"):
        no_c_calls.init_tree(ei, QQ, 5, Q, rank=torch.zeros(9, dtype=torch.int64))
    with pytest.raises(TypeError, match="int32"):
        no_c_calls.init_tree(ei, QQ, 5, Q, in_tree=torch.zeros(9, dtype=torch.float64))


def test_wrapper_rejects_wrong_shapes_and_values_before_the_c_call(no_c_calls):
    ei, QQ, Q = tensors()
    with pytest.raises(ValueError, match="edge_index"):
        no_c_calls.init_tree(ei.t(), QQ, 5, Q)
    with pytest.raises(ValueError, match="edge_index"):
        no_c_calls.init_tree(ei[:0], QQ[:0], 5, Q)
    with pytest.raises(ValueError, match="QQ"):
        no_c_calls.init_tree(ei, QQ[:-1], 5, Q)
    with pytest.raises(ValueError, match="Q must"):
        no_c_calls.init_tree(ei, QQ, 6, Q)
    with pytest.raises(ValueError, match="Q must"):
        no_c_calls.init_tree(ei, QQ, 5, Q[:, :3])
    with pytest.raises(ValueError, match="rank"):
        no_c_calls.init_tree(ei, QQ, 5, Q, rank=torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="in_tree"):
        no_c_calls.init_tree(ei, QQ, 5, Q, in_tree=torch.zeros(10, dtype=torch.int32))
    for bad in (0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            no_c_calls.init_tree(ei, QQ, bad, torch.zeros((max(bad, 0) if bad < 2 ** 31 else 1, 4), dtype=torch.float64))
    for bad in (0, -1, 6):
        with pytest.raises(ValueError, match="f must"):
            no_c_calls.init_tree(ei, QQ, 5, Q, f=bad)


def test_rank_from_cycle_check_on_a_hand_written_table(no_c_calls):
    #                       supported  supported  untested  contradicted  contradicted  supported (saturated counts)
    count = torch.tensor([3, 1, 0, 1, 7, 2 ** 31 - 1], dtype=torch.int32)
    ok = torch.tensor([1, 1, 0, 0, 0, 2 ** 31 - 1], dtype=torch.int32)
    rank = no_c_calls.rank_from_cycle_check(count, ok)
    assert rank.dtype == torch.int32 and rank.tolist() == [0, 0, 1, 2, 2, 0]
    with pytest.raises(TypeError, match="int32"):
        no_c_calls.rank_from_cycle_check(count.long(), ok)
    with pytest.raises(ValueError, match="tri_ok"):
        no_c_calls.rank_from_cycle_check(count, ok[:-1])


# ---- the kernels' steps against Kruskal and a long-double propagation, under sanitizers, as a child process ------------------
FLAGS = ["-std=c++17", "-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "irotavg_amd", "csrc")]


def test_treeinit_host_check_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "treeinit_host_check")
    r = subprocess.run(["g++", *FLAGS, os.path.join(ROOT, "tools", "treeinit_host_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "treeinit host check ok" in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
