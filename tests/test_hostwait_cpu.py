"""The host's half of the completion protocol (irotavg_amd/csrc/hostwait.hpp), the host arithmetic of the window
kernels (winbatch.hpp) and the route decision of the banded direct solver (bcr_route.hpp) without a device: the
stand-alone programs under tools/ are built with AddressSanitizer and
UndefinedBehaviorSanitizer and run as child processes. Nothing is preloaded and nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-g", "-O2", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-I", os.path.join(ROOT, "irotavg_amd", "csrc")]


@pytest.fixture(scope="module")
def sanitizer_runtime(tmp_path_factory):
    """skips only where g++ cannot link a program with the two sanitizers"""
    d = tmp_path_factory.mktemp("probe")
    src = d / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++", *FLAGS, str(src), "-o", str(d / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("g++ lacks the ASan / UBSan runtime: " + r.stderr.strip().splitlines()[-1])


@pytest.mark.parametrize("name,says", [("hostwait_check", "hostwait check ok"), ("winbatch_host_check", "winbatch host check ok"),
                                       ("bcr_route_host_check", "bcr route host check ok")])
def test_host_check_is_clean_under_asan_and_ubsan(sanitizer_runtime, tmp_path, name, says):
    exe = str(tmp_path / name)
    r = subprocess.run(["g++", *FLAGS, os.path.join(ROOT, "tools", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and says in r.stdout and not r.stderr, (r.returncode, r.stdout, r.stderr)
