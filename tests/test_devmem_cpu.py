"""The device-memory ownership policy (pynndescent_amd/csrc/devmem.h) on a CPU: the header is compiled by the host compiler
with a counting allocator that can be told to fail (devmem_cpu.cpp) under AddressSanitizer, which judges the double frees."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pynndescent_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

CASES = [
    "alloc_release",      # alloc x 3, release_all: nothing live, each block freed once; a second release_all is a no-op
    "grow_noop",          # need <= cap: no allocator call
    "grow_success",       # the old block goes, the capacity becomes new_cap
    "grow_fail_single",   # (nullptr, 0), no entry; the next grow succeeds
    "grow2_fail_first",   # paired growth, first allocation fails: both null, capacity 0, nothing live
    "grow2_fail_second",  # ... second allocation fails: the first is given back
    "free_then_release",  # free of one pointer, then release_all: no double free
    "biased",             # the working pointer is base - offset: release_all frees the base
    "scratch",            # early return out of a scope frees all; a failed get leaves the earlier ones owned
]


@pytest.fixture(scope="module")
def devmem_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devmem") / "devmem_cpu")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "devmem_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "devmem.h must compile with the plain host compiler (no HIP headers):\n" + r.stderr
    return exe


@pytest.mark.parametrize("case", CASES)
def test_devmem_policy(devmem_exe, case):
    # (the sanitizer runtime may not be the first library of the process where something else is preloaded: it still works;
    # leaks are counted by the fake allocator itself)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0:abort_on_error=0")
    r = subprocess.run([devmem_exe, case], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr
