"""The work-item arithmetic of the typed-rows conversion (pynndescent_amd/csrc/convert_index.h: scalar head, aligned vector
body, scalar tail over rows * d elements) on a CPU: the header is compiled by the host compiler into a stand-alone program
(convert_index_cpu.cpp) with the address and undefined-behaviour sanitizers, which walks the items of a sweep of shapes, element
sizes and source misalignments against exact-size buffers."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pynndescent_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")


def test_every_element_is_converted_once_and_in_bounds(tmp_path):
    exe = str(tmp_path / "convert_index_cpu")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "convert_index_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "convert_index.h must compile with the plain host compiler (no HIP headers):\n" + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    m = re.match(r"plans (\d+) elements (\d+) bad (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    print(r.stdout.strip())
    assert r.returncode == 0 and int(m.group(3)) == 0, r.stdout + r.stderr
    assert int(m.group(1)) > 5000 and int(m.group(2)) > 10_000_000
