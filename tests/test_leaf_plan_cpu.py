"""The leaf-seeding table (pynndescent_amd/csrc/leaf_plan.h) on a CPU: the header is compiled by the plain host compiler, without
HIP headers, under AddressSanitizer / UBSan (leaf_plan_cpu.cpp), and what it launches for EVERY pair (k in 1..256, longest run in
2..256) is compared with the host model of the seeding (tests/leaf_reference.py forms): the kernels' names, their order and m_lo.
The launch geometry is pinned to the figures the kernels are written for: one workgroup per leaf (grid.y = 1) of 512 threads,
256 for the four-wave class <4,4,64,true>; a row-block workgroup takes 64 rows, so grid.y = 2 / 3 / 4 for leaves of up to
128 / 160 / 256 points.
"""
import os
import shutil
import subprocess

import pytest

from tests import leaf_reference as LR

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pynndescent_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

KS, RUNS = range(1, 257), range(2, 257)
GEOMETRY = {  # name: (grid.y, threads)
    "k_leaf_join<4,8,64,true>": (1, 512), "k_leaf_join<4,4,64,true>": (1, 256), "k_leaf_join<5,8,64,true>": (1, 512),
    "k_leaf_join<6,8,64,true>": (1, 512), "k_leaf_join<4,8,64>": (1, 512), "k_leaf_join<5,8,64>": (1, 512), "k_leaf_join<6,8,64>": (1, 512),
    "k_leaf_join_sym<6,8>": (1, 512), "k_leaf_join_sym<10,8>": (1, 512),
    "k_leaf_join_rb<8,8>": (2, 512), "k_leaf_join_rb<10,8>": (3, 512), "k_leaf_join_rb<16,8>": (4, 512),
    "k_leaf_join_rb<8,8,true>": (2, 512), "k_leaf_join_rb<10,8,true>": (3, 512), "k_leaf_join_rb<16,8,true>": (4, 512),
}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{(k, longest): [(name, m_lo, grid.y, threads), ...]} as leaf_plan.h states it"""
    exe = str(tmp_path_factory.mktemp("leaf_plan") / "leaf_plan_cpu")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "leaf_plan_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "leaf_plan.h must compile with the plain host compiler (no HIP headers):\n" + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        assert len(w) in (6, 10), ln  # one or two launches
        out[int(w[0]), int(w[1])] = [(w[i], int(w[i + 1]), int(w[i + 2]), int(w[i + 3])) for i in range(2, len(w), 4)]
    return out


def test_every_pair_is_planned(table):
    assert sorted(table) == [(k, m) for k in KS for m in RUNS]


def test_launches_equal_the_model(table):
    """names, order and m_lo of every pair against leaf_reference.forms"""
    bad = [(k, m, [(f.name, f.m_lo) for f in LR.forms(k, m)], [e[:2] for e in table[k, m]])
           for k in KS for m in RUNS if [(f.name, f.m_lo) for f in LR.forms(k, m)] != [e[:2] for e in table[k, m]]]
    assert not bad, "%d pairs differ (k, longest, model, leaf_plan.h), the first: %s" % (len(bad), bad[:3])


def test_launch_geometry(table):
    seen = {e for es in table.values() for e in es}
    assert {e[0] for e in seen} == set(GEOMETRY), "the 15 forms, each reached by some pair"
    assert {(name, gy, threads) for name, _, gy, threads in seen} == {(name,) + g for name, g in GEOMETRY.items()}
