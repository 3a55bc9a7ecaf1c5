"""The plan of a handle (pynndescent_amd/csrc/plan.h) on a CPU: the header is compiled by the plain host compiler, without HIP
headers, under AddressSanitizer / UBSan (plan_cpu.cpp), and the padded widths, table capacities and routing-forest geometry it
derives are pinned to figures worked out by hand from the expressions nnd_create has always used:

  dp = ceil32(dim), ks = ceil16(k), mcp = 16 / 32 / 64 / 128 by max_candidates (32 at least when ks > 64), rcap = 32 / 64 / 128,
  pcap = 64, join_blocks = (k <= 64 ? 1 : ceil(k / 32)) * (mc > 64 ? 2 : 1) when left to the library;
  P = trees * n, max_segs = P // (leaf + 1) + trees + 8;
  routing (graph handle, n >= 131072, dp <= 256): s_m = n // 16, node_cap = trees * s_m // 6 + 4 * trees + 64,
  cell_cap = node_cap + trees, max_segs += cell_cap.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pynndescent_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

BENCH = dict(dp=128, ks=16, mcp=16, rcap=32, pcap=64, join_blocks=1, jb_auto=1, s_stride=16, s_m=62500, cell_leaf=24, early_stop=0,
             node_cap=83429, cell_cap=83437, P=8000000, max_segs=214600)
PLANS = {
    "bench": BENCH,                                                     # n 1 000 000, dim 128, k 15, mc 15, 8 trees, leaf 60
    "route_edge": dict(dp=32, s_m=8192, node_cap=2802, cell_cap=2804, max_segs=11270, routes=1),   # n 131 072, dim 8, k 10, mc 10, 2 trees, leaf 30
    "route_below": dict(s_m=0, max_segs=8466, routes=0),                # the same with n 131 071
    "route_wide_rows": dict(dp=288, s_m=0, routes=0),                   # n 200 000, dim 257
    "route_no_graph": dict(s_m=0, routes=0),                            # bench with NND_FLAG_NO_GRAPH
    "wide_k": dict(ks=80, mcp=32, rcap=32, join_blocks=3),              # k 70, mc 10
    "wide_k_mc": dict(mcp=128, rcap=128, join_blocks=6),                # k 70, mc 65
    "mc_16": dict(mcp=16, rcap=32),
    "mc_17": dict(mcp=32, rcap=32),
    "mc_32": dict(mcp=32, rcap=32),
    "mc_33": dict(mcp=64, rcap=64),
    "mc_64": dict(mcp=64, rcap=64),
    "mc_65": dict(mcp=128, rcap=128),
    "explicit_jb": dict(join_blocks=5, jb_auto=0),
    "shard": dict(own_lo=400, own_hi=1000, n_ranks=2, slim=1),          # n 1000, bounds {0, 400, 1000}, rank 1
    "shard_one_rank": dict(own_lo=0, own_hi=1000, n_ranks=1, slim=0),
}
BAD_BOUNDS = "nnd_create: bad shard bounds (need 1 <= n_ranks <= 64, bounds from 0 to n)"
REFUSALS = {
    "bad_n": "nnd_create: need n >= 1 and dim >= 1 (got n=0 dim=8)",
    "bad_dim": "nnd_create: need n >= 1 and dim >= 1 (got n=1000 dim=0)",
    "bad_metric": "nnd_create: unknown metric 7",
    "bad_k_low": "nnd_create: n_neighbors must be in 1..256 (got 0)",
    "bad_k_high": "nnd_create: n_neighbors must be in 1..256 (got 257)",
    "bad_mc_low": "nnd_create: max_candidates must be in 1..128 (got 0)",
    "bad_mc_high": "nnd_create: max_candidates must be in 1..128 (got 129)",
    "bad_trees": "nnd_create: bad n_trees (0..4096) / leaf_size",
    "bad_leaf": "nnd_create: bad n_trees (0..4096) / leaf_size",
    "bad_n_int32": "nnd_create: n too large for int32 ids",
    "bad_positions": "nnd_create: n_trees * n = 2147483632 exceeds the forest's int32 position space (2^31)",  # 16 trees x 134 217 727
    "bad_bounds_start": BAD_BOUNDS,
    "bad_bounds_falling": "nnd_create: shard bounds must not decrease",
    "bad_bounds_end": BAD_BOUNDS,
    "bad_ranks": BAD_BOUNDS,                                            # 65 ranks
}


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_cpu")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "plan_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "plan.h must compile with the plain host compiler (no HIP headers):\n" + r.stderr
    return exe


def _run(exe, case):
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0:abort_on_error=0")
    r = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("case", sorted(PLANS))
def test_plan_fields(plan_exe, case):
    got = {name: int(value) for name, value in (ln.split() for ln in _run(plan_exe, case).splitlines())}
    print(case, got)
    assert {name: got[name] for name in PLANS[case]} == PLANS[case]


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_plan_refusals(plan_exe, case):
    assert _run(plan_exe, case).splitlines() == ["refused 1", REFUSALS[case]]
