"""The rounding-error bands of the exact search's certificate (pynndescent_amd/csrc/exact_band.h) on a CPU: the header is
compiled by the host compiler, the scan's float32 arithmetic is emulated (exact_band_cpu.cpp: preparation, norm word, the Gram
value as an fmaf chain in the kernel's K order, nnd_gram_to_dist) and |f32 kernel value - float64 value of the raw rows| <= band
is asserted for every pair of 300 query rows and all rows of each set."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.util_data import clustered

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pynndescent_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
N_QUERY = 300


def _bimodal():
    rs = np.random.RandomState(7)
    x = 0.01 * rs.standard_normal((3000, 24))
    return (x + np.where(rs.rand(3000, 1) < 0.5, 1000.0, -1000.0)).astype(np.float32)


def _spread_norms():
    rs = np.random.RandomState(4)
    return (clustered(3000, 24, 6, 24, 5) * np.power(10.0, rs.uniform(-3.0, 3.0, (3000, 1)))).astype(np.float32)


def _unit_extremes(nonneg=False):
    """near-duplicates (a row and copies 1e-4 away) and near-orthogonal rows (iid directions in 130 dimensions)"""
    rs = np.random.RandomState(9)
    base = rs.standard_normal((1000, 130))
    x = np.vstack([base, base[:500] + 1e-4 * rs.standard_normal((500, 130)), base[:500] * 3.0])
    x = x[rs.permutation(x.shape[0])]
    return np.ascontiguousarray(np.abs(x) if nonneg else x, dtype=np.float32)


# name -> (metric code, data)
CASES = {
    "bimodal_sqeuclid": (0, _bimodal),
    "clustered130_sqeuclid": (0, lambda: clustered(3000, 130, 6, 24, 230)),
    "clustered130_cosine": (1, lambda: clustered(3000, 130, 6, 24, 230)),
    "offset1e4_sqeuclid": (0, lambda: clustered(3000, 24, 6, 24, 6) + np.float32(1e4)),
    "offset1e4_correlation": (4, lambda: clustered(3000, 24, 6, 24, 6) + np.float32(1e4)),
    "offset1e4_cosine": (1, lambda: clustered(3000, 24, 6, 24, 6) + np.float32(1e4)),
    "spread_norms_sqeuclid": (0, _spread_norms),
    "spread_norms_inner_product": (3, _spread_norms),
    "spread_norms_cosine": (1, _spread_norms),
    "unit_extremes_cosine": (1, _unit_extremes),
    "unit_extremes_dot": (2, _unit_extremes),
    "unit_extremes_correlation": (4, _unit_extremes),
    "unit_extremes_hellinger": (5, lambda: _unit_extremes(nonneg=True)),
}


@pytest.fixture(scope="module")
def band_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("exact_band") / "exact_band_cpu")
    cmd = [CXX, "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "exact_band_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "exact_band.h must compile with the plain host compiler (no HIP headers):\n" + r.stderr
    return exe


@pytest.mark.parametrize("case", sorted(CASES))
def test_band_covers_the_kernel_arithmetic(band_exe, case, tmp_path):
    metric, make = CASES[case]
    x = np.ascontiguousarray(make(), dtype=np.float32)
    path = str(tmp_path / "x.f32")
    x.tofile(path)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0:abort_on_error=0")
    r = subprocess.run([band_exe, str(metric), str(x.shape[0]), str(x.shape[1]), str(N_QUERY), path], capture_output=True, text=True,
                       env=env, timeout=300)
    m = re.match(r"pairs (\d+) worst (\S+) bad (\d+)", r.stdout)
    assert m, r.stdout + r.stderr
    print(case, r.stdout.strip())
    assert r.returncode == 0 and int(m.group(3)) == 0, "%s: %s pairs exceed the band, worst error / band = %s" % (case, m.group(3), m.group(2))
    assert int(m.group(1)) >= N_QUERY * (x.shape[0] - 10)
