"""The float64 "sums to distance" function of pynndescent_amd/csrc/metric.h (nnd_ref_dist: what k_finalize hands back and the
exact search ranks by) on a CPU: the header is compiled by the host compiler (metric_cpu.cpp, no HIP headers) under
AddressSanitizer and UBSan, fed the float64 sums of row pairs, and compared with the float64 formulas of tests/metric_util.py
(the proxy's: tests/proxy_util.py).  Both sides evaluate the same expression on the same three doubles -- square root and
division are exact to the last bit, only libm's log2 may differ from numpy's -- so a value is within one float32 ulp of the
float64 value rounded to float32, and the special cases (0, 1, FLT_MAX) are equal bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import metric_util as MU
from tests import proxy_util as PU

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pynndescent_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")

FLT_MAX = MU.FLT_MAX
NAMES = {0: "sqeuclidean", 1: "cosine", 2: "dot", 3: "inner_product", 4: "correlation", 5: "hellinger", 6: PU.METRIC}
N_PAIRS = 200

# rows of four columns whose sums hit every special case, and what the kernels' conventions (metric.h) make of them per code
# (None: no special value, the formula applies; hellinger takes no negative entries)
Z = [0.0, 0.0, 0.0, 0.0]
SPECIAL = {
    #                                                          code: 0     1        2        3        4     5        6
    "both rows zero":          (Z, Z,                                {0: 0.0, 1: 0.0, 2: FLT_MAX, 3: FLT_MAX, 4: 0.0, 5: 0.0, 6: FLT_MAX}),
    "one row zero":            (Z, [1.0, 2.0, 0.5, 3.0],             {0: None, 1: FLT_MAX, 2: FLT_MAX, 3: FLT_MAX, 4: 1.0, 5: FLT_MAX, 6: FLT_MAX}),
    "dot = 0":                 ([1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], {0: None, 1: FLT_MAX, 2: FLT_MAX, 3: FLT_MAX, 4: None, 5: FLT_MAX, 6: FLT_MAX}),
    "centred dot = 0":         ([1.0, -1.0, 0.0, 0.0], [0.0, 0.0, 1.0, -1.0], {0: None, 1: FLT_MAX, 2: FLT_MAX, 3: FLT_MAX, 4: 1.0, 6: FLT_MAX}),
    "dot < 0":                 ([1.0, -1.0, 0.0, 0.0], [-1.0, 1.0, 0.0, 0.0], {0: None, 1: FLT_MAX, 2: FLT_MAX, 3: FLT_MAX, 4: None, 6: FLT_MAX}),
    "both rows constant":      ([0.3] * 4, [-2.0] * 4,               {4: 0.0}),
    "one row constant":        ([0.3] * 4, [1.0, 2.0, 0.5, 3.0],     {4: 1.0}),
    "1 / dot above FLT_MAX":   ([1e-20, 0.0, 0.0, 0.0], [1e-20, 0.0, 0.0, 0.0], {0: None, 1: None, 2: None, 3: FLT_MAX, 5: None, 6: None}),
}


def _rows(code):
    """N_PAIRS row pairs of the fixture data of the code's metric (cosine and sqeuclidean: dot's rows, which hold zero rows),
    the zero and constant rows among them."""
    x, _ = MU.metric_data(NAMES[code] if code in (2, 3, 4, 5) else ("inner_product" if code == 6 else "dot"))
    rng = np.random.default_rng(100 + code)
    i, j = rng.integers(0, len(x), N_PAIRS), rng.integers(0, len(x), N_PAIRS)
    marked = [7, 500, 1500, 11, 900, 1200]  # metric_data's zero rows and correlation's constant rows
    i[:6], j[:6] = marked, marked[::-1]
    i[6:12], j[6:12] = marked, rng.integers(0, len(x), 6)
    return x[i].astype(np.float64), x[j].astype(np.float64)


def _sums(code, a, b):
    """(dot, ax, ay) as the kernels accumulate them, in float64: the very sums the reference formulas below take."""
    if code == 0:
        s = ((a - b) ** 2).sum(-1)
        return s, np.zeros_like(s), np.zeros_like(s)
    name = NAMES[code] if code in (4, 5) else "dot"
    ta, tb = MU.transformed(name, a), MU.transformed(name, b)
    if code == 5:
        return (ta * tb).sum(-1), a.sum(-1), b.sum(-1)
    return (ta * tb).sum(-1), (ta * ta).sum(-1), (tb * tb).sum(-1)


def _reference(code, a, b):
    """The float64 distance of every pair, clamped into [0, FLT_MAX] like every distance the kernels rank."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if code == 0:
            r = ((a - b) ** 2).sum(-1)
        elif code == 1:  # alternative_cosine (distances.py:583-630): hellinger's expression on <a,b>, |a|^2, |b|^2
            g, na, nb = (a * b).sum(-1), (a * a).sum(-1), (b * b).sum(-1)
            far = (na == 0.0) | (nb == 0.0) | (g <= 0.0)
            r = np.where((na == 0.0) & (nb == 0.0), 0.0, np.where(far, FLT_MAX, np.log2(np.sqrt(na * nb) / g)))
        elif code == 6:
            r = PU.proxy_pairs(a, b)
        else:
            r = MU.alt_dist_pairs(NAMES[code], a, b)[0]
    return np.clip(r, 0.0, FLT_MAX)


def _cases(code):
    """(labels, a, b, exact): the fixture pairs, then the special cases this code takes; exact[i]: the value that must come
    out bit for bit, nan where the formula applies."""
    a, b = _rows(code)
    labels, exact = ["pair %d" % i for i in range(len(a))], [np.nan] * len(a)
    for label, (ra, rb, want) in SPECIAL.items():
        if code in want:
            for u, v in ((ra, rb), (rb, ra)):  # (the four-column pattern repeated across the row: every property stays)
                a, b = np.vstack([a, np.tile(u, a.shape[1] // 4)]), np.vstack([b, np.tile(v, a.shape[1] // 4)])
                labels.append(label)
                exact.append(np.nan if want[code] is None else want[code])
    return labels, a, b, np.asarray(exact)


@pytest.fixture(scope="module")
def metric_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("metric") / "metric_cpu")
    cmd = [CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(HERE, "metric_cpu.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "metric.h must compile with the plain host compiler (no HIP headers):\n" + r.stderr
    return exe


@pytest.mark.parametrize("code", sorted(NAMES))
def test_sums_to_distance(metric_exe, code):
    labels, a, b, exact = _cases(code)
    dt, ax, ay = _sums(code, a, b)
    text = "".join("%d %s %s %s\n" % (code, float(p).hex(), float(q).hex(), float(r).hex()) for p, q, r in zip(dt, ax, ay))
    # (the sanitizer runtime may not be the first library of the process where something else is preloaded: it still works)
    env = dict(os.environ, ASAN_OPTIONS="verify_asan_link_order=0:detect_leaks=0:abort_on_error=0")
    r = subprocess.run([metric_exe], input=text, capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = np.array([int(w, 16) for w in r.stdout.split()], np.uint32)
    assert len(got) == len(labels)
    want = _reference(code, a, b).astype(np.float32)
    special = ~np.isnan(exact)
    assert np.array_equal(want[special], exact[special].astype(np.float32)), "the float64 formulas disagree with the special-case table"
    assert set(np.unique(want[special])) <= {np.float32(0.0), np.float32(1.0), np.float32(FLT_MAX)}
    # non-negative floats order like their bit patterns: a distance of one ulp is a difference of 1
    off = np.abs(got.astype(np.int64) - want.view(np.uint32).astype(np.int64))
    bad = np.flatnonzero(np.where(special, off > 0, off > 1))
    assert bad.size == 0, [(labels[i], hex(got[i]), float(want[i])) for i in bad[:10]]
