"""The boolean metrics (jaccard, dice, sokalsneath, matching, rogerstanimoto, sokalmichener, kulsinski, russellrao, yule) without a
GPU: names, codes and the header's enumeration; the corrections against the fixture the reference wrote; the float64 conversion
of csrc/metric.h, compiled into a stand-alone host program, against the numpy formulas on every count tuple with d <= 12; the
refusals.  The GPU side is tests/test_gpu_boolean_metrics.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from pynndescent_amd import NNDescent, _capi, exact_knn, nn_descent
from pynndescent_amd import nndescent as N
from tests import boolean_util as BU

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pynndescent_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")


def test_names_resolve_and_codes_agree_with_the_header():
    header = open(os.path.join(ROOT, "include", "pynnd_amd.h")).read()
    enum = dict((name.lower(), int(v)) for name, v in re.findall(r"NND_METRIC_([A-Z]+) = (\d+)", header) if int(v) >= 8)
    assert enum == BU.CODES == _capi.BOOLEAN_METRIC_CODES
    assert sorted(BU.CODES.values()) == list(range(8, 17))  # 7 stays unknown: tests/test_plan_cpu.py pins that refusal
    assert not re.findall(r"#define NND_METRIC_(JACCARD|DICE|YULE|MATCHING)", header)  # an enumeration, not #define lines
    assert int(re.search(r"#define NND_ABI_VERSION (\d+)", header).group(1)) == 6
    for name, code in BU.CODES.items():
        m = N._metric_record(name)
        assert m is N._metric_of(name) is N._BOOLEAN_METRICS[name]
        assert m.code == code == _capi.metric_code(name) and m.boolean and not (m.uint8 or m.linear or m.proxy or m.normalize)
        assert m.angular == (name in ("jaccard", "dice"))  # what the reference reports (pynndescent_.py:1075-1086)
        assert (m.device_kind == _capi.NND_CORRECT_COPY) == (name != "jaccard")


def test_the_metric_table_is_untouched():
    assert sorted(N._METRICS) == sorted(["euclidean", "l2", "sqeuclidean", "cosine", "dot", "inner_product", "correlation",
                                          "hellinger", "proxy_inner_product"])
    assert not set(BU.METRICS) & (set(N._METRICS) | set(N._LINEAR_METRICS) | set(_capi.METRIC_CODES))


def test_corrections_reproduce_the_fixtures():
    g = BU.golden()
    for seed in BU.SEEDS:
        dist = g["jaccard_dist_%d" % seed]
        want = g["jaccard_corrected_%d" % seed]
        got = N._BOOLEAN_METRICS["jaccard"].correction(dist)
        # float64 like the reference's ufunc; its pow is the C library's, element by element, numpy's is vectorised: the two may
        # differ in the last bit of 2^-v, one ulp of a value in (0.5, 1], so 2^-53 .. 2^-52 of the difference from 1
        assert got.dtype == np.float64 and np.abs(got - want).max() <= 2.0 ** -52
        assert np.array_equal(BU.correct("jaccard", dist), got)
        assert (want[np.isinf(dist)] == 1.0).all()
        # FLT_MAX, which the kernels have where the reference has +inf, corrects to exactly 1 too
        assert (N._BOOLEAN_METRICS["jaccard"].correction(np.float32([BU.FLT_MAX])) == 1.0).all()
    for name in BU.RATIONAL:
        d = g["%s_dist_%d" % (name, BU.SEEDS[0])]
        got = N._BOOLEAN_METRICS[name].correction(d)
        assert got is not d and np.array_equal(got, d)


def test_fixture_distances_are_the_numpy_formulas():
    """The helper's float64 formulas against what the reference itself computed (float32 in its heaps)."""
    g = BU.golden()
    x = g["x"]
    for name in BU.METRICS:
        idx, dist = g["%s_idx_%d" % (name, BU.SEEDS[0])].astype(np.int64), g["%s_dist_%d" % (name, BU.SEEDS[0])]
        ok = idx >= 0
        want = BU.dist_pairs(name, x[:, None, :], x[np.maximum(idx, 0)])
        ref = np.where(np.isinf(dist), BU.FLT_MAX, dist.astype(np.float64))
        assert np.allclose(ref[ok], want[ok], rtol=1e-6, atol=0.0), name
        assert float(g["%s_recall_%d" % (name, BU.SEEDS[0])]) >= 0.9


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_float64_twin_equals_numpy_on_every_count_tuple(tmp_path):
    exe = str(tmp_path / "boolean_cpu")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "boolean_cpu.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, "metric.h must compile with the plain host compiler (no HIP headers):\n" + r.stderr
    r = subprocess.run([exe, "12"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines()]
    code, c, a, b, d = (np.array([int(t[i]) for t in rows], np.float64) for i in range(5))
    got = np.array([float.fromhex(t[5]) for t in rows])
    per_code = sum(1 for dd in range(1, 13) for aa in range(dd + 1) for bb in range(dd + 1)
                   for cc in range(max(0, aa + bb - dd), min(aa, bb) + 1))
    assert len(rows) == 9 * per_code
    for name, cd in BU.CODES.items():
        sel = code == cd
        want = BU.dist_from_counts(name, c[sel], a[sel], b[sel], d[sel])
        assert np.isfinite(got[sel]).all() and (got[sel] >= 0.0).all()
        if name == "jaccard":  # log2 is the C library's there and numpy's here
            assert np.array_equal(got[sel] == BU.FLT_MAX, want == BU.FLT_MAX)
            assert np.allclose(got[sel], want, rtol=4e-16, atol=0.0)
        else:
            assert np.array_equal(got[sel], want), name
        same = (c[sel] == a[sel]) & (a[sel] == b[sel])
        assert (got[sel][same] == 0.0).all(), name  # equal indicator rows are at distance 0 under all nine


def test_refusals():
    x = BU.random_rows(64, 8, 1)
    for name in BU.METRICS:
        with pytest.raises(ValueError, match="Not uint8 quantization version of " + name):
            NNDescent(x, metric=name, n_neighbors=5, quantization="uint8")
        with pytest.raises(NotImplementedError, match="on one GPU"):
            NNDescent(x, metric=name, n_neighbors=5, n_devices=2)
    for name in ("manhattan", "true_angular", "hamming", "bit_jaccard"):
        with pytest.raises(NotImplementedError) as e:
            NNDescent(x, metric=name, n_neighbors=5)
        assert "mahalanobis" in str(e.value) and "use pynndescent.NNDescent" in str(e.value) and "jaccard" in str(e.value)
        with pytest.raises(NotImplementedError):
            exact_knn(x, k=3, metric=name)
    with pytest.raises(ValueError):
        NNDescent(x, metric="no_such_metric", n_neighbors=5)
    with pytest.raises(NotImplementedError):
        nn_descent(x, 5, np.array([1, 2, 3], np.int64), dist="hamming", leaf_array=np.zeros((1, 4), np.int32))
    assert {"jaccard", "alternative_jaccard", "yule"} <= set(N._ND_DISTS)
