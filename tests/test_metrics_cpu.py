"""dot / inner_product / correlation / hellinger: the host side (constants, corrections, rejected inputs) -- no GPU needed."""
import os
import re

import numpy as np
import pytest

from pynndescent_amd import _capi, nndescent
from tests import metric_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _header_metrics():
    text = open(os.path.join(ROOT, "include", "pynnd_amd.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (NND_METRIC_\w+) (\d+)", text)}


def test_header_metric_codes_match_capi():
    defs = _header_metrics()
    assert defs == {"NND_METRIC_SQEUCLIDEAN": 0, "NND_METRIC_ALT_COSINE": 1, "NND_METRIC_ALT_DOT": 2,
                    "NND_METRIC_ALT_INNER_PRODUCT": 3, "NND_METRIC_CORRELATION": 4, "NND_METRIC_ALT_HELLINGER": 5}
    for name, code in defs.items():
        assert getattr(_capi, name) == code
    assert _capi.METRIC_CODES["dot"] == _capi.NND_METRIC_ALT_DOT
    assert _capi.METRIC_CODES["inner_product"] == _capi.NND_METRIC_ALT_INNER_PRODUCT
    assert _capi.METRIC_CODES["correlation"] == _capi.NND_METRIC_CORRELATION
    assert _capi.METRIC_CODES["hellinger"] == _capi.NND_METRIC_ALT_HELLINGER
    # trees: angular for every unit-row metric, euclidean for inner_product (pynndescent_.py:1075-1095)
    for m in ("dot", "correlation", "hellinger"):
        assert m in nndescent._ANGULAR_METRICS
    assert "inner_product" not in nndescent._ANGULAR_METRICS


@pytest.mark.parametrize("metric", MU.NEW_METRICS)
def test_corrections_reproduce_the_reference(metric):
    f = np.load(os.path.join(GOLDEN, "metric_%s.npz" % metric))
    corr = nndescent._DISTANCE_CORRECTIONS[metric]
    for s in f["seeds"]:
        dist, want = f["dist_%d" % s], f["corrected_%d" % s]
        got = corr(dist)
        assert got.dtype == want.dtype
        assert got is not dist  # a copy, like the other corrections
        np.testing.assert_allclose(got, want, rtol=1e-6)
    if metric == "inner_product":  # FLT_MAX (no positive inner product) -> 0
        assert nndescent._DISTANCE_CORRECTIONS[metric](np.array([np.finfo(np.float32).max], np.float32))[0] == 0.0


@pytest.mark.parametrize("metric", MU.NEW_METRICS)
def test_nn_descent_accepts_the_reference_names(metric):
    alt = {"dot": "alternative_dot", "inner_product": "alternative_inner_product", "correlation": "correlation",
           "hellinger": "alternative_hellinger"}[metric]
    assert nndescent._ND_DISTS[alt] == (_capi.METRIC_CODES[metric], None)
    assert nndescent._ND_DISTS[metric][0] == _capi.METRIC_CODES[metric]


def test_hellinger_rejects_negative_input():
    x = np.abs(np.random.RandomState(0).standard_normal((50, 8))).astype(np.float32)
    x[3, 2] = -0.5
    idx = np.tile(np.arange(5, dtype=np.int32), (50, 1))
    with pytest.raises(ValueError, match="non-negative"):
        nndescent.NNDescent.from_graph(x, idx, np.zeros((50, 5), np.float32), metric="hellinger")


@pytest.mark.parametrize("metric", ["true_angular", "manhattan"])
def test_out_of_scope_metrics_still_raise(metric):
    x = np.random.RandomState(0).standard_normal((50, 8)).astype(np.float32)
    with pytest.raises(NotImplementedError):
        nndescent.NNDescent(x, metric=metric)
