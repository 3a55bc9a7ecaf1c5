"""quantization="uint8": the host side -- the codebook against the reference's own (tests/golden/quantized_uint8.npz,
tests/golden/make_golden_quantized.py) and the errors prepare() / query() raise before any device work.  No GPU needed."""
import os

import numpy as np
import pytest
from sklearn.preprocessing import normalize

from pynndescent_amd import NNDescent

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantized_uint8.npz")
METRICS = ("euclidean", "cosine", "dot")


def _golden():
    return np.load(GOLDEN)


def _index(metric="euclidean", quantization="uint8", n=300, d=8):
    """An un-prepared index around a small random graph (no device work until prepare())."""
    rs = np.random.RandomState(0)
    x = rs.standard_normal((n, d)).astype(np.float32)
    idx = np.stack([(np.arange(n) + j) % n for j in range(10)], 1).astype(np.int32)
    dist = np.sort(rs.uniform(0.0, 1.0, idx.shape), axis=1).astype(np.float32)
    dist[:, 0] = 0.0
    return NNDescent.from_graph(x, idx, dist, metric=metric, random_state=3, quantization=quantization)


@pytest.mark.parametrize("metric", METRICS)
def test_codebook_matches_reference(metric):
    """The host codebook helper reproduces the reference's _quantized_values bit for bit (rows in their original order;
    NNDescent normalises dot data first, as the reference does)."""
    from pynndescent_amd.nndescent import uint8_codebook

    g = _golden()
    x = g["x_%s" % metric]
    if metric == "dot":
        x = normalize(x, norm="l2")
    values = uint8_codebook(np.ascontiguousarray(x, np.float32), 3)
    ref = g["values_%s" % metric]
    assert values.dtype == np.float32 and values.shape == ref.shape == (256,)
    assert values.tobytes() == ref.tobytes()


def test_codebook_of_few_distinct_values_is_unique():
    """At most 256 distinct sampled values: the codebook is np.unique of the sample (pynndescent_.py:2201-2202)."""
    from pynndescent_amd.nndescent import uint8_codebook

    rs = np.random.RandomState(1)
    x = rs.randint(0, 40, (500, 6)).astype(np.float32) * np.float32(0.25)
    values = uint8_codebook(x, 7)
    np.testing.assert_array_equal(values, np.unique(x).astype(np.float32))
    assert values.dtype == np.float32


def test_codes_are_searchsorted_of_the_codebook_in_the_fixture():
    """The fixture's codes are np.searchsorted(values, rows) cast to uint8, rows in the search tree's order -- the rule
    the device kernel reproduces (tests/test_gpu_quantized.py checks the kernel against it)."""
    g = _golden()
    for metric in METRICS:
        x = g["x_%s" % metric]
        if metric == "dot":
            x = normalize(x, norm="l2")
        order = g["vertex_order_%s" % metric]
        codes = np.searchsorted(g["values_%s" % metric], x[order]).astype(np.uint8)
        np.testing.assert_array_equal(codes, g["codes_%s" % metric])


def test_uint8_of_an_unsupported_metric_raises_value_error():
    index = _index("correlation")
    with pytest.raises(ValueError, match="Not uint8 quantization version of correlation"):
        index.prepare()


def test_unknown_quantization_raises_value_error():
    index = _index("euclidean", "int7")
    with pytest.raises(ValueError, match="Unrecognized quantization type int7"):
        index.prepare()
    with pytest.raises(ValueError, match="Unrecognized quantization type int7"):
        index.query(np.zeros((2, 8), np.float32), k=5)


@pytest.mark.parametrize("quantization", ["uint4", "binary"])
def test_uint4_and_binary_stay_out_of_scope(quantization):
    index = _index("euclidean", quantization)
    with pytest.raises(NotImplementedError, match="to_reference"):
        index.prepare()


def test_search_k_above_256_is_rejected_before_prepare():
    """proxy_beam_size * k > 256 is the result bound of k_query; query() checks it before it prepares anything."""
    index = _index("euclidean")
    with pytest.raises(NotImplementedError, match="260"):
        index.query(np.zeros((2, 8), np.float32), k=65, proxy_beam_size=4)
    assert not hasattr(index, "_search_graph")
    with pytest.raises(ValueError, match="proxy_beam_size"):
        index.query(np.zeros((2, 8), np.float32), k=10, proxy_beam_size=0)
