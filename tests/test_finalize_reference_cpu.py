"""The host model of finalize (tests/finalize_reference.py) against a plain float64 evaluation, and proof that the bit
comparison of tests/test_gpu_finalize_exact.py notices a wrong order of operations."""
from fractions import Fraction

import numpy as np
import pytest

from tests import finalize_reference as FR


def _ulp32_apart(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)  # (non-negative finite values: the bit patterns are ordered as the values)


def test_fma_rounds_once():
    rs = np.random.RandomState(0)
    for _ in range(2000):
        a, b, c = (float(v) for v in rs.standard_normal(3) * 2.0 ** rs.randint(-30, 30, 3))
        if rs.rand() < 0.3:
            c = -a * b  # cancellation: what is left is the product's rounding error
        want = float(Fraction(a) * Fraction(b) + Fraction(c))  # Fraction -> float rounds to nearest even
        assert FR.fma(a, b, c) == want
    assert FR.fma(0.0, 5.0, 0.0) == 0.0 and FR.fma(3.0, 0.0, 7.0) == 7.0 and FR.fma(2.0, 3.0, 0.0) == 6.0
    # one rounding, not two: 1 + 2^-53 + 2^-106 lies above the tie that a rounded product would leave
    assert FR.fma(1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, -1.0) == 2.0 ** -51 + 2.0 ** -104


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("d", [4, 20, 64, 132])
def test_model_matches_plain_float64(metric, d):
    """within 2 ulp of float32: the model's sums differ from numpy's by float64 roundings only"""
    rs = np.random.RandomState(d + metric)
    n, k = 12, 5
    x = (rs.standard_normal((n, d)) + 0.5).astype(np.float32)
    x[3] = x[7]  # duplicate points
    g = np.stack([rs.permutation(n)[:k] for _ in range(n)]).astype(np.int32)
    g[2, 1:] = -1
    g[5] = -1
    idx, dist = FR.finalize_rows(x, g, metric)
    x64 = x.astype(np.float64)
    for i in range(n):
        m = idx[i] >= 0
        assert sorted(idx[i][m].tolist()) == sorted(g[i][g[i] >= 0].tolist())
        assert np.all(idx[i][~m] == -1) and np.all(np.isinf(dist[i][~m])) and (not m.any() or m[:m.sum()].all())
        nb = x64[idx[i][m]]
        if metric == 0:
            want = ((x64[i] - nb) ** 2).sum(1)
        else:
            dot, na, nbn = nb @ x64[i], x64[i] @ x64[i], (nb * nb).sum(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                want = np.where(dot > 0, np.maximum(np.log2(np.sqrt(na * nbn) / dot), 0.0), FR.FLT_MAX)
        assert _ulp32_apart(dist[i][m], want.astype(np.float32)).max(initial=0) <= 2
        keys = [(int(b), int(j)) for b, j in zip(dist[i][m].view(np.uint32), idx[i][m])]
        assert keys == sorted(keys)
    # the duplicate points are at the same distance from everyone: ties go by index
    assert FR.Model(x, metric).value(0, 3).tobytes() == FR.Model(x, metric).value(0, 7).tobytes()


def test_cosine_conventions():
    x = np.zeros((4, 8), np.float32)
    x[1, :4] = [1, 2, 3, 4]
    x[2, :4] = [-1, -2, -3, -4]
    x[3, :4] = [2, 4, 6, 8]
    m = FR.Model(x, 1)
    assert m.value(0, 0) == 0.0 and m.value(0, 1) == np.float32(FR.FLT_MAX) and m.value(1, 2) == np.float32(FR.FLT_MAX)
    assert m.value(1, 3) == 0.0 and m.value(1, 1) == 0.0


def test_planted_fma_order_is_caught():
    x = FR.sensitive_fma_rows()
    g = np.array([[1], [0]], np.int32)
    good = FR.finalize_rows(x, g, 0)[1]
    bad = FR.finalize_rows(x, g, 0, fma_order=(2, 0, 3))  # p0 and p2 swapped
    assert good[0, 0] == np.float32(1.0 + 2.0 ** -23) and bad[1][0, 0] == np.float32(1.0)
    assert good.tobytes() != bad[1].tobytes()


def test_planted_butterfly_is_caught():
    x = FR.sensitive_butterfly_rows()
    g = np.array([[1], [0]], np.int32)
    good = FR.finalize_rows(x, g, 0)[1]
    bad = FR.finalize_rows(x, g, 0, butterfly=(1, 2, 4, 8))[1]
    assert good[0, 0] == np.float32(1.0 + 2.0 ** -23) and bad[0, 0] == np.float32(1.0)
    assert good.tobytes() != bad.tobytes()
