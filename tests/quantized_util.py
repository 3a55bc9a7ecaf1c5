"""Inputs and float64 ground truth of the quantization="uint8" fixture (tests/golden/make_golden_quantized.py).  Test
helpers only."""
import numpy as np

from tests import metric_util as MU

K = 10


def fixture_data(metric):
    """The fixture's rows and held-out queries (NNDescent normalises the dot rows itself, as the reference does)."""
    x, q = MU.metric_data(metric)
    if metric == "dot":
        q[[5]] = 0.0  # a zero query: the reference skips it (pynndescent_.py:1806-1811)
    return x, q


def truth(metric, x, q, k=K):
    """Exact k nearest rows of x for every query by the metric (ties by id); dot ranks by the normalised rows."""
    a, b = q.astype(np.float64), x.astype(np.float64)
    if metric == "euclidean":
        dm = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * a @ b.T
    else:
        bn = b / np.maximum(np.linalg.norm(b, axis=1, keepdims=True), 1e-300)
        an = a / np.maximum(np.linalg.norm(a, axis=1, keepdims=True), 1e-300) if metric == "cosine" else a
        dm = -(an @ bn.T)
    return np.argsort(dm, axis=1, kind="stable")[:, :k]


def exact_corrected(metric, x, q, idx):
    """float64 true distances from each query to the rows idx (n_queries, k) refer to, by the rule of the reference's
    rerank: the RAW query against the index's rows (dot: 1 - q.x with x normalised and q as given)."""
    a = q.astype(np.float64)[:, None, :]
    b = x.astype(np.float64)[np.clip(idx, 0, None)]
    if metric == "euclidean":
        return np.sqrt(((a - b) ** 2).sum(-1))
    g = (a * b).sum(-1)
    if metric == "dot":
        return 1.0 - g
    return 1.0 - g / np.sqrt((a * a).sum(-1) * (b * b).sum(-1))
