"""Generate tests/golden/quantized_uint8.npz -- the reference's quantization="uint8" search -- from the REFERENCE ITSELF.

Run in the build container only (needs the reference tree, loaded un-jitted through ``oracle/ref_t0.py`` exactly as
``make_golden_metrics.py`` does):

    python tests/golden/make_golden_quantized.py

Per metric (euclidean, cosine, dot): the data (tests/metric_util.py metric_data: 2000 x 16 clustered, 200 held-out
queries; dot with zero rows and one zero query), the reference's ``NNDescent(metric=..., n_neighbors=10, random_state=3,
quantization="uint8")`` after ``prepare()``: its ``_quantized_values``, ``_quantized_data`` (the search tree's order, as the
reference keeps it) and ``_vertex_order``, the answers of ``query(k=10)`` (corrected distances), and recall@10 against
float64 brute force of that index and of the same index built without quantization.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_t0  # noqa: E402
from tests import metric_util as MU  # noqa: E402
from tests import quantized_util as QU  # noqa: E402

METRICS = ("euclidean", "cosine", "dot")
SEED = 3
K = QU.K


def main():
    pynndescent = ref_t0.load_reference()
    out = {}
    for metric in METRICS:
        x, q = QU.fixture_data(metric)
        t = QU.truth(metric, x, q)
        out["x_%s" % metric], out["queries_%s" % metric] = x, q
        for quant in ("uint8", None):
            t0 = time.time()
            index = pynndescent.NNDescent(x, metric=metric, n_neighbors=K, random_state=SEED, quantization=quant)
            index.prepare()
            qi, qd = index.query(q, k=K)
            rec = MU.recall(t, np.asarray(qi))
            if quant is None:
                out["recall_plain_%s" % metric] = np.float64(rec)
            else:
                out["values_%s" % metric] = np.asarray(index._quantized_values, np.float32)
                out["codes_%s" % metric] = np.asarray(index._quantized_data, np.uint8)
                out["vertex_order_%s" % metric] = np.asarray(index._vertex_order, np.int64)
                out["q_idx_%s" % metric] = np.asarray(qi, np.int64)
                out["q_dist_%s" % metric] = np.asarray(qd, np.float64)
                out["recall_uint8_%s" % metric] = np.float64(rec)
            print("%s quantization=%s: recall@10 %.4f (%.1f s)" % (metric, quant, rec, time.time() - t0), flush=True)
    path = os.path.join(HERE, "quantized_uint8.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
