"""Generate tests/golden/metric_linear.npz for mahalanobis / seuclidean / wminkowski (p = 2) from the REFERENCE ITSELF.

Run in the build container only (needs the reference tree, loaded un-jitted through ``oracle/ref_t0.py`` exactly as
``make_golden_metrics.py`` does):

    python tests/golden/make_golden_linear.py [--only mahalanobis ...]

The data: tests/metric_util.py ``metric_data("euclidean")`` (2000 x 16 clustered, 200 held-out queries) and the parameters of
tests/linear_util.py ``fixture_kwds`` (a fixed SPD VI, V = the column variances, a fixed w with one zero entry).  Per metric:
three builds of the reference's ``NNDescent(metric=..., metric_kwds=..., n_neighbors=10)`` -- its ``neighbor_graph``, recall@10
against float64 brute force -- and the answers of ``query(k=10)`` after ``prepare()`` on the first build with their recall.
With ``--only`` the other metrics' entries of an existing file are kept.
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_t0  # noqa: E402
from tests import linear_util as LU  # noqa: E402
from tests import metric_util as MU  # noqa: E402

SEEDS = (3, 17, 42)
K = 10
PATH = os.path.join(HERE, "metric_linear.npz")


def make(metric, out):
    pynndescent = ref_t0.load_reference()
    x, q = LU.fixture_data()
    kwds = LU.fixture_kwds(x)[metric]
    truth = LU.brute_knn(metric, kwds, x, k=K)
    q_truth = LU.brute_knn(metric, kwds, x, q, k=K)
    for s in SEEDS:
        t0 = time.time()
        index = pynndescent.NNDescent(x, metric=metric, metric_kwds=kwds, n_neighbors=K, random_state=s)
        idx, dist = index.neighbor_graph
        out["%s_idx_%d" % (metric, s)] = np.asarray(idx, np.int32)
        out["%s_dist_%d" % (metric, s)] = np.asarray(dist, np.float32)
        out["%s_recall_%d" % (metric, s)] = np.float64(MU.recall(truth, idx))
        print("%s seed %d: recall %.4f (%.1f s)" % (metric, s, out["%s_recall_%d" % (metric, s)], time.time() - t0), flush=True)
        if s == SEEDS[0]:
            t0 = time.time()
            index.prepare()
            qi, qd = index.query(q, k=K)
            out[metric + "_q_idx"] = np.asarray(qi, np.int32)
            out[metric + "_q_dist"] = np.asarray(qd, np.float32)
            out[metric + "_q_recall"] = np.float64(MU.recall(q_truth, qi))
            print("%s query: recall %.4f (%.1f s)" % (metric, out[metric + "_q_recall"], time.time() - t0), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=list(LU.METRICS))
    ap.add_argument("--out", default=PATH)
    args = ap.parse_args()
    PATH = args.out
    out = dict(np.load(PATH)) if os.path.exists(PATH) else {}
    out["seeds"] = np.array(SEEDS, np.int64)
    for m in args.only:
        make(m, out)
    np.savez_compressed(PATH, **out)
    print("wrote %s (%.1f KB)" % (PATH, os.path.getsize(PATH) / 1024.0))
