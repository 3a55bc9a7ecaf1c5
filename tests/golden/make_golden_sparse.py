"""Generate tests/golden/sparse_input.npz from the REFERENCE's own sparse path.

Run in the build container only (needs the reference tree, loaded un-jitted through ``oracle/ref_t0.py`` exactly as
``make_golden_metrics.py`` does):

    python tests/golden/make_golden_sparse.py [--only euclidean ...]

The data is ``tests/sparse_util.fixture_data()`` (2000 x 64 clustered rows at density about 0.15, no explicitly stored zero, and
200 held-out queries); it is generated again by the test and not stored.  Per metric (euclidean, cosine, hellinger, jaccard) and
seed: the graph of the reference's ``NNDescent(csr, metric=..., n_neighbors=10)`` and its recall@10, and for the first seed the
answers of ``query(csr_queries, k=10)`` with their recall.  Recall is counted by distance
(``sparse_util.recall_by_distance``).  The reference's own mean recall must be at least 0.9 for every metric, or the script
stops: a margin of 0.01 against a poor graph would say little.

``--only`` regenerates the named metrics and keeps the others' entries of an existing file.
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_t0  # noqa: E402
from tests import sparse_util as SU  # noqa: E402

SEEDS = (3, 17, 42)
METRICS = ("euclidean", "cosine", "hellinger", "jaccard")
K = 10


def make(metric, out):
    pynndescent = ref_t0.load_reference()
    x, q = SU.fixture_data()
    csr, csr_q = sp.csr_matrix(x), sp.csr_matrix(q)
    assert (csr.data != 0).all() and (csr_q.data != 0).all()
    kth = SU.kth_distance(metric, x, x, K)
    recalls = []
    for s in SEEDS:
        t0 = time.time()
        index = pynndescent.NNDescent(csr, metric=metric, n_neighbors=K, random_state=s)
        idx = np.asarray(index._neighbor_graph[0], np.int32)
        out["%s_idx_%d" % (metric, s)] = idx
        recalls.append(SU.recall_by_distance(metric, x, x, idx, kth))
        out["%s_recall_%d" % (metric, s)] = np.float64(recalls[-1])
        print("%s seed %d: recall %.4f (%.1f s)" % (metric, s, recalls[-1], time.time() - t0), flush=True)
        if s == SEEDS[0]:
            t0 = time.time()
            index.prepare()
            qi, qd = index.query(csr_q, k=K)
            qi = np.asarray(qi, np.int32)
            out[metric + "_q_idx"], out[metric + "_q_dist"] = qi, np.asarray(qd)
            out[metric + "_q_recall"] = np.float64(SU.recall_by_distance(metric, q, x, qi, SU.kth_distance(metric, q, x, K)))
            print("%s query: recall %.4f (%.1f s)" % (metric, out[metric + "_q_recall"], time.time() - t0), flush=True)
    if np.mean(recalls) < 0.9:
        raise SystemExit("%s: the reference's own mean recall is %.4f < 0.9 -- choose other data" % (metric, np.mean(recalls)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=list(METRICS))
    args = ap.parse_args()
    path = os.path.join(HERE, "sparse_input.npz")
    out = dict(np.load(path)) if os.path.exists(path) else {}
    out["seeds"] = np.array(SEEDS, np.int64)
    for m in args.only:
        make(m, out)
        np.savez_compressed(path, **out)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))
