"""Generate tests/golden/metric_<name>.npz for dot / inner_product / correlation / hellinger from the REFERENCE ITSELF.

Run in the build container only (needs the reference tree, loaded un-jitted through ``oracle/ref_t0.py`` exactly as
``make_golden.py`` does):

    python tests/golden/make_golden_metrics.py [--only dot ...]
    python tests/golden/make_golden_metrics.py --search-graph


Per metric: the data (tests/metric_util.py metric_data: 2000 x 16 clustered, with zero / constant rows), three builds
of the reference's ``NNDescent(metric=..., n_neighbors=10)`` -- its ``_neighbor_graph`` and corrected ``neighbor_graph``,
recall@10 against float64 brute force, the share of rows whose first neighbour is the row itself -- and the answers of
``query(k=10)`` for 200 held-out queries after ``prepare()`` on the first build.

``--search-graph`` writes metric_search_graph.npz instead and leaves the other fixtures alone: per metric, the reference's
search graph after ``prepare()`` on the seed-3 build, its edges mapped back to original ids through ``_vertex_order``
(``<metric>_rows`` / ``<metric>_cols``, sorted by (row, col)).

``corrected`` is the reference's own correction applied to the float64 view of the distances: the jitted reference's
``numba.vectorize`` corrections return float64; the un-jitted stub would keep float32 under NumPy 2.
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
from tests import metric_util as MU  # noqa: E402

SEEDS = (3, 17, 42)
K = 10


def make(metric):
    pynndescent = ref_t0.load_reference()
    from pynndescent import distances as D

    x, q = MU.metric_data(metric)
    if metric == "dot":
        q[[5]] = 0.0  # a zero query: the reference skips it (pynndescent_.py:1806-1811)
    truth = MU.brute_knn(metric, x if metric != "dot" else _normalised(x), k=K)
    out = dict(x=x, queries=q, seeds=np.array(SEEDS, np.int64))
    corr = {"dot": D.correct_alternative_cosine, "inner_product": D.correct_alternative_inner_product,
            "hellinger": D.correct_alternative_hellinger}.get(metric)
    for s in SEEDS:
        t0 = time.time()
        index = pynndescent.NNDescent(x, metric=metric, n_neighbors=K, random_state=s)
        idx, dist = index._neighbor_graph
        out["idx_%d" % s] = idx.astype(np.int32)
        out["dist_%d" % s] = dist.astype(np.float32)
        out["corrected_%d" % s] = (corr(dist.astype(np.float64)) if corr else dist.astype(np.float32))
        out["recall_%d" % s] = np.float64(MU.recall(truth, idx))
        out["self_first_%d" % s] = np.float64(MU.self_first_share(idx))
        print("%s seed %d: recall %.4f self-first %.3f (%.1f s)" % (metric, s, out["recall_%d" % s], out["self_first_%d" % s],
                                                                    time.time() - t0))
        if s == SEEDS[0]:
            t0 = time.time()
            index.prepare()
            qi, qd = index.query(q, k=K)
            out["q_idx"] = np.asarray(qi, np.int32)
            out["q_dist"] = np.asarray(qd)
            print("%s query: %.1f s" % (metric, time.time() - t0))
    path = os.path.join(HERE, "metric_%s.npz" % metric)
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


def make_search_graph(metrics):
    pynndescent = ref_t0.load_reference()
    out = {}
    for metric in metrics:
        t0 = time.time()
        x, _ = MU.metric_data(metric)
        index = pynndescent.NNDescent(x, metric=metric, n_neighbors=K, random_state=SEEDS[0])
        index.prepare()
        g = index._search_graph.tocoo()
        order = np.asarray(index._vertex_order)
        rows, cols = order[g.row].astype(np.int32), order[g.col].astype(np.int32)
        keep = np.lexsort((cols, rows))
        out[metric + "_rows"], out[metric + "_cols"] = rows[keep], cols[keep]
        print("%s search graph: %d edges (%.1f s)" % (metric, rows.size, time.time() - t0))
    path = os.path.join(HERE, "metric_search_graph.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))


def _normalised(x):
    from sklearn.preprocessing import normalize

    return normalize(x, norm="l2")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=list(MU.NEW_METRICS))
    ap.add_argument("--search-graph", action="store_true")
    args = ap.parse_args()
    if args.search_graph:
        make_search_graph(args.only)
    else:
        for m in args.only:
            make(m)
