"""Generate tests/golden/proxy_inner_product.npz -- the reference's metric="proxy_inner_product" -- from the REFERENCE ITSELF.

Run in the build container only (needs the reference tree, loaded un-jitted through ``oracle/ref_t0.py`` exactly as
``make_golden_quantized.py`` does; about half a minute per seed):

    python tests/golden/make_golden_proxy.py

The data is tests/metric_util.py metric_data("inner_product"): 2000 x 16 clustered rows, 200 held-out queries.  Per seed (3 .. 7),
the reference's ``NNDescent(metric="proxy_inner_product", n_neighbors=10, random_state=seed)`` after ``prepare()``: its
``neighbor_graph`` (proxy distances, uncorrected, in the original numbering), ``_vertex_order`` and ``_min_distance``, the answers
of ``query(k=10)`` at ``proxy_beam_size`` 4 and 1 (negative inner products), the recall@10 of each against the float64 maximum
inner products, and the recall@10 of the graph against float64 proxy-distance brute force.
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_t0  # noqa: E402
from tests import proxy_util as PU  # noqa: E402


def main():
    pynndescent = ref_t0.load_reference()
    x, q = PU.fixture_data()
    mips = PU.mips_truth(x, q)
    proxy_nn = PU.proxy_truth(x)
    out = {"x": x, "queries": q, "seeds": np.asarray(PU.SEEDS, np.int64)}
    for seed in PU.SEEDS:
        t0 = time.time()
        index = pynndescent.NNDescent(x, metric=PU.METRIC, n_neighbors=PU.K, random_state=seed)
        assert index._is_proxy_distance and index._distance_correction is None and not index._angular_trees
        gi, gd = index.neighbor_graph
        out["graph_idx_%d" % seed] = np.asarray(gi, np.int32)
        out["graph_dist_%d" % seed] = np.asarray(gd, np.float32)
        out["graph_recall_%d" % seed] = np.float64(PU.recall(proxy_nn, np.asarray(gi)))
        index.prepare()
        out["vertex_order_%d" % seed] = np.asarray(index._vertex_order, np.int64)
        out["min_distance_%d" % seed] = np.float32(index._min_distance)
        line = "seed %d: graph recall@10 (proxy brute force) %.4f" % (seed, out["graph_recall_%d" % seed])
        for beam in (4, 1):
            qi, qd = index.query(q, k=PU.K, proxy_beam_size=beam)
            out["q_idx_b%d_%d" % (beam, seed)] = np.asarray(qi, np.int64)
            out["q_dist_b%d_%d" % (beam, seed)] = np.asarray(qd, np.float64)
            out["q_recall_b%d_%d" % (beam, seed)] = np.float64(PU.recall(mips, np.asarray(qi)))
            line += ", query beam %d recall@10 (true MIPS) %.4f" % (beam, out["q_recall_b%d_%d" % (beam, seed)])
        print("%s, min_distance %.4f (%.1f s)" % (line, float(index._min_distance), time.time() - t0), flush=True)
    np.savez_compressed(PU.GOLDEN, **out)
    print("wrote %s (%.1f KB)" % (PU.GOLDEN, os.path.getsize(PU.GOLDEN) / 1024.0))


if __name__ == "__main__":
    main()
