"""Generate tests/golden/boolean_metrics.npz -- the nine boolean metrics -- from the REFERENCE ITSELF.

Run in the build container only (needs the reference tree, loaded un-jitted through ``oracle/ref_t0.py`` exactly as
``make_golden_metrics.py`` does; one worker process per metric):

    python tests/golden/make_golden_boolean.py [--only jaccard ...] [--jobs 9]

The data is tests/boolean_util.py fixture_data(): 2000 x 48 clustered binary rows (density 0.1 .. 0.4, two all-zero rows, one
all-ones row, five exact duplicates) and 200 held-out queries, one of them all-zero; stored as uint8 indicators.  Per metric and
seed (3, 17, 42), the reference's ``NNDescent(metric=..., n_neighbors=10, random_state=seed)``: its ``_neighbor_graph`` (ids as
int16, distances as float32; +inf where alternative_jaccard has it), the corrected graph where the metric has a correction
(jaccard: float64, the reference's own ufunc on the float64 view; for the other eight the corrected graph IS ``dist``) and the
distance-recall@10 against float64 brute force; after ``prepare()`` on the first seed, the answers of ``query(k=10)`` and their
distance-recall.  The reference alone must reach a distance-recall@10 of 0.9 on every metric; the script refuses to write the
file otherwise."""
import argparse
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_t0  # noqa: E402
from tests import boolean_util as BU  # noqa: E402


def make(metric):
    pynndescent = ref_t0.load_reference()
    from pynndescent import distances as D

    x, q = BU.fixture_data()
    out = {}
    lines = []
    for s in BU.SEEDS:
        t0 = time.time()
        index = pynndescent.NNDescent(x, metric=metric, n_neighbors=BU.K, random_state=s)
        assert index._angular_trees == (metric in ("jaccard", "dice"))
        idx, dist = index._neighbor_graph
        out["%s_idx_%d" % (metric, s)] = np.asarray(idx).astype(np.int16)
        out["%s_dist_%d" % (metric, s)] = np.asarray(dist).astype(np.float32)
        if metric == "jaccard":
            out["%s_corrected_%d" % (metric, s)] = D.correct_alternative_jaccard(np.asarray(dist).astype(np.float64))
        r = BU.distance_recall(metric, x, np.asarray(idx))
        out["%s_recall_%d" % (metric, s)] = np.float64(r)
        lines.append("%s seed %d: distance-recall@10 %.4f (%.1f s)" % (metric, s, r, time.time() - t0))
        print(lines[-1], flush=True)
        if s == BU.SEEDS[0]:
            t0 = time.time()
            index.prepare()
            qi, qd = index.query(q, k=BU.K)
            out["%s_q_idx" % metric] = np.asarray(qi).astype(np.int16)
            out["%s_q_dist" % metric] = np.asarray(qd, np.float64)
            rq = BU.distance_recall(metric, x, np.asarray(qi), q=q)
            out["%s_q_recall" % metric] = np.float64(rq)
            lines.append("%s query: distance-recall@10 %.4f (%.1f s)" % (metric, rq, time.time() - t0))
            print(lines[-1], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=list(BU.METRICS))
    ap.add_argument("--jobs", type=int, default=9)
    args = ap.parse_args()
    x, q = BU.fixture_data()
    out = {"x": x.astype(np.uint8), "queries": q.astype(np.uint8), "seeds": np.asarray(BU.SEEDS, np.int64)}
    if os.path.exists(BU.GOLDEN) and set(args.only) != set(BU.METRICS):
        with np.load(BU.GOLDEN) as old:
            out.update({key: old[key] for key in old.files if key.split("_")[0] not in args.only})
    with multiprocessing.get_context("spawn").Pool(min(args.jobs, len(args.only))) as pool:
        for part in pool.map(make, args.only):
            out.update(part)
    low = [(m, s, float(out["%s_recall_%d" % (m, s)])) for m in args.only for s in BU.SEEDS if out["%s_recall_%d" % (m, s)] < 0.9]
    if low:
        raise SystemExit("the reference is below distance-recall 0.9: %r -- change the data, not the bar" % (low,))
    np.savez_compressed(BU.GOLDEN, **out)
    print("wrote %s (%.1f KB)" % (BU.GOLDEN, os.path.getsize(BU.GOLDEN) / 1024.0))


if __name__ == "__main__":
    main()
