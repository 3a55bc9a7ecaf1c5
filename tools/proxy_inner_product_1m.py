"""Build and query measurements of metric="proxy_inner_product" next to "inner_product" and "cosine" (profiles/proxy_inner_product_1m.txt).

The method of profiles/metrics_build_times_1m.txt: tests/util_data.clustered(n + n_queries, 128, 16, 64, seed=1, nonneg=True), the
first n rows built with NNDescent(x, metric, n_neighbors=15, n_trees=8, random_state=1), best of two builds per metric,
device_ms = the sum of the _build_stats stage times, iters = iterations to the stop rule.  Then, for the inner-product metrics,
prepare() and query(q, k=10, epsilon=0.1) of the held-out rows: queries / s (the median of --repeats calls) and recall@10 against
the true maximum inner products (float64, --truth-rows of the queries; proxy_inner_product at every --proxy-beam-size).

usage: python tools/proxy_inner_product_1m.py [n] [n_queries] [--metrics ...]     (one JSON line per metric)
Set PYNND_AMD_LIB to another build of the library to measure that build's kernels with the same script."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pynndescent_amd import NNDescent, nndescent  # noqa: E402
from tests.util_data import clustered  # noqa: E402

STAGES = ("ms_prep", "ms_forest", "ms_leaf_init", "ms_random_init", "ms_descent", "ms_finalize")


def mips_truth(x, q, k):
    out = np.empty((q.shape[0], k), np.int64)
    x64 = x.astype(np.float64)
    for a in range(0, q.shape[0], 32):
        g = q[a:a + 32].astype(np.float64) @ x64.T
        part = np.argpartition(-g, k, axis=1)[:, :k]
        out[a:a + 32] = np.take_along_axis(part, np.argsort(-np.take_along_axis(g, part, 1), axis=1, kind="stable"), 1)
    return out


def recall(truth, idx):
    return float(np.mean([len(set(t.tolist()) & set(r.tolist())) / len(t) for t, r in zip(truth, idx)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("n_queries", nargs="?", type=int, default=10_000)
    ap.add_argument("--metrics", nargs="+", default=["cosine", "inner_product", "proxy_inner_product"])
    ap.add_argument("--proxy-beam-size", type=int, nargs="+", default=[4, 1])
    ap.add_argument("--truth-rows", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--epsilon", type=float, default=0.1)
    args = ap.parse_args()
    pts = clustered(args.n + args.n_queries, 128, 16, 64, seed=1, nonneg=True)
    x, q = np.ascontiguousarray(pts[:args.n]), np.ascontiguousarray(pts[args.n:])
    rows = np.arange(0, args.n_queries, max(1, args.n_queries // args.truth_rows))
    truth = None
    for metric in args.metrics:
        if metric not in nndescent._METRICS:
            print(json.dumps({"metric": metric, "skipped": "this build of the package does not know the metric"}), flush=True)
            continue
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            index = NNDescent(x, metric=metric, n_neighbors=15, n_trees=8, random_state=1)
            wall = (time.perf_counter() - t0) * 1e3
            st = index._build_stats
            row = {"metric": metric, "device_ms": round(sum(st[s] for s in STAGES), 2), "wall_ms": round(wall, 1), "iters": st["n_iters_run"]}
            row.update({s: round(st[s], 2) for s in STAGES})
            if best is None or row["device_ms"] < best[0]["device_ms"]:
                best = (row, index)
        row, index = best
        if "inner_product" in metric:
            if truth is None:
                truth = mips_truth(x, q[rows], args.k)
            t0 = time.perf_counter()
            index.prepare()
            row["prepare_s"] = round(time.perf_counter() - t0, 3)
            row["queries"] = []
            for beam in (args.proxy_beam_size if getattr(nndescent._METRICS[metric], "proxy", False) else [None]):
                kw = {} if beam is None else {"proxy_beam_size": beam}
                index.query(q[:256], k=args.k, epsilon=args.epsilon, **kw)  # warm
                times = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    qi, _ = index.query(q, k=args.k, epsilon=args.epsilon, **kw)
                    times.append(time.perf_counter() - t0)
                row["queries"].append({"proxy_beam_size": beam, "queries_per_s": round(args.n_queries / float(np.median(times)), 1),
                                       "recall_at_%d_true_mips" % args.k: round(recall(truth, qi[rows]), 4),
                                       "spilled": index._searcher.last_spilled()})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
