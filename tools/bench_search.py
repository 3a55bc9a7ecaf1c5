"""prepare() and query() of a GPU-built index at scale (SURVEY.md section 8f rows 2 and 4 to the measurement bar):
build 1 M x 128 (euclidean, k = 15), time prepare() by stage, then batched queries: queries / s and recall@10 vs exact.
usage: python tools/bench_search.py [n] [n_queries] [--quantization uint8] [--proxy-beam-size 4 1] [--epsilons 0.0 0.1 0.2]
(no torch; prints one JSON line).  With --quantization uint8 the same index is then switched to quantization="uint8": the
result gains the prepare() and device quantize times and one query row per proxy beam size and epsilon."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pynndescent_amd import NNDescent  # noqa: E402
from pynndescent_amd.search_tree import make_hub_tree  # noqa: E402
from tools.qbench import sift_like_np  # noqa: E402


def exact(x, q, k):
    out = np.empty((q.shape[0], k), np.int64)
    xn = (x.astype(np.float64) ** 2).sum(1)
    for a in range(0, q.shape[0], 64):
        qq = q[a:a + 64].astype(np.float64)
        dd = (qq * qq).sum(1)[:, None] + xn[None, :] - 2.0 * qq @ x.T.astype(np.float64)
        out[a:a + 64] = np.argpartition(dd, k, axis=1)[:, :k]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", nargs="?", type=int, default=1_000_000)
    ap.add_argument("n_queries", nargs="?", type=int, default=20_000)
    ap.add_argument("--quantization", choices=("none", "uint8"), default="none")
    ap.add_argument("--proxy-beam-size", type=int, nargs="+", default=[4])
    ap.add_argument("--epsilons", type=float, nargs="+", default=[0.0, 0.1, 0.2])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--truth-rows", type=int, default=500, help="queries whose recall is checked against exact search")
    ap.add_argument("--repeats", type=int, default=1, help="timed query() calls per row (the median is reported)")
    ap.add_argument("--proxy-ceiling", type=int, default=0, metavar="ROWS",
                    help="uint8: for ROWS of the checked queries, the share of the true top k inside the EXHAUSTIVE proxy top "
                         "proxy_beam_size * k (what a perfect walk on the codes could rerank)")
    args = ap.parse_args()
    n, nq, k = args.n, args.n_queries, args.k
    allx = sift_like_np(n + nq, 128, seed=1)
    x, q = allx[:n], allx[n:]
    t0 = time.perf_counter()
    index = NNDescent(x, "euclidean", n_neighbors=15, n_trees=8, random_state=3)
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    tree = make_hub_tree(x, index._neighbor_graph[0], "euclidean", 30, 200)
    t_tree = time.perf_counter() - t0
    t0 = time.perf_counter()
    index.prepare()
    t_prepare = time.perf_counter() - t0
    index.query(q[:256], k=k, epsilon=0.1)  # warm
    res = {"n": n, "n_queries": nq, "k": k, "build_s_incl_h2d_d2h": round(t_build, 3), "hub_tree_alone_s": round(t_tree, 3),
           "hub_tree_nodes": int(tree.children.shape[0]), "prepare_total_s": round(t_prepare, 3), "queries": []}
    rows = np.arange(0, nq, max(1, nq // args.truth_rows))
    truth = exact(x, q[rows], k)

    def measure(quantization, beam):
        for eps in args.epsilons:
            dts = []
            for _ in range(max(1, args.repeats)):
                t0 = time.perf_counter()
                qi, qd = index.query(q, k=k, epsilon=eps, proxy_beam_size=beam)
                dts.append(time.perf_counter() - t0)
            dt = float(np.median(dts))
            rec = float(np.mean([len(np.intersect1d(t, a)) / float(k) for t, a in zip(truth, qi[rows])]))
            res["queries"].append({"quantization": quantization, "proxy_beam_size": beam if quantization != "none" else None,
                                   "epsilon": eps, "queries_per_s_host_to_host": round(nq / dt, 1), "call_ms_median": round(dt * 1e3, 3),
                                   "call_ms_min_max": [round(min(dts) * 1e3, 3), round(max(dts) * 1e3, 3)], "recall_at_10": round(rec, 4),
                                   "spilled_to_global_tier": index._searcher.last_spilled()})

    measure("none", 1)
    if args.quantization == "uint8":
        index.quantization = "uint8"  # the same graph and searcher: prepare() adds the codebook and the device codes
        t0 = time.perf_counter()
        index.prepare()
        res["uint8_prepare_s"] = round(time.perf_counter() - t0, 4)
        values = index._quantized_values
        times = []
        for _ in range(3):  # the device step alone (the codes stay on the device), then with the codes' copy to the host
            t0 = time.perf_counter()
            index._searcher.quantize_u8(values, fetch=False)
            times.append(time.perf_counter() - t0)
        res["uint8_quantize_device_s"] = round(min(times), 5)
        t0 = time.perf_counter()
        index._searcher.quantize_u8(values, fetch=True)
        res["uint8_quantize_with_d2h_s"] = round(time.perf_counter() - t0, 5)
        index.query(q[:256], k=k, epsilon=0.1, proxy_beam_size=args.proxy_beam_size[0])  # warm
        for beam in args.proxy_beam_size:
            measure("uint8", beam)
        if args.proxy_ceiling > 0:
            values = np.concatenate([values, np.full(256 - len(values), values[-1], np.float32)])
            xq = values[index._quantized_data[np.argsort(index._vertex_order)]]  # dequantized rows, original order
            sub = rows[: args.proxy_ceiling]
            for beam in args.proxy_beam_size:
                top = exact(xq, q[sub], beam * k)
                share = float(np.mean([len(np.intersect1d(t, a)) / float(k) for t, a in zip(truth[: len(sub)], top)]))
                res.setdefault("uint8_exhaustive_proxy_ceiling", []).append(
                    {"proxy_beam_size": beam, "queries": int(len(sub)), "true_top_k_in_proxy_top_search_k": round(share, 4)})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
