"""What t-SNE's perplexity affinities of a device-resident index cost at 1 M x 128 float32 (euclidean, k = 90 = 3 * perplexity, the
benchmark's stand-in data): one process, ONE built index, the legs alternating, one warm-up of each, then REPS timed repetitions.

  gpu    index.perplexity_affinities(30)               csrc/affinity.hip and the sum merge of csrc/csr_graph.hip, tensors on the device
  gpu3   index.perplexity_affinities([10, 30, 60])     the multiscale form: three searches in one pass over the rows
  host   neighbor_graph brought down, the binary search of tests/affinity_util.py restated in numpy over all unfinished rows at
         once (float32), then scipy's P + P.T over the total: the route the call replaces

The clock is the host's, from a device synchronise to a device synchronise; the gpu legs also report their stream time (two events
around the call).  Last, the bytes k_perplexity_search has to move once (ids and distances read; ids, entries and betas written)
and the stream time of a memset of that many bytes.  The kernel's own time is not visible from here: run the gpu legs alone
under a kernel trace (``--gpu-only``) and read the k_perplexity_search lines of its statistics.  Run from the repository root:

    python tools/ab/perplexity_affinities_timing.py [--n N] [--d D] [--k K] [--reps R] [--gpu-only]
"""
import argparse
import os
import statistics
import sys
import time


def host_route(np, sp, ids, dists, perplexity):
    """The search for every row that has not stopped yet, then P + P.T over twice the total."""
    n, k = ids.shape
    counts = (ids >= 0) & (ids != np.arange(n)[:, None])
    e = np.where(counts, dists * dists, np.float32(np.inf)).astype(np.float32)
    with np.errstate(invalid="ignore"):  # (a row without a counting place: inf - inf, and its exp(nan) never counts)
        e -= e.min(axis=1, keepdims=True)
    w = np.where(counts, e, np.float32(0))  # the factor in sum e p: 0 where the place does not count (its p is exp(-inf) = 0)
    target = np.float32(np.log(perplexity))
    beta, lo, hi = np.ones(n, np.float32), np.full(n, -np.inf, np.float32), np.full(n, np.inf, np.float32)
    live, cond = np.arange(n), np.empty((n, k), np.float32)
    for step in range(100):
        b = beta[live]
        p = np.exp(-b[:, None] * e[live])
        s = np.maximum(p.sum(axis=1, dtype=np.float32), np.float32(1e-8))
        h = np.log(s) + b * (w[live] * p).sum(axis=1, dtype=np.float32) / s
        stop = (np.abs(h - target) <= np.float32(1e-5)) | (step == 99)
        cond[live[stop]] = p[stop] / s[stop, None]
        live, b, over = live[~stop], b[~stop], (h > target)[~stop]
        if not live.size:
            break
        lo[live], hi[live] = np.where(over, b, lo[live]), np.where(over, hi[live], b)
        other = np.where(over, hi[live], lo[live])
        beta[live] = np.where(np.isfinite(other), (b + other) / 2, np.where(over, b * 2, b / 2)).astype(np.float32)
    keep = counts & (cond != 0)
    a = sp.coo_array((cond[keep], (np.nonzero(keep)[0].astype(np.int32), ids[keep])), shape=(n, n)).tocsr()
    return (a + a.T.tocsr()) / np.float32(2.0 * cond[keep].sum(dtype=np.float64)), beta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, default=90)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpu-only", action="store_true", help="the gpu legs alone (for a kernel trace)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import numpy as np
    import scipy.sparse as sp
    import torch

    import bench
    from pynndescent_amd import NNDescent

    n, d, k, perplexity = args.n, args.d, args.k, args.k / 3.0
    x = bench.sift_like(n, d, seed=1, device=torch.device("cuda:0"), sample_seed=100)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = NNDescent(x, n_neighbors=k, n_trees=8, random_state=1234)
    torch.cuda.synchronize()
    print("index of %d x %d, n_neighbors %d built in %.1f s" % (n, d, k, time.perf_counter() - t0), flush=True)

    def host():
        ids, dists = index.neighbor_graph
        return host_route(np, sp, ids.cpu().numpy(), dists.cpu().numpy().astype(np.float32), perplexity)

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(e0.elapsed_time(e1)), out

    legs = {"gpu": lambda: index.perplexity_affinities(perplexity),
            "gpu3": lambda: index.perplexity_affinities([perplexity / 3.0, perplexity, 2.0 * perplexity])}
    if not args.gpu_only:
        legs["host"] = host
    results, kept = {}, {}
    for name, fn in legs.items():
        timed(fn)  # warm-up
    for _ in range(args.reps):  # alternating, so that drift of the machine lands on every leg alike
        for name, fn in legs.items():
            wall, stream, out = timed(fn)
            results.setdefault(name, []).append((wall, stream))
            kept[name] = out
    for name in legs:
        wall = [r[0] for r in results[name]]
        nnz = int(kept[name][0].nnz) if name == "host" else int(kept[name][0].values().shape[0])
        print("%-5s wall   min %9.2f  median %9.2f  max %9.2f ms  (%d reps, nnz %d)"
              % (name, min(wall), statistics.median(wall), max(wall), len(wall), nnz), flush=True)
        if name != "host":
            stream = [r[1] for r in results[name]]
            print("%-5s stream min %9.2f  median %9.2f  max %9.2f ms" % (name, min(stream), statistics.median(stream), max(stream)), flush=True)
    if not args.gpu_only:
        (g, betas), (h, betas_h) = kept["gpu"], kept["host"]
        print("largest relative difference of the betas %.3g; nnz gpu %d host %d; sum of the gpu matrix %.9f"
              % (float(np.abs(betas.cpu().numpy() / betas_h - 1).max()), int(g.values().shape[0]), int(h.nnz),
                 float(g.values().sum(dtype=torch.float64))), flush=True)
        print("host / gpu = %.1f x  (medians of the wall clock)"
              % (statistics.median(r[0] for r in results["host"]) / statistics.median(r[0] for r in results["gpu"])), flush=True)
    moved = 16 * n * k + 4 * n  # int32 ids and float32 distances read; int32 ids, float32 entries and betas written
    buf = torch.empty(moved, dtype=torch.uint8, device="cuda:0")
    sets = [timed(lambda: buf.zero_())[1] for _ in range(args.reps + 1)][1:]
    print("k_perplexity_search moves %d bytes once; a memset of as many: median %.3f ms of stream time (%.0f GB/s)"
          % (moved, statistics.median(sets), moved / statistics.median(sets) / 1e6), flush=True)


if __name__ == "__main__":
    main()
