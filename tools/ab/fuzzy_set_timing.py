"""What UMAP's fuzzy simplicial set of a device-resident index costs at 1 M x 128 float32 (euclidean, k = 15, the benchmark's
stand-in data): one process, ONE built index, the legs alternating, one warm-up of each, then REPS timed repetitions.

  gpu    index.fuzzy_simplicial_set()      csrc/fuzzy.hip and the fuzzy merge of csrc/csr_graph.hip, tensors on the device
  host   neighbor_graph brought down, smooth_knn_dist and the membership strengths restated in numpy over all rows at once
         (float32, what numba runs), then scipy's A + A.T - A.multiply(A.T): the route the call replaces

The clock is the host's, from a device synchronise to a device synchronise; the gpu leg also reports its stream time (two events
around the call).  Last, the bytes k_smooth_knn has to move once (ids and distances read; ids, weights, sigmas and rhos written)
and the stream time of a memset of that many bytes.  The kernel's own time is not visible from here: run the gpu leg alone
under a kernel trace (``--gpu-only``) and read the k_smooth_knn line of its statistics.  Run from the repository root:

    python tools/ab/fuzzy_set_timing.py [--n N] [--d D] [--reps R] [--gpu-only]
"""
import argparse
import os
import statistics
import sys
import time


def host_route(np, sp, ids, dists):
    """Steps 1-3 for local_connectivity = bandwidth = 1 on every row at once, then the union (mix = 1)."""
    n, k = ids.shape
    target = np.float32(np.log2(k))
    positive = dists > 0
    first = np.argmax(positive, axis=1)  # nz[0]: the first positive distance of the row
    rho = np.where(positive.any(axis=1), dists[np.arange(n), first], np.float32(0)).astype(np.float32)
    gap = np.maximum(dists[:, 1:] - rho[:, None], np.float32(0))
    lo, hi, mid = np.zeros(n, np.float32), np.full(n, np.inf, np.float32), np.ones(n, np.float32)
    live = np.ones(n, bool)
    for _ in range(64):
        psum = np.exp(-gap / mid[:, None]).sum(axis=1, dtype=np.float32)
        live &= ~(np.abs(psum - target) < np.float32(1e-5))
        if not live.any():
            break
        over = psum > target
        new_hi = np.where(over, mid, hi)
        new_lo = np.where(over, lo, mid)
        new_mid = np.where(over | np.isfinite(new_hi), (new_lo + new_hi) / 2, mid * 2).astype(np.float32)
        lo, hi, mid = np.where(live, new_lo, lo), np.where(live, new_hi, hi), np.where(live, new_mid, mid)
    floor = np.where(rho > 0, dists.mean(axis=1, dtype=np.float64), dists.mean(dtype=np.float64)) * 1e-3
    sigma = np.maximum(mid, floor).astype(np.float32)
    w = np.exp(-np.maximum(dists - rho[:, None], np.float32(0)) / sigma[:, None]).astype(np.float32)
    w[ids == np.arange(n)[:, None]] = 0
    a = sp.coo_array((w.ravel(), (np.repeat(np.arange(n, dtype=np.int32), k), ids.ravel())), shape=(n, n)).tocsr()
    a.eliminate_zeros()
    t = a.T.tocsr()
    return a + t - a.multiply(t), sigma, rho


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpu-only", action="store_true", help="the gpu leg alone (for a kernel trace)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import numpy as np
    import scipy.sparse as sp
    import torch

    import bench
    from pynndescent_amd import NNDescent

    n, d, k = args.n, args.d, 15
    x = bench.sift_like(n, d, seed=1, device=torch.device("cuda:0"), sample_seed=100)
    torch.cuda.synchronize()
    index = NNDescent(x, n_neighbors=k, n_trees=8, random_state=1234)
    torch.cuda.synchronize()

    def host():
        ids, dists = index.neighbor_graph
        return host_route(np, sp, ids.cpu().numpy(), dists.cpu().numpy().astype(np.float32))

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(e0.elapsed_time(e1)), out

    legs = {"gpu": lambda: index.fuzzy_simplicial_set()}
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
        nnz = int(kept[name][0].values().shape[0]) if name == "gpu" else int(kept[name][0].nnz)
        print("%-5s wall   min %9.2f  median %9.2f  max %9.2f ms  (%d reps, nnz %d)"
              % (name, min(wall), statistics.median(wall), max(wall), len(wall), nnz), flush=True)
        if name == "gpu":
            stream = [r[1] for r in results[name]]
            print("%-5s stream min %9.2f  median %9.2f  max %9.2f ms" % (name, min(stream), statistics.median(stream), max(stream)), flush=True)
    if not args.gpu_only:
        (g, sigmas, rhos), (h, sigmas_h, rhos_h) = kept["gpu"], kept["host"]
        print("rhos equal: %s; largest relative difference of the sigmas %.3g; nnz gpu %d host %d"
              % (bool((rhos.cpu().numpy() == rhos_h).all()), float(np.abs(sigmas.cpu().numpy() / sigmas_h - 1).max()),
                 int(g.values().shape[0]), int(h.nnz)), flush=True)
        print("host / gpu = %.1f x  (medians of the wall clock)"
              % (statistics.median(r[0] for r in results["host"]) / statistics.median(r[0] for r in results["gpu"])), flush=True)
    moved = 16 * n * k + 8 * n  # int32 ids and float32 distances read; int32 ids, float32 weights, sigmas and rhos written
    buf = torch.empty(moved, dtype=torch.uint8, device="cuda:0")
    sets = [timed(lambda: buf.zero_())[1] for _ in range(args.reps + 1)][1:]
    print("k_smooth_knn moves %d bytes once; a memset of as many: median %.3f ms of stream time (%.0f GB/s)"
          % (moved, statistics.median(sets), moved / statistics.median(sets) / 1e6), flush=True)


if __name__ == "__main__":
    main()
