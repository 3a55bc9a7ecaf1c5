"""What the spanning forest of a device-resident index costs at 1 M x 128 float32 (euclidean, k = 15 and k = 30,
min_samples = 5, the benchmark's stand-in data): one process, ONE built index per k, the legs alternating, one warm-up of
each, then REPS timed repetitions.

  gpu    index.spanning_forest()     csrc/mst.hip and the min merge of csrc/csr_graph.hip, tensors on the device
  host   neighbor_graph brought down, the core distances and the min-combined mutual-reachability matrix with numpy and scipy,
         then scipy.sparse.csgraph's connected_components and minimum_spanning_tree: the route the call replaces

The clock is the host's, from a device synchronise to a device synchronise; the gpu leg also reports its stream time (two events
around the call) and the Boruvka rounds.  Last, the bytes k_mst_scan asks for in its first rounds -- per entry of the symmetric
matrix a column and a weight read in order and one gathered component id -- next to the stream time of a memset of as many.  The
kernels' own times are not visible from here: run the gpu leg alone under a kernel trace (``--gpu-only``) and read the k_mst_*
lines of its statistics.  Run from the repository root:

    python tools/ab/spanning_forest_timing.py [--n N] [--d D] [--k K [K ...]] [--reps R] [--gpu-only]
"""
import argparse
import os
import statistics
import sys
import time


def host_route(np, sp, csgraph, ids, dists, min_samples):
    """Core distances (the row's own place counts), max(core(i), core(j), d) per edge, the smaller of an edge and its twin,
    then the components and the spanning tree.  (scipy's tree drops zero weights: the stand-in data has none.)"""
    n, k = ids.shape
    core = np.sort(dists, axis=1)[:, min_samples - 1]
    rows = np.repeat(np.arange(n, dtype=np.int32), k)
    cols = ids.ravel()
    w = np.maximum(np.maximum(core[rows], core[cols]), dists.ravel())
    off = cols != rows
    a = sp.coo_array((w[off], (rows[off], cols[off])), shape=(n, n)).tocsr()
    at = a.T.tocsr()
    larger, smaller = a.maximum(at), a.minimum(at)  # smaller: 0 where one direction alone is stored
    graph = (larger - larger.multiply(smaller > 0) + smaller).tocsr()  # the smaller where both are, else the one there is
    graph.eliminate_zeros()
    n_components, labels = csgraph.connected_components(graph, directed=False)
    tree = csgraph.minimum_spanning_tree(graph)
    return tree, labels, core


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, nargs="+", default=[15, 30])
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpu-only", action="store_true", help="the gpu leg alone (for a kernel trace)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import numpy as np
    import scipy.sparse as sp
    import torch
    from scipy.sparse import csgraph

    import bench
    from pynndescent_amd import NNDescent, _capi

    n, d = args.n, args.d
    x = bench.sift_like(n, d, seed=1, device=torch.device("cuda:0"), sample_seed=100)
    torch.cuda.synchronize()

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(e0.elapsed_time(e1)), out

    for k in args.k:
        index = NNDescent(x, n_neighbors=k, n_trees=8, random_state=1234)
        torch.cuda.synchronize()
        print("---- k = %d: index of %d x %d built" % (k, n, d), flush=True)
        legs = {"gpu": lambda: index.spanning_forest(min_samples=args.min_samples)}
        if not args.gpu_only:
            legs["host"] = lambda: host_route(np, sp, csgraph, index.neighbor_graph[0].cpu().numpy(), index.neighbor_graph[1].cpu().numpy(),
                                              args.min_samples)
        results, kept = {}, {}
        for name, fn in legs.items():
            timed(fn)  # warm-up
        for _ in range(args.reps):  # alternating, so that drift of the machine lands on every leg alike
            for name, fn in legs.items():
                wall, stream, out = timed(fn)
                results.setdefault(name, []).append((wall, stream))
                print("      %-5s %9.2f ms" % (name, wall), file=sys.stderr, flush=True)
                kept[name] = out
        for name in legs:
            wall = [r[0] for r in results[name]]
            edges = int(kept[name][0].values().shape[0]) // 2 if name == "gpu" else int(kept[name][0].nnz)
            print("%-5s wall   min %9.2f  median %9.2f  max %9.2f ms  (%d reps, %d forest edges, %d components)"
                  % (name, min(wall), statistics.median(wall), max(wall), len(wall), edges, int(kept[name][1].max()) + 1), flush=True)
            if name == "gpu":
                stream = [r[1] for r in results[name]]
                print("%-5s stream min %9.2f  median %9.2f  max %9.2f ms" % (name, min(stream), statistics.median(stream), max(stream)), flush=True)
        ids, dists = index.neighbor_graph[0].cpu().numpy(), index.neighbor_graph[1].cpu().numpy()
        rounds = _capi.spanning_forest(ids, dists, args.min_samples, want_rounds=True)[5]
        sym = int(index.kneighbors_graph(symmetric=True, include_self=False).values().shape[0])
        print("rounds that joined components: %d (and one that found nothing to join); entries of the symmetric matrix: %d" % (rounds, sym), flush=True)
        if not args.gpu_only:
            (g, gl, gc), (h, hl, hc) = kept["gpu"], kept["host"]
            same = (np.array_equal(gl.cpu().numpy(), hl) and np.array_equal(gc.cpu().numpy(), hc)
                    and np.array_equal(np.sort(g.values().cpu().numpy().astype(np.float64))[::2], np.sort(h.data)))
            print("same labels, core distances and sorted tree weights: %s" % same, flush=True)
            print("host / gpu = %.1f x  (medians of the wall clock)"
                  % (statistics.median(r[0] for r in results["host"]) / statistics.median(r[0] for r in results["gpu"])), flush=True)
        del index, kept
        # per entry: column and weight in order (8 bytes), the other end's component gathered (4 bytes; round 0 gathers nothing)
        for what, moved in (("k_mst_scan reads in order", 8 * sym), ("k_mst_scan's gather asks for", 4 * sym)):
            buf = torch.empty(moved, dtype=torch.uint8, device="cuda:0")
            sets = [timed(lambda: buf.zero_())[1] for _ in range(args.reps + 1)][1:]
            print("%s %d bytes a round; a memset of as many: median %.3f ms of stream time (%.0f GB/s)"
                  % (what, moved, statistics.median(sets), moved / statistics.median(sets) / 1e6), flush=True)
            del buf


if __name__ == "__main__":
    main()
