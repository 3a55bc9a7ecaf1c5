"""What the shared-neighbour graph of a device-resident index costs at 1 M x 128 float32 (euclidean, k = 15 and k = 30, the
benchmark's stand-in data): one process, ONE built index per k, the legs alternating, one warm-up of each, then REPS timed
repetitions.

  gpu    index.shared_neighbor_graph()     csrc/snn.hip and the min merge of csrc/csr_graph.hip, tensors on the device
  host   neighbor_graph brought down, scipy's A @ A.T (A: the lists and the diagonal) kept on A's pattern, in blocks of rows so
         that the product fits, the Jaccard division, then the union with the transpose: the route the call replaces

The clock is the host's, from a device synchronise to a device synchronise; the gpu leg also reports its stream time (two events
around the call).  Last, for each of the two kernels the bytes it has to move once, the bytes the gather of k_snn_weights asks
for (n k rows of 4 k bytes) and the stream time of a memset of as many bytes.  The kernels' own times are not visible from here:
run the gpu leg alone under a kernel trace (``--gpu-only``) and read the k_snn_sets and k_snn_weights lines of its statistics.
Run from the repository root:

    python tools/ab/snn_graph_timing.py [--n N] [--d D] [--k K [K ...]] [--reps R] [--gpu-only]
"""
import argparse
import os
import statistics
import sys
import time


def host_route(np, sp, ids, block=50_000):
    """Jaccard weights with the rows themselves in their sets, every edge of the lists, then the union."""
    n, k = ids.shape
    rows = np.repeat(np.arange(n, dtype=np.int32), k)
    cols = ids.ravel()
    off = cols != rows  # (the lists hold no id twice; a row that lists itself does not make an edge)
    edges = sp.coo_array((np.ones(int(off.sum()), np.float32), (rows[off], cols[off])), shape=(n, n)).tocsr()
    a = (edges + sp.eye_array(n, dtype=np.float32, format="csr")).tocsr()
    at = a.T.tocsr()
    sizes = np.diff(a.indptr).astype(np.float32)
    parts = []
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        pattern = edges[lo:hi]
        shared = (a[lo:hi] @ at).multiply(pattern).tocsr()  # >= 1 on every edge: both ends hold both ends
        shared.sort_indices()
        i = np.repeat(np.arange(lo, hi), np.diff(shared.indptr))
        shared.data = shared.data / (sizes[i] + sizes[shared.indices] - shared.data)
        parts.append(shared)
    w = sp.vstack(parts, format="csr")
    return w.maximum(w.T.tocsr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--k", type=int, nargs="+", default=[15, 30])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gpu-only", action="store_true", help="the gpu leg alone (for a kernel trace)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import numpy as np
    import scipy.sparse as sp
    import torch

    import bench
    from pynndescent_amd import NNDescent

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
        legs = {"gpu": lambda: index.shared_neighbor_graph()}
        if not args.gpu_only:
            legs["host"] = lambda: host_route(np, sp, index.neighbor_graph[0].cpu().numpy())
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
            nnz = int(kept[name].values().shape[0]) if name == "gpu" else int(kept[name].nnz)
            print("%-5s wall   min %9.2f  median %9.2f  max %9.2f ms  (%d reps, nnz %d)"
                  % (name, min(wall), statistics.median(wall), max(wall), len(wall), nnz), flush=True)
            if name == "gpu":
                stream = [r[1] for r in results[name]]
                print("%-5s stream min %9.2f  median %9.2f  max %9.2f ms" % (name, min(stream), statistics.median(stream), max(stream)), flush=True)
        if not args.gpu_only:
            g, h = kept["gpu"], kept["host"]
            h.sort_indices()
            same = (int(g.values().shape[0]) == int(h.nnz) and np.array_equal(g.col_indices().cpu().numpy(), h.indices)
                    and float(np.abs(g.values().cpu().numpy() - h.data).max()) <= 2.0 ** -24)
            print("same pattern, weights within one float32 rounding: %s; nnz gpu %d host %d" % (same, int(g.values().shape[0]), int(h.nnz)), flush=True)
            print("host / gpu = %.1f x  (medians of the wall clock)"
                  % (statistics.median(r[0] for r in results["host"]) / statistics.median(r[0] for r in results["gpu"])), flush=True)
        del index, kept
        # int32 ids read, clean lists written | clean lists read once, columns and weights written | the rows the gather asks for
        for what, moved in (("k_snn_sets moves", 8 * n * k), ("k_snn_weights moves", 12 * n * k), ("k_snn_weights' gather asks for", 4 * n * k * k)):
            buf = torch.empty(moved, dtype=torch.uint8, device="cuda:0")
            sets = [timed(lambda: buf.zero_())[1] for _ in range(args.reps + 1)][1:]
            print("%s %d bytes once; a memset of as many: median %.3f ms of stream time (%.0f GB/s)"
                  % (what, moved, statistics.median(sets), moved / statistics.median(sets) / 1e6), flush=True)
            del buf


if __name__ == "__main__":
    main()
