"""What the sparse neighbour matrix of a device-resident index costs at 1 M x 128 float32 (euclidean, k = 15, the benchmark's
stand-in data): one process, ONE built index, the legs alternating, one warm-up of each, then REPS timed repetitions.

  gpu-dir    index.kneighbors_graph()                 the kernels of csrc/csr_graph.hip, a torch.sparse_csr_tensor on the device
  host-dir   neighbor_graph brought down, np.repeat + coo_array(...).tocsr()      what a caller did before the export existed
  gpu-sym    index.kneighbors_graph(symmetric=True)   the min-union with the transpose on the device
  host-sym   A.maximum(A.T) on the host, A the matrix of host-dir (made outside the clock)

The clock is the host's, from a device synchronise to a device synchronise.  The gpu legs also report their stream time (two
events around the call: it holds the kernels, the scans and the waits of the two totals the host reads) against the bytes the
form has to move once: ids and values read, CSR written.  Run from the repository root:

    python tools/ab/graph_export_timing.py [--n N] [--d D] [--reps R]
"""
import argparse
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
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

    def host_directed():
        ids, vals = index.neighbor_graph
        ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
        a = sp.coo_array((vals.ravel(), (np.repeat(np.arange(n, dtype=np.int32), k), ids.ravel())), shape=(n, n)).tocsr()
        return a

    a_host = host_directed()

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, float(e0.elapsed_time(e1)), out

    legs = {
        "gpu-dir": lambda: index.kneighbors_graph(),
        "host-dir": host_directed,
        "gpu-sym": lambda: index.kneighbors_graph(symmetric=True),
        "host-sym": lambda: a_host.maximum(a_host.T),
    }
    results, nnz = {}, {}
    for name, fn in legs.items():
        timed(fn)  # warm-up
    for _ in range(args.reps):  # alternating, so that drift of the machine lands on every leg alike
        for name, fn in legs.items():
            wall, stream, out = timed(fn)
            results.setdefault(name, []).append((wall, stream))
            nnz[name] = int(out.values().shape[0]) if name.startswith("gpu") else int(out.nnz)
            del out
    for name in legs:
        wall = [r[0] for r in results[name]]
        print("%-9s wall   min %9.2f  median %9.2f  max %9.2f ms  (%d reps, nnz %d)"
              % (name, min(wall), statistics.median(wall), max(wall), len(wall), nnz[name]), flush=True)
        if name.startswith("gpu"):
            stream = [r[1] for r in results[name]]
            floor = 8 * n * k + 8 * nnz[name] + 8 * (n + 1)  # ids + values read once, indices + data + indptr written once
            med = statistics.median(stream)
            print("%-9s stream min %9.2f  median %9.2f  max %9.2f ms; bytes that have to move once %d (%.1f GB/s at the median)"
                  % (name, min(stream), med, max(stream), floor, floor / med / 1e6), flush=True)
    # scipy's maximum() leaves out an entry whose result is 0.0: the host's union has lost the stored zeros (the diagonal of a
    # euclidean graph, and duplicates of a point), the device's union keeps them
    zeros = legs["gpu-sym"]().values().eq(0).sum().item()
    print("stored zeros of the device's union: %d" % zeros, flush=True)
    assert nnz["gpu-dir"] == nnz["host-dir"] and nnz["gpu-sym"] == nnz["host-sym"] + zeros
    print("directed:  host / gpu = %.1f x   symmetric: host / gpu = %.1f x  (medians of the wall clock)"
          % (statistics.median(r[0] for r in results["host-dir"]) / statistics.median(r[0] for r in results["gpu-dir"]),
             statistics.median(r[0] for r in results["host-sym"]) / statistics.median(r[0] for r in results["gpu-sym"])), flush=True)


if __name__ == "__main__":
    main()
