"""What the spanning tree of a device-resident index costs at 1 M x 128 float32 (euclidean, k = 15 and k = 30, min_samples = 5,
the benchmark's stand-in data): one process, ONE built index per k, the legs alternating, one warm-up of each, then REPS timed
repetitions.

  tree    index.spanning_tree()      csrc/mst.hip, then the joining rounds of csrc/cross.hip, tensors on the device
  forest  index.spanning_forest()    csrc/mst.hip alone: what the tree's first half costs by itself

The clock is the host's, from a device synchronise to a device synchronise; each leg also reports its stream time (two events
around the call).  Then the call's statistics: the forest's components, the joining rounds, the query rows (first round and
summed), the rows the float64 tier answered, the data slices, and the f32 MFMA instructions the scans issued -- divided by the
time the tree takes beyond the forest this is a LOWER bound of the scan's issue rate (the difference also holds the refinement,
the round kernels and the final merge); the scan's own time needs the tree leg alone under a kernel trace (``--tree-only``) and
the k_cross_scan line of its statistics.  Run from the repository root:

    python tools/ab/spanning_tree_timing.py [--n N] [--d D] [--k K [K ...]] [--reps R] [--tree-only]
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
    ap.add_argument("--k", type=int, nargs="+", default=[15, 30])
    ap.add_argument("--min-samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tree-only", action="store_true", help="the tree leg alone (for a kernel trace)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import torch

    import bench
    from pynndescent_amd import NNDescent, spanning_tree

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
        legs = {"tree": lambda: index.spanning_tree(min_samples=args.min_samples)}
        if not args.tree_only:
            legs["forest"] = lambda: index.spanning_forest(min_samples=args.min_samples)
        results, kept = {}, {}
        for name, fn in legs.items():
            timed(fn)  # warm-up
        for _ in range(args.reps):  # alternating, so that drift of the machine lands on every leg alike
            for name, fn in legs.items():
                wall, stream, out = timed(fn)
                results.setdefault(name, []).append((wall, stream))
                print("      %-6s %9.2f ms" % (name, wall), file=sys.stderr, flush=True)
                kept[name] = out
        for name in legs:
            wall, stream = [r[0] for r in results[name]], [r[1] for r in results[name]]
            print("%-6s wall   min %9.2f  median %9.2f  max %9.2f ms  (%d reps, %d edges)"
                  % (name, min(wall), statistics.median(wall), max(wall), len(wall), int(kept[name][0].values().shape[0]) // 2), flush=True)
            print("%-6s stream min %9.2f  median %9.2f  max %9.2f ms" % (name, min(stream), statistics.median(stream), max(stream)), flush=True)
        ids, dists = index.neighbor_graph
        stats = spanning_tree(x, ids, dists.float(), "euclidean", args.min_samples, return_stats=True)[3]
        print("statistics of one call: %s" % stats, flush=True)
        if not args.tree_only:
            extra = statistics.median(r[0] for r in results["tree"]) - statistics.median(r[0] for r in results["forest"])
            print("the joining beyond the forest: %.2f ms (medians of the wall clock); %d 16x16x4 f32 MFMA x 2048 flop / that time "
                  ">= %.1f Tflop/s issued by the scans" % (extra, stats["mfma"], stats["mfma"] * 2048 / (extra * 1e-3) / 1e12), flush=True)
        del index, kept


if __name__ == "__main__":
    main()
