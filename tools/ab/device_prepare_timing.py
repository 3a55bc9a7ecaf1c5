"""What prepare() of an index built from a device array costs at 1 M x 128 float32 (euclidean, k = 15, the benchmark's stand-in
data), by the path it takes: one process, ONE graph, the two paths alternating, one warm-up of each, then REPS timed repetitions.

  device   prepare() from the device tensors (hub rank, tree, pruning pass, reorder, searcher fill on the device)
  host     the same index with ``_host_prepare = True``: the path of a host-built index (mirrors fetched, three uploads of the
           rows, the scipy reorder) -- the code every prepare() took before the device path existed

Every repetition prepares a fresh shallow copy of the one built index (same tensors, no prepared state, no cached mirror), so a
host repetition pays for its mirrors as a caller's first prepare() does.  The clock is the host's, around prepare(), from a
device synchronise to a device synchronise.  Run from the repository root:

    python tools/ab/device_prepare_timing.py [--legs device,host] [--root OTHER_TREE] [--label NAME] [--n N] [--d D] [--reps R]

``--root``: import the package and bench.py from another checkout; a tree without the device path knows the host leg only
(``--legs host``), and its figures next to this tree's host leg show that the switch reproduces it.  One line per leg: min /
median / max in ms; the device leg also splits into the stream time of its stages, and both legs list the bytes they copy
between host and device, counted from the arrays they move."""
import argparse
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="device,host")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    import bench
    from pynndescent_amd import NNDescent

    legs = args.legs.split(",")
    n, d, k = args.n, args.d, 15
    device = torch.device("cuda:0")
    x = bench.sift_like(n, d, seed=1, device=device, sample_seed=100)
    torch.cuda.synchronize()
    base = NNDescent(x, n_neighbors=k, n_trees=8, random_state=1234)
    torch.cuda.synchronize()
    pristine = dict(base.__dict__)  # tensors by reference; neither a mirror nor prepared state

    def line(name, what, ms):
        print("%-10s %-8s %-44s min %9.2f  median %9.2f  max %9.2f ms  (%d reps)"
              % (args.label, name, what, min(ms), statistics.median(ms), max(ms), len(ms)), flush=True)

    def leg(host):
        index = object.__new__(NNDescent)
        index.__dict__.update(pristine)
        if host:
            index._host_prepare = True
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index.prepare()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        took_device = "_device_search_graph" in index.__dict__
        assert took_device == (not host), "the leg did not take its path"
        nnz = int(index._search_graph.nnz)  # (after the clock: on the device leg this read is what fetches the mirror)
        nodes = int(index._search_forest[0].hyperplanes.shape[0]) if index._search_forest else 0
        stats = dict(index.__dict__.get("_device_prepare_stats", {}))
        return ms, stats, nnz, nodes

    results = {}
    for name in legs:
        leg(name == "host")  # warm-up
    for _ in range(args.reps):  # alternating, so that drift of the machine lands on both legs alike
        for name in legs:
            results.setdefault(name, []).append(leg(name == "host"))
    for name in legs:
        runs = results[name]
        line(name, "prepare() + device synchronise", [r[0] for r in runs])
        for stage in ("ms_rank", "ms_hub_tree", "ms_search_graph", "ms_reorder", "ms_searcher_fill"):
            if all(stage in r[1] for r in runs):
                line(name, "  stream time: " + stage, [r[1][stage] for r in runs])
        nnz, nodes = runs[0][2], runs[0][3]
        tree = nodes * d * 4 + nodes * 4 + nodes * 8 + n * 4  # hyperplanes, offsets, children, indices
        rows, graph, csr = 4 * n * d, 8 * n * k, 4 * (n + 1) + 4 * nnz
        if name == "host":  # mirrors down; rows up three times (tree, pass, searcher), graph and rank order up, CSR down and up
            down, up = rows + graph + tree + csr, 3 * rows + graph + 4 * n + csr + tree
        else:  # tree tables down, leaf order up, tree tables up with the searcher
            down, up = tree, 4 * n + tree
        print("%-10s %-8s bytes device -> host %13d   host -> device %13d   (n %d, d %d, k %d, nnz %d, tree nodes %d)"
              % (args.label, name, down, up, n, d, k, nnz, nodes), flush=True)
        if name == "device":
            print("%-10s %-8s device bytes of the reorder: CSR read + written %d, rows read + written %d"
                  % (args.label, name, 2 * csr, 2 * rows), flush=True)


if __name__ == "__main__":
    main()
