"""What a caller of the public class pays at 1 M x 128 (euclidean, k = 15, 8 trees, the benchmark's stand-in data), by where the
input lives: one process, one warm-up of every leg, then REPS timed repetitions each.

  a  NNDescent(x_numpy).neighbor_graph                      host buffers in and out
  b  NNDescent(x_cuda).neighbor_graph, to a stream sync     device array in, device tensors out
  c  b with a float16 tensor                                converted on the device
  d  the bare set_data_device + build_device loop of bench.py: the floor

Run from the repository root:  python tools/ab/device_arrays_timing.py [--legs a,b,c,d] [--root OTHER_TREE] [--label NAME]
``--root``: import the package and bench.py from another checkout (a parent commit knows legs a and d only).  One line per leg:
min / median / max in ms; legs b and c also split into constructor, neighbor_graph and the device stages the build reports."""
import argparse
import os
import statistics
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    import bench
    from pynndescent_amd import NNDescent, _capi

    legs = args.legs.split(",")
    n, d, k, n_trees = args.n, args.d, 15, 8
    device = torch.device("cuda:0")
    x = bench.sift_like(n, d, seed=1, device=device, sample_seed=100)
    torch.cuda.synchronize()
    x_host = x.cpu().numpy()
    x16 = x.half()
    kw = dict(n_neighbors=k, n_trees=n_trees, random_state=1234)

    def line(name, what, ms):
        print("%-8s %-10s %-52s min %8.2f  median %8.2f  max %8.2f ms  (%d reps)"
              % (args.label, name, what, min(ms), statistics.median(ms), max(ms), len(ms)), flush=True)

    def host_leg():
        t0 = time.perf_counter()
        NNDescent(x_host, **kw).neighbor_graph
        return (time.perf_counter() - t0) * 1e3, None

    def device_leg(xt):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = NNDescent(xt, **kw)
        t1 = time.perf_counter()
        graph = index.neighbor_graph
        torch.cuda.current_stream().synchronize()
        t2 = time.perf_counter()
        st = index._build_stats
        stages = sum(st[s] for s in ("ms_prep", "ms_forest", "ms_leaf_init", "ms_random_init", "ms_descent", "ms_finalize"))
        del graph
        return (t2 - t0) * 1e3, ((t1 - t0) * 1e3, (t2 - t1) * 1e3, stages)

    def floor_leg(state={}):
        if not state:
            lim = np.iinfo(np.int32)
            rs = np.random.RandomState(1234)
            rng_state = rs.randint(lim.min + 1, lim.max - 1, 3).astype(np.int64)
            rs.randint(lim.min + 1, lim.max - 1, 3)
            tree_states = rs.randint(lim.min + 1, lim.max - 1, size=(n_trees, 3)).astype(np.int64)
            state["b"] = _capi.Builder(n, d, _capi.NND_METRIC_SQEUCLIDEAN, k, n_trees, max(60, min(256, 5 * k)), 200, min(60, k),
                                       max(5, int(round(np.log2(n)))), 0.001, rng_state, tree_states[0], device=0)
            state["oi"] = torch.empty((n, k), dtype=torch.int32, device=device)
            state["od"] = torch.empty((n, k), dtype=torch.float32, device=device)
            torch.cuda.synchronize()
        b = state["b"]
        b.synchronize()
        t0 = time.perf_counter()
        b.set_data_device(x.data_ptr(), keepalive=x)
        b.build_device(state["oi"].data_ptr(), state["od"].data_ptr())
        b.synchronize()
        return (time.perf_counter() - t0) * 1e3, None

    table = {"a": ("NNDescent(x_numpy).neighbor_graph", host_leg),
             "b": ("NNDescent(x_cuda float32).neighbor_graph + stream sync", lambda: device_leg(x)),
             "c": ("NNDescent(x_cuda float16).neighbor_graph + stream sync", lambda: device_leg(x16)),
             "d": ("set_data_device + build_device (bench.py's loop)", floor_leg)}
    for name in legs:
        what, fn = table[name]
        fn()  # warm-up
        runs = [fn() for _ in range(args.reps)]
        line(name, what, [r[0] for r in runs])
        if runs[0][1] is not None:
            for i, part in enumerate(("constructor", "neighbor_graph (clone, correction, sync)", "device stages reported by the build")):
                line(name + "." + str(i + 1), part, [r[1][i] for r in runs])


if __name__ == "__main__":
    main()
