"""What a filtered query costs and finds at 1 M x 128 float32 (euclidean, k = 10, epsilon 0.1, the benchmark's stand-in data,
10 000 held-out queries), by selectivity and by path -- and what the unfiltered query costs before and after the change.

Run from the repository root:

    python tools/ab/filtered_query_timing.py [--n N] [--d D] [--nq NQ] [--reps R] [--parent-lib PATH] [--step-timeout SECONDS]
                                             [--selectivities 0.5,0.1,0.01,0.001] [--no-unfiltered]

Without ``--step`` this is the driver: it starts no device work itself and runs the steps below one after the other, each as a
child process of its own under ``timeout`` (one GPU process at a time); a step that fails, is killed or runs out of time ends
the run there.

  sel:S       an index built from a device tensor, the mask ``RandomState(7).random_sample(n) < S`` as a device tensor, device
              queries.  Three legs alternate, one warm-up each, then R timed repetitions (host clock between device synchronises):
                walk    query(q, k, epsilon, filter=mask, filter_mode="walk")
                exact   query(q, k, filter=mask, filter_mode="exact")
                post    what the code could do before: query(q, k', epsilon) with k' = min(256, ceil(k / S)), then the first k
                        allowed ids of every row (torch, on the device; inside the clock)
              For every leg: queries per second from the median, and recall@10 against exact_knn over the allowed rows.
  unfiltered  two searchers filled from the same host arrays of one prepared index, one under this tree's library and one under
              the library at --parent-lib (the parent commit's build), answering the same device queries in turn, R times: the
              time per call of each, the parent's own run-to-run spread, and whether the two outputs are the same bits.
              Without --parent-lib only this tree's library is timed.  Also the recall@10 of the unfiltered query against
              exact_knn over all rows, for the scale of the filtered recalls."""
import argparse
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SELECTIVITIES = ("0.5", "0.1", "0.01", "0.001")
K, EPSILON = 10, 0.1


def driver(args):
    steps = ["sel:" + s for s in args.selectivities.split(",") if s] + ([] if args.no_unfiltered else ["unfiltered"])
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(args.n),
               "--d", str(args.d), "--nq", str(args.nq), "--reps", str(args.reps)]
        if args.parent_lib:
            cmd += ["--parent-lib", args.parent_lib]
        print("==== step %s" % step, flush=True)
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print("step %s ended with status %d: nothing further is started" % (step, rc), flush=True)
            return rc
    return 0


def line(step, leg, what, values, unit="ms"):
    print("%-12s %-7s %-34s min %10.3f  median %10.3f  max %10.3f %s  (%d reps)" % (
        step, leg, what, min(values), statistics.median(values), max(values), unit, len(values)), flush=True)


def build(args):
    import torch

    import bench
    from pynndescent_amd import NNDescent

    device = torch.device("cuda:0")
    x = bench.sift_like(args.n + args.nq, args.d, seed=1, device=device, sample_seed=100)
    rows, q = x[:args.n].contiguous(), x[args.n:].contiguous()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = NNDescent(rows, n_neighbors=15, n_trees=8, random_state=1234)
    index.prepare()
    torch.cuda.synchronize()
    print("%-12s index of %d x %d built and prepared in %.0f ms" % (args.step, args.n, args.d, (time.perf_counter() - t0) * 1e3), flush=True)
    return torch, index, rows, q


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def step_selectivity(args, sel):
    import numpy as np

    from pynndescent_amd import exact_knn

    torch, index, rows, q = build(args)
    n, nq = args.n, args.nq
    mask_host = np.random.RandomState(7).random_sample(n) < sel
    mask = torch.from_numpy(mask_host).to(q.device)
    allowed = torch.nonzero(mask).reshape(-1)
    n_allowed = int(allowed.numel())
    kk = min(K, n_allowed)
    t_idx, _ = exact_knn(rows[allowed], queries=q, k=kk, metric="euclidean")
    truth = allowed[t_idx.long()]
    k_post = min(256, int(math.ceil(K / sel)))
    print("%-12s %d of %d rows allowed; post-filter k' = %d" % (args.step, n_allowed, n, k_post), flush=True)

    def post():
        ids, _ = index.query(q, k=k_post, epsilon=EPSILON)
        ok = (ids >= 0) & mask[ids.clamp(min=0).long()]
        rank = torch.cumsum(ok, 1)
        keep = ok & (rank <= K)
        out = torch.full((nq, K), -1, dtype=torch.int32, device=q.device)
        r, c = torch.nonzero(keep, as_tuple=True)
        out[r, rank[r, c] - 1] = ids[r, c]
        return out

    legs = {"walk": lambda: index.query(q, k=K, epsilon=EPSILON, filter=mask, filter_mode="walk")[0],
            "exact": lambda: index.query(q, k=K, epsilon=EPSILON, filter=mask, filter_mode="exact")[0],
            "post": post}

    def recall(ids):
        hit = (ids[:, :, None] == truth[:, None, :]) & (ids[:, :, None] >= 0)
        return float(hit.any(-1).sum().item()) / float(nq * kk), float((ids >= 0).sum().item()) / nq

    ms, found, spilled = {}, {}, {}
    for name, fn in legs.items():  # warm-up, and the answers
        _, ids = timed(torch, fn)
        found[name] = recall(ids)
        spilled[name] = index._searcher.last_spilled() if name != "exact" else 0
    for _ in range(args.reps):  # alternating, so that drift of the machine lands on every leg alike
        for name, fn in legs.items():
            ms.setdefault(name, []).append(timed(torch, fn)[0])
    for name in legs:
        line(args.step, name, "query of %d + device synchronise" % nq, ms[name])
        print("%-12s %-7s %12.0f queries/s   recall@10 %.4f   %.2f of %d places filled   %d queries on the global-memory tier" % (
            args.step, name, nq / (statistics.median(ms[name]) * 1e-3), found[name][0], found[name][1], K, spilled[name]), flush=True)


def step_unfiltered(args):
    import ctypes as C

    import numpy as np

    from pynndescent_amd import _capi
    from pynndescent_amd.metrics import _metric_of

    torch, index, rows, q = build(args)
    nq = args.nq
    tree = index._search_forest[0] if index._search_forest else None
    host_rows, graph = index._work_rows(), index._search_graph
    create = (host_rows, graph, tree, _metric_of(index.metric).code, index._min_distance, index.n_neighbors, index.search_rng_state)

    def under(lib):
        saved, _capi._lib = _capi._lib, lib
        try:
            return _capi.Searcher(*create)
        finally:
            _capi._lib = saved

    libs = {"new": _capi.load_library()}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        for name, restype, argtypes in _capi._SIGNATURES:
            fn = getattr(parent, name, None)  # (the parent has no filter entries)
            if fn is not None:
                fn.restype, fn.argtypes = restype, argtypes
        libs = {"parent": parent, "new": libs["new"]}
    searchers = {name: under(lib) for name, lib in libs.items()}
    out = {name: (torch.empty((nq, K), dtype=torch.int32, device=q.device), torch.empty((nq, K), dtype=torch.float32, device=q.device))
           for name in libs}
    stream = torch.cuda.current_stream().cuda_stream

    def call(name):
        idx, dist = out[name]
        searchers[name].query_device("float", q.data_ptr(), nq, K, K, EPSILON, idx.data_ptr(), dist.data_ptr(), stream)

    ms = {}
    for name in libs:
        timed(torch, lambda: call(name))
    for _ in range(args.reps):
        for name in libs:
            ms.setdefault(name, []).append(timed(torch, lambda: call(name))[0])
    for name in libs:
        line(args.step, name, "unfiltered query of %d" % nq, ms[name])
    if "parent" in libs:
        same = all(np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)) for a, b in zip(out["parent"], out["new"]))
        spread = max(ms["parent"]) - min(ms["parent"])
        diff = statistics.median(ms["new"]) - statistics.median(ms["parent"])
        print("%-12s new - parent (medians) %+.3f ms; the parent's own spread (max - min) %.3f ms; outputs bit-identical: %s" % (
            args.step, diff, spread, "yes" if same else "NO"), flush=True)
    from pynndescent_amd import exact_knn

    truth, _ = exact_knn(rows, queries=q, k=K, metric="euclidean")
    ids, _ = index.query(q, k=K, epsilon=EPSILON)
    hit = (ids[:, :, None] == truth[:, None, :]).any(-1)
    print("%-12s recall@10 of the unfiltered query against exact_knn over all rows: %.4f" % (args.step, float(hit.sum().item()) / (nq * K)), flush=True)
    for s in searchers.values():
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default=None)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--selectivities", default=",".join(SELECTIVITIES))
    ap.add_argument("--no-unfiltered", action="store_true")
    args = ap.parse_args()
    if args.step is None:
        return driver(args)
    sys.path.insert(0, ROOT)
    if args.step == "unfiltered":
        step_unfiltered(args)
    else:
        step_selectivity(args, float(args.step.split(":", 1)[1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
