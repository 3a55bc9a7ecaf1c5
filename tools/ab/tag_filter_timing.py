"""What per-query filters cost and find at 1 M x 128 float32 (euclidean, k = 10, epsilon 0.1, the benchmark's stand-in data,
10 000 held-out queries): 64 tags in four bands of 16 whose per-tag selectivities are 0.5 / 0.1 / 0.01 / 0.001, one tag per query.

Run from the repository root, and keep the output as profiles/tag_filter_1m.txt:

    python tools/ab/tag_filter_timing.py [--n N] [--d D] [--nq NQ] [--reps R] [--parent-lib PATH] [--step-timeout SECONDS]
                                         [--bands 0.5,0.1,0.01,0.001] [--no-parent]

Without ``--step`` this is the driver: it starts no device work itself and runs the steps below one after the other, each as a
child process of its own under ``timeout`` (one GPU process at a time); a step that fails, is killed or runs out of time ends
the run there.

  band:S   an index built from a device tensor with the 64 tag words set as a device tensor; every query takes one of the 16 tags
           of the band of selectivity S (query i: tag i % 16 of the band), masks and queries on the device.  Three legs alternate,
           one warm-up each, then R timed repetitions (host clock between device synchronises):
             walk     query(q, k, epsilon, query_tags=masks, filter_mode="walk")
             exact    query(q, k, query_tags=masks, filter_mode="exact")
             percall  the only route the parent commit has: one query(q[its queries], filter=(tags & mask) != 0) call per
                      distinct mask (filter_mode="auto"), the answers scattered back
           For every leg the median, queries per second, and for walk and percall recall@10 against the masked exact answers.
           The two bracketing measurements of the crossing of walk and exact go next to filtered.TAG_EXACT_MAX_ROWS.
  parent   two searchers filled from the same host arrays of one prepared index, one under this tree's library and one under
           the library at --parent-lib (the parent commit's build), answering the same device queries in turn, R times, once
           unfiltered and once under one allow set (selectivity 0.1): the time per call of each, the parent's own run-to-run
           spread, and whether the two outputs are the same bits.  Their kernels are unchanged: new - parent must stay within
           that spread."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
BANDS = ("0.5", "0.1", "0.01", "0.001")
TAGS_PER_BAND = 16
K, EPSILON = 10, 0.1


def driver(args):
    steps = ["band:" + s for s in args.bands.split(",") if s] + ([] if args.no_parent or not args.parent_lib else ["parent"])
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(args.n),
               "--d", str(args.d), "--nq", str(args.nq), "--reps", str(args.reps), "--bands", args.bands]
        if args.parent_lib:
            cmd += ["--parent-lib", args.parent_lib]
        print("==== step %s" % step, flush=True)
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            print("step %s ended with status %d: nothing further is started" % (step, rc), flush=True)
            return rc
    return 0


def tag_words(n, bands):
    """n uint64 words: tag 16 b + t (t < 16) on about bands[b] of the rows, every tag drawn on its own."""
    import numpy as np

    rs = np.random.RandomState(7)
    tags = np.zeros(n, np.uint64)
    for b, sel in enumerate(bands):
        for t in range(TAGS_PER_BAND):
            tags[rs.random_sample(n) < sel] |= np.uint64(1) << np.uint64(TAGS_PER_BAND * b + t)
    return tags


def step_band(args, sel):
    import numpy as np

    import filtered_query_timing as FQ

    torch, index, rows, q = FQ.build(args)
    n, nq = args.n, args.nq
    bands = [float(s) for s in args.bands.split(",") if s]
    band = bands.index(sel)
    tags_host = tag_words(n, bands)
    tags = torch.from_numpy(tags_host.view(np.int64)).to(q.device)
    index.set_row_tags(tags)
    masks_host = np.uint64(1) << (np.uint64(TAGS_PER_BAND * band) + (np.arange(nq) % TAGS_PER_BAND).astype(np.uint64))
    masks = torch.from_numpy(masks_host.view(np.int64)).to(q.device)
    distinct = np.unique(masks_host)
    groups = [(torch.from_numpy(np.flatnonzero(masks_host == m)).to(q.device), (tags & int(np.int64(np.uint64(m).view(np.int64)))) != 0) for m in distinct]
    counts = [int(g[1].sum().item()) for g in groups]
    print("%-12s %d distinct masks; rows allowed per mask: min %d, median %d, max %d" % (
        args.step, len(distinct), min(counts), int(statistics.median(counts)), max(counts)), flush=True)

    def percall():
        out = torch.full((nq, K), -1, dtype=torch.int32, device=q.device)
        for where, allow in groups:
            out[where] = index.query(q[where], k=K, epsilon=EPSILON, filter=allow)[0]
        return out

    legs = {"walk": lambda: index.query(q, k=K, epsilon=EPSILON, query_tags=masks, filter_mode="walk")[0],
            "exact": lambda: index.query(q, k=K, epsilon=EPSILON, query_tags=masks, filter_mode="exact")[0],
            "percall": percall}
    ms, answers = {}, {}
    for name, fn in legs.items():  # warm-up, and the answers
        answers[name] = FQ.timed(torch, fn)[1]
    truth = answers["exact"]
    for _ in range(args.reps):  # alternating, so that drift of the machine lands on every leg alike
        for name, fn in legs.items():
            ms.setdefault(name, []).append(FQ.timed(torch, fn)[0])
    places = float((truth >= 0).sum().item())
    for name in legs:
        FQ.line(args.step, name, "query of %d + device synchronise" % nq, ms[name])
        ids = answers[name]
        hit = ((ids[:, :, None] == truth[:, None, :]) & (ids[:, :, None] >= 0)).any(-1)
        print("%-12s %-7s %12.0f queries/s   recall@10 against the masked exact answers %.4f   %.2f of %d places filled" % (
            args.step, name, nq / (statistics.median(ms[name]) * 1e-3), float(hit.sum().item()) / places, float((ids >= 0).sum().item()) / nq, K),
            flush=True)


def step_parent(args):
    import ctypes as C

    import numpy as np

    import filtered_query_timing as FQ
    from pynndescent_amd import _capi
    from pynndescent_amd.metrics import _metric_of

    torch, index, rows, q = FQ.build(args)
    nq = args.nq
    tree = index._search_forest[0] if index._search_forest else None
    create = (index._work_rows(), index._search_graph, tree, _metric_of(index.metric).code, index._min_distance, index.n_neighbors,
              index.search_rng_state)
    parent = C.CDLL(os.path.abspath(args.parent_lib))
    for name, restype, argtypes in _capi._SIGNATURES:
        fn = getattr(parent, name, None)  # (the parent has no tag entries)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    libs = {"parent": parent, "new": _capi.load_library()}
    searchers = {}
    for name, lib in libs.items():
        saved, _capi._lib = _capi._lib, lib
        try:
            searchers[name] = _capi.Searcher(*create)
        finally:
            _capi._lib = saved
    out = {name: (torch.empty((nq, K), dtype=torch.int32, device=q.device), torch.empty((nq, K), dtype=torch.float32, device=q.device))
           for name in libs}
    stream = torch.cuda.current_stream().cuda_stream
    allow = np.random.RandomState(7).random_sample(args.n) < 0.1

    def call(name):
        idx, dist = out[name]
        searchers[name].query_device("float", q.data_ptr(), nq, K, K, EPSILON, idx.data_ptr(), dist.data_ptr(), stream)

    for what in ("unfiltered", "single set 0.1"):
        if what != "unfiltered":
            for s in searchers.values():
                s.set_filter(allow, index._vertex_order)
        ms = {}
        for name in libs:
            FQ.timed(torch, lambda: call(name))
        for _ in range(args.reps):
            for name in libs:
                ms.setdefault(name, []).append(FQ.timed(torch, lambda: call(name))[0])
        for name in libs:
            FQ.line(args.step, name, "%s query of %d" % (what, nq), ms[name])
        same = all(np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32)) for a, b in zip(out["parent"], out["new"]))
        print("%-12s %s: new - parent (medians) %+.3f ms; the parent's own spread (max - min) %.3f ms; outputs bit-identical: %s" % (
            args.step, what, statistics.median(ms["new"]) - statistics.median(ms["parent"]), max(ms["parent"]) - min(ms["parent"]),
            "yes" if same else "NO"), flush=True)
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
    ap.add_argument("--bands", default=",".join(BANDS))
    ap.add_argument("--no-parent", action="store_true")
    args = ap.parse_args()
    if args.step is None:
        return driver(args)
    sys.path.insert(0, ROOT)
    if args.step == "parent":
        step_parent(args)
    else:
        step_band(args, float(args.step.split(":", 1)[1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
