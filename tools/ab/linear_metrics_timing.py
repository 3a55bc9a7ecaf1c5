"""What the metrics with a linear map cost at 1 M x 128 float32 (k = 15, the benchmark's stand-in data, rows on the device): one
process, the legs alternating, one warm-up of each, then REPS timed repetitions.

  euclidean    NNDescent(T, "euclidean"): the build of rows transformed beforehand -- the yardstick
  mahalanobis  NNDescent(x, "mahalanobis", {"VI": VI}): the dense map (parse + factor on the host, the shift's sample, the
               transform kernel, then the same build)
  seuclidean   NNDescent(x, "seuclidean", {"V": V}): the diagonal map
  kernel       k_linear_rows alone, dense and diagonal, in stream time between two events, with its achieved bytes/s against
               the floor of 2 * n * d * 4 bytes (every row read once and written once)

A metric build should cost the euclidean build plus the transform pass; the host-side stages of the metric legs (metric_kwds
parsed and VI factored, the shift's strided sample gathered and averaged, the map uploaded and the rows transformed) are timed
inside the build and listed, so the log says where any rest goes.  The clock is the host's, from a device synchronise to a
device synchronise.  Run from the repository root:

    python tools/ab/linear_metrics_timing.py [--n N] [--d D] [--reps R]
"""
import argparse
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch

    import bench
    from pynndescent_amd import NNDescent, _capi, linear_map, nndescent

    n, d, k = args.n, args.d, 15
    device = torch.device("cuda:0")
    x = bench.sift_like(n, d, seed=1, device=device, sample_seed=100).contiguous()
    rs = np.random.RandomState(3)
    b = rs.standard_normal((d, d))
    vi = b @ b.T / d + 0.5 * np.eye(d)
    v = x[:: max(1, n // 20000)].double().var(dim=0).cpu().numpy() + 1e-6
    kw = {"mahalanobis": {"VI": vi}, "seuclidean": {"V": v}}

    def line(name, what, values, unit="ms"):
        print("%-12s %-58s min %10.3f  median %10.3f  max %10.3f %s  (%d reps)"
              % (name, what, min(values), statistics.median(values), max(values), unit, len(values)), flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    # the host-side stages of a metric build, timed where they run (each wrapper synchronises: the stages add up on the host clock)
    stages = {}
    real_parse, real_shift, real_rows = linear_map.parse_metric_kwds, linear_map.shift_of, nndescent._DeviceLinear.rows

    def staged(name, fn):
        def wrapper(*a, **kwargs):
            ms, out = timed(lambda: fn(*a, **kwargs))
            stages[name] = stages.get(name, 0.0) + ms
            return out
        return wrapper

    linear_map.parse_metric_kwds = staged("parse", real_parse)
    linear_map.shift_of = staged("shift", real_shift)
    nndescent._DeviceLinear.rows = staged("transform", real_rows)

    # the rows transformed beforehand: the mahalanobis map of an index of x
    lin = real_parse("mahalanobis", kw["mahalanobis"], d)
    lin = lin._replace(shift=real_shift(nndescent._DeviceRowsView(x)))
    dense = nndescent._DeviceLinear(lin, device, 0)
    lin_diag = real_parse("seuclidean", kw["seuclidean"], d)._replace(shift=lin.shift)
    diag = nndescent._DeviceLinear(lin_diag, device, 0)
    t = real_rows(dense, x, _capi.NND_DTYPE_FLOAT32, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    def build(metric):
        stages.clear()
        if metric == "euclidean":
            ms, index = timed(lambda: NNDescent(t, metric="euclidean", n_neighbors=k, n_trees=8, random_state=1234))
        else:
            ms, index = timed(lambda: NNDescent(x, metric=metric, metric_kwds=kw[metric], n_neighbors=k, n_trees=8, random_state=1234))
        return ms, dict(stages), int(index._build_stats["n_iters_run"])

    def kernel(dl):
        out = torch.empty_like(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream()
        e0.record(stream)
        _capi.device_linear_rows(0, stream.cuda_stream, dl.kind, d, dl.a.data_ptr(), dl.shift.data_ptr(), x.data_ptr(), n, out.data_ptr())
        e1.record(stream)
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    legs = ("euclidean", "mahalanobis", "seuclidean")
    results, kernels = {}, {"dense": [], "diagonal": []}
    for name in legs:
        build(name)  # warm-up
    kernel(dense), kernel(diag)
    for _ in range(args.reps):  # alternating, so that drift of the machine lands on every leg alike
        for name in legs:
            results.setdefault(name, []).append(build(name))
        kernels["dense"].append(kernel(dense))
        kernels["diagonal"].append(kernel(diag))
    print("n %d, d %d, k %d, n_trees 8, float32 rows on the device" % (n, d, k), flush=True)
    base = statistics.median(r[0] for r in results["euclidean"])
    for name in legs:
        runs = results[name]
        line(name, "NNDescent(...) + device synchronise (%d iterations)" % runs[0][2], [r[0] for r in runs])
        if name != "euclidean":
            for stage, what in (("parse", "metric_kwds parsed, VI factored (host)"), ("shift", "the shift: strided sample gathered, mean (host)"),
                                ("transform", "map used on the device: conversion + k_linear_rows")):
                line(name, "  " + what, [r[1].get(stage, 0.0) for r in runs])
            med = statistics.median(r[0] for r in runs)
            rest = med - base - sum(statistics.median(r[1].get(s, 0.0) for r in runs) for s in ("parse", "shift", "transform"))
            print("%-12s   median over the euclidean build: %+.3f ms; of that outside the three stages: %+.3f ms" % (name, med - base, rest), flush=True)
    floor = 2 * n * d * 4
    for name in ("dense", "diagonal"):
        line("kernel", "k_linear_rows %s, stream time" % name, kernels[name])
        line("kernel", "  %d bytes (floor: one read, one write), achieved" % floor, [floor / (ms * 1e-3) / 1e12 for ms in kernels[name]], unit="TB/s")
    flop = 2.0 * n * d * d
    line("kernel", "  dense: %.3g flop, achieved" % flop, [flop / (ms * 1e-3) / 1e12 for ms in kernels["dense"]], unit="TFLOP/s")


if __name__ == "__main__":
    main()
