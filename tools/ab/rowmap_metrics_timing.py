"""What the two derived metrics cost at 1 M rows (k = 15, rows on the device): one process, each derived metric alternating
with its yardstick (who goes first alternates too), one warm-up of each, then REPS timed repetitions.

  correlation  NNDescent(R, "correlation"): the build of the 1 M x 128 rows ranked beforehand -- the yardstick of ...
  spearmanr    NNDescent(x, "spearmanr"): k_rank_rows, then the same build
  euclidean    NNDescent(P, "euclidean"): the build of the 1 M x 3 sphere rows made beforehand -- the yardstick of ...
  haversine    NNDescent(latlon, "haversine"): the shift's sample (host), k_sphere_rows, then the same build
  kernel       each map kernel alone, in stream time between two events, against its two floors:
                 bytes   one read and one write of the rows: what hipMemsetAsync of a buffer of that many bytes takes on this
                         device (torch's zero_ of a byte tensor; the same stream, the same events)
                 issue   k_rank_rows only: 2 d^2 / 64 compare-and-count wave-instructions per row at 4 cycles each on 1024 SIMDs
                         (4 per CU, 256 CUs) at --ghz (default 2.4)

The clock of the builds is the host's, from a device synchronise to a device synchronise.  Run from the repository root:

    python tools/ab/rowmap_metrics_timing.py [--n N] [--d D] [--reps R]
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
    ap.add_argument("--ghz", type=float, default=2.4, help="SIMD clock for the issue floor")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch

    import bench
    from pynndescent_amd import NNDescent, _capi, nndescent, row_map

    n, d, k = args.n, args.d, 15
    device = torch.device("cuda:0")
    x = bench.sift_like(n, d, seed=1, device=device, sample_seed=100).contiguous()
    rs = np.random.RandomState(3)  # clustered (lat, lon): 2000 centres on the sphere, 0.02 rad of spread
    centres = np.stack([np.arcsin(rs.uniform(-1, 1, 2000)), rs.uniform(-np.pi, np.pi, 2000)], 1)
    latlon = (centres[rs.randint(0, 2000, n)] + rs.standard_normal((n, 2)) * 0.02).astype(np.float32)
    latlon[:, 0] = np.clip(latlon[:, 0], -np.pi / 2, np.pi / 2)
    latlon = torch.from_numpy(latlon).to(device)

    def line(name, what, values, unit="ms"):
        print("%-12s %-62s min %10.3f  median %10.3f  max %10.3f %s  (%d reps)"
              % (name, what, min(values), statistics.median(values), max(values), unit, len(values)), flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    stream = torch.cuda.current_stream()
    rank_map = row_map.RowMap(_capi.NND_ROWMAP_RANK, None)
    sphere_map = row_map.with_shift(row_map.RowMap(_capi.NND_ROWMAP_SPHERE, None), nndescent._DeviceRowsView(latlon))
    ranked = nndescent.device_arrays._device_map(rank_map, device, 0).rows(x, _capi.NND_DTYPE_FLOAT32, stream.cuda_stream)
    sphere = nndescent.device_arrays._device_map(sphere_map, device, 0)
    points = sphere.rows(latlon, _capi.NND_DTYPE_FLOAT32, stream.cuda_stream)
    torch.cuda.synchronize()

    legs = {"correlation": (ranked, "correlation"), "spearmanr": (x, "spearmanr"), "euclidean": (points, "euclidean"),
            "haversine": (latlon, "haversine")}

    def build(name):
        rows, metric = legs[name]
        ms, index = timed(lambda: NNDescent(rows, metric=metric, n_neighbors=k, n_trees=8, random_state=1234))
        return ms, int(index._build_stats["n_iters_run"])

    def stream_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    out_rank, out_sphere = torch.empty_like(x), torch.empty((n, 3), dtype=torch.float32, device=device)
    kernels = {
        "k_rank_rows": (lambda: _capi.device_map_rows(0, stream.cuda_stream, _capi.NND_ROWMAP_RANK, d, d, 0, x.data_ptr(), n, out_rank.data_ptr()),
                        2 * n * d * 4),
        "k_sphere_rows": (lambda: _capi.device_map_rows(0, stream.cuda_stream, _capi.NND_ROWMAP_SPHERE, 2, 2, sphere.shift.data_ptr(),
                                                        latlon.data_ptr(), n, out_sphere.data_ptr()), n * (2 + 3) * 4),
    }
    memset_buffers = {name: torch.empty((nbytes,), dtype=torch.uint8, device=device) for name, (_, nbytes) in kernels.items()}

    # A build that follows a build of another shape costs 5 - 6 ms more than one that follows its own shape (seen with the four
    # legs in one rotation: the handle's buffers are reused only for the same shape), so each derived metric alternates with its
    # own yardstick alone -- both work on rows of one shape -- and who goes first alternates too.
    results, kernel_ms, memset_ms = {}, {}, {}
    for pair in (("correlation", "spearmanr"), ("euclidean", "haversine")):
        for name in pair:
            build(name)  # warm-up
        for rep in range(args.reps):
            for name in (pair if rep % 2 == 0 else pair[::-1]):
                results.setdefault(name, []).append(build(name))
    for name, (fn, _) in kernels.items():
        stream_ms(fn), stream_ms(memset_buffers[name].zero_)
    for rep in range(args.reps):
        for name, (fn, _) in kernels.items():
            kernel_ms.setdefault(name, []).append(stream_ms(fn))
            memset_ms.setdefault(name, []).append(stream_ms(memset_buffers[name].zero_))
    print("n %d, k %d, n_trees 8, float32 rows on the device; spearmanr legs d = %d, haversine legs 2 -> 3 columns" % (n, k, d), flush=True)
    for name in legs:
        line(name, "NNDescent(...) + device synchronise (%d iterations)" % results[name][0][1], [r[0] for r in results[name]])
        print("%-12s   the repetitions in order: %s" % (name, "  ".join("%.3f" % r[0] for r in results[name])), flush=True)
    for derived, base in (("spearmanr", "correlation"), ("haversine", "euclidean")):
        print("%-12s median over the %s build of rows mapped beforehand: %+.3f ms"
              % (derived, base, statistics.median(r[0] for r in results[derived]) - statistics.median(r[0] for r in results[base])), flush=True)
    for name, (_, nbytes) in kernels.items():
        line("kernel", "%s, stream time" % name, kernel_ms[name])
        line("kernel", "  bytes floor: memset of %d bytes (one read + one write of the rows)" % nbytes, memset_ms[name])
        line("kernel", "  achieved over those bytes", [nbytes / (ms * 1e-3) / 1e12 for ms in kernel_ms[name]], unit="TB/s")
    insts = 2.0 * d * d / 64.0 * n
    issue_ms = insts * 4.0 / 1024.0 / (args.ghz * 1e9) * 1e3
    print("%-12s   issue floor of k_rank_rows: %.3g wave-instructions, 4 cycles each on 1024 SIMDs at %.2f GHz: %.3f ms; the kernel's median is "
          "%.2f x that" % ("kernel", insts, args.ghz, issue_ms, statistics.median(kernel_ms["k_rank_rows"]) / issue_ms), flush=True)
    assert torch.equal(out_rank, ranked) and torch.equal(out_sphere, points)


if __name__ == "__main__":
    main()
