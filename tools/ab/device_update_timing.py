"""What update() and recall() of an index built from a device array cost at 1 M x 128 float32 (euclidean, k = 15, the benchmark's
stand-in data), by the path they take: one process, ONE built index, the two paths alternating, one warm-up of each, then REPS
timed repetitions.

  device   update(xs_fresh=tensor, xs_updated=tensor, updated_indices=ids) and recall(n_rows=1000) on the device tensors: the new
           rows and the invalidated graph assembled on the device, the rebuild reading them in place; the exact search and the
           hit count of recall() on the tensors
  host     the same index taken through the host path with the same rows as host arrays (``tensor.cpu()``): the mirrors of the rows
           and the graph fetched, numpy assembly, the rebuild from host rows -- what every update() of a device-built index did
           before the device path existed; recall() through the mirrors (fetched, the rows uploaded again, the graph read on the
           host), as it ran then

Every repetition works on a fresh shallow copy of the one built index (same tensors, no cached mirror), so a host repetition pays
for its mirrors as a caller's first call does.  update() adds 10 000 fresh rows and replaces 1 000.  The clock is the host's, from a
device synchronise to a device synchronise.  Run from the repository root:

    python tools/ab/device_update_timing.py [--legs device,host] [--n N] [--d D] [--reps R] [--fresh F] [--updated U]

One line per leg and call: min / median / max in ms; the device leg also splits into the stream time of its stages (read from
events after the clock has stopped) with the bytes the row assembly moves and the rate that gives, and both legs list the bytes
they copy between host and device, counted from the arrays they move."""
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
    ap.add_argument("--fresh", type=int, default=10_000)
    ap.add_argument("--updated", type=int, default=1_000)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch

    import bench
    from pynndescent_amd import NNDescent

    legs = args.legs.split(",")
    n, d, k, f, u = args.n, args.d, 15, args.fresh, args.updated
    device = torch.device("cuda:0")
    x = bench.sift_like(n + f + u, d, seed=1, device=device, sample_seed=100)
    rows, fresh, updated = x[:n].contiguous(), x[n:n + f].contiguous(), x[n + f:].contiguous()
    ids = np.random.RandomState(7).choice(n, u, replace=False).tolist()
    fresh_host, updated_host = fresh.cpu().numpy(), updated.cpu().numpy()
    torch.cuda.synchronize()
    base = NNDescent(rows, n_neighbors=k, n_trees=8, random_state=1234)
    torch.cuda.synchronize()
    pristine = dict(base.__dict__)  # tensors by reference; neither a mirror nor prepared state

    def line(name, what, values, unit="ms"):
        print("%-10s %-8s %-52s min %10.3f  median %10.3f  max %10.3f %s  (%d reps)"
              % (args.label, name, what, min(values), statistics.median(values), max(values), unit, len(values)), flush=True)

    def copy_of_the_index():
        index = object.__new__(NNDescent)
        index.__dict__.update(pristine)
        return index

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def host_recall(index):  # the mirrors fetched, the tensors let go: recall() as it ran through the host
        index._raw_data, index._neighbor_graph
        index._drop_device_copies()
        return index.recall(n_rows=1000, random_state=0)

    # the device leg's two assembly stages between events on the stream they run on (read after the clock has stopped), with the
    # bytes they move counted from their arguments; the library itself keeps no such record
    from pynndescent_amd import _capi

    staged, esz = {}, {_capi.NND_DTYPE_FLOAT32: 4, _capi.NND_DTYPE_FLOAT16: 2, _capi.NND_DTYPE_BFLOAT16: 2, _capi.NND_DTYPE_FLOAT64: 8}
    real_rows, real_graph = _capi.device_update_rows, _capi.device_update_graph

    def between_events(stream_ptr, fn):
        on = torch.cuda.ExternalStream(stream_ptr) if stream_ptr else torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(on)
        fn()
        e1.record(on)
        return e0, e1

    def rows_stage(device_, stream_ptr, dim, old, fresh_, updated_, pairs, out_ptr, out_dtype):
        staged["rows"] = between_events(stream_ptr, lambda: real_rows(device_, stream_ptr, dim, old, fresh_, updated_, pairs, out_ptr, out_dtype))
        staged["bytes_rows"] = sum(rows_ * dim * (esz[dt] + esz[out_dtype]) for _, dt, rows_ in (old, fresh_)) + pairs[2] * dim * (esz[updated_[1]] + esz[out_dtype])
        staged["bytes_up"] = 8 * pairs[2]

    def graph_stage(device_, stream_ptr, idx_ptr, dist_ptr, n_old, k_, ids_ptr, n_upd, n_new, map_ptr, out_idx_ptr, out_dist_ptr):
        staged["graph"] = between_events(stream_ptr, lambda: real_graph(device_, stream_ptr, idx_ptr, dist_ptr, n_old, k_, ids_ptr, n_upd, n_new,
                                                                        map_ptr, out_idx_ptr, out_dist_ptr))
        staged["bytes_graph"] = 8 * n_old * k_ + 8 * n_new * k_ + n_old

    _capi.device_update_rows, _capi.device_update_graph = rows_stage, graph_stage

    def leg(host):
        index = copy_of_the_index()
        staged.clear()
        if host:
            ms_update, _ = timed(lambda: index.update(xs_fresh=fresh_host, xs_updated=updated_host, updated_indices=ids))
        else:
            ms_update, _ = timed(lambda: index.update(xs_fresh=fresh, xs_updated=updated, updated_indices=ids))
        assert ("_device_data" in index.__dict__) == (not host), "the leg did not take its path"
        for stage in ("rows", "graph"):  # (after the clock and its synchronise: the events are complete)
            if stage in staged:
                staged["ms_" + stage] = staged[stage][0].elapsed_time(staged[stage][1])
        stages = dict(staged) if not host else {}
        probe = copy_of_the_index()
        ms_recall, value = timed((lambda: host_recall(probe)) if host else (lambda: probe.recall(n_rows=1000, random_state=0)))
        assert host or not any(name in probe.__dict__ for name in ("_raw_data", "_neighbor_graph")), "recall() fetched a mirror"
        return ms_update, ms_recall, value, stages, int(index._build_stats["n_iters_run"])

    results = {}
    for name in legs:
        leg(name == "host")  # warm-up
    for _ in range(args.reps):  # alternating, so that drift of the machine lands on both legs alike
        for name in legs:
            results.setdefault(name, []).append(leg(name == "host"))
    m = n + f
    for name in legs:
        runs = results[name]
        line(name, "update() + device synchronise", [r[0] for r in runs])
        line(name, "recall(n_rows=1000) + device synchronise", [r[1] for r in runs])
        print("%-10s %-8s recall %.6f, rebuild iterations %d" % (args.label, name, runs[0][2], runs[0][4]), flush=True)
        if name == "device":
            line(name, "  stream time: new rows (copy, append, scatter)", [r[3]["ms_rows"] for r in runs])
            line(name, "  stream time: invalidated + padded graph", [r[3]["ms_graph"] for r in runs])
            line(name, "  new rows: %d bytes read + written, rate" % runs[0][3]["bytes_rows"],
                 [r[3]["bytes_rows"] / (r[3]["ms_rows"] * 1e-3) / 1e12 for r in runs], unit="TB/s")
            line(name, "  graph: %d bytes read + written, rate" % runs[0][3]["bytes_graph"],
                 [r[3]["bytes_graph"] / (r[3]["ms_graph"] * 1e-3) / 1e12 for r in runs], unit="TB/s")
            up, down = runs[0][3]["bytes_up"], 0
            r_up, r_down = 4 * 1000, 8
        else:  # mirrors down (rows, graph); the new rows and the padded graph up; recall: mirrors down, rows up again, ids up, truth down
            down, up = 4 * n * d + 8 * n * k, 4 * m * d + 8 * m * k
            r_down, r_up = 4 * n * d + 8 * n * k + 8 * 1000 * 10, 4 * n * d + 8 * 1000
        print("%-10s %-8s update(): bytes device -> host %13d   host -> device %13d (besides the build's scalars)   (n %d, d %d, k %d, "
              "fresh %d, updated %d)" % (args.label, name, down, up, n, d, k, f, u), flush=True)
        print("%-10s %-8s recall(): bytes device -> host %13d   host -> device %13d" % (args.label, name, r_down, r_up), flush=True)


if __name__ == "__main__":
    main()
