"""What sparse input costs (csrc/sparse.hip, pynndescent_amd/sparse_input.py): one process, the legs alternating, warm-up of each,
then REPS timed repetitions, min / median / max of each.

  (a) the kernel alone, k_csr_rows in stream time between two events, at 1 M x 512 density 0.05, 1 M x 128 density 0.2 and
      100 k x 20 000 density 0.002 (--sizes), with its achieved bytes/s against its byte floor -- 4 n d written plus
      8 nnz + 4 (n + 1) read (int32 indices and indptr, float32 values) -- and a hipMemsetAsync of the same buffer in the same
      run, alternating with it: the practical ceiling of writing that many bytes.
  (b) the class call NNDescent(csr, metric="cosine") against NNDescent(csr.toarray()) from host memory, at the first two sizes
      (--class-sizes): the dense call is what the index could do before, the baseline.  Host clock, from a device synchronise to a
      device synchronise.  The two graphs are compared once (they must be equal).

The matrices are drawn on the device (uniform pattern, values in [0.5, 1.5)) and brought to the host for (b).  Run from the
repository root; the log goes to --out as well as to the terminal:

    python tools/ab/sparse_input_timing.py [--reps R] [--out profiles/sparse_input.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

SIZES = "1000000x512x0.05,1000000x128x0.2,100000x20000x0.002"


def parse_sizes(text):
    return [(int(n), int(d), float(p)) for n, d, p in (item.split("x") for item in text.split(",") if item)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--sizes", default=SIZES)
    ap.add_argument("--class-sizes", default=",".join(SIZES.split(",")[:2]))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "sparse_input.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import scipy.sparse as sp
    import torch

    from pynndescent_amd import NNDescent, _capi

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    device = torch.device("cuda:0")
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    log = open(args.out, "w")

    def say(text=""):
        print(text, flush=True)
        log.write(text + "\n")
        log.flush()

    def line(name, what, values, unit="ms", extra=""):
        say("%-10s %-46s min %10.3f  median %10.3f  max %10.3f %s  (%d reps)%s"
            % (name, what, min(values), statistics.median(values), max(values), unit, len(values), extra))

    def draw(n, d, density, seed):
        """(indptr int32 (n + 1), indices int32, values float32) on the device: canonical by construction."""
        gen = torch.Generator(device=device).manual_seed(seed)
        step = max(1, (1 << 26) // d)
        counts, cols = [], []
        for lo in range(0, n, step):
            mask = torch.rand((min(step, n - lo), d), generator=gen, device=device) < density
            counts.append(mask.sum(1, dtype=torch.int64))
            cols.append(mask.nonzero()[:, 1].to(torch.int32))
        indptr = torch.zeros((n + 1,), dtype=torch.int64, device=device)
        indptr[1:] = torch.cumsum(torch.cat(counts), 0)
        indices = torch.cat(cols)
        assert int(indptr[-1].item()) == indices.numel() < 2 ** 31
        values = torch.rand((indices.numel(),), generator=gen, device=device) + 0.5
        return indptr.to(torch.int32), indices, values

    def stream_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    say("sparse input: %s, torch %s, %d repetitions per leg, legs alternating" % (torch.cuda.get_device_name(0), torch.__version__, args.reps))
    say()
    say("(a) k_csr_rows alone, stream time; floor = 4 n d written + 8 nnz + 4 (n + 1) read")
    drawn = {}
    for n, d, density in parse_sizes(args.sizes):
        indptr, indices, values = drawn[(n, d, density)] = draw(n, d, density, seed=n % 1000 + d)
        nnz = indices.numel()
        dst = torch.empty((n, d), dtype=torch.float32, device=device)
        stream = torch.cuda.current_stream(0).cuda_stream

        def kernel():
            _capi.device_csr_rows(0, stream, indptr.data_ptr(), 4, indices.data_ptr(), 4, values.data_ptr(), n, d, dst.data_ptr())

        def memset():
            assert hip.hipMemsetAsync(dst.data_ptr(), 0, dst.numel() * 4, stream) == 0

        for _ in range(2):
            kernel()
            memset()
        torch.cuda.synchronize()
        t_kernel, t_memset = [], []
        for rep in range(args.reps):
            for leg in ((kernel, memset) if rep % 2 == 0 else (memset, kernel)):
                (t_kernel if leg is kernel else t_memset).append(stream_ms(leg))
        kernel()  # (the last leg may have been the memset) the result, checked against torch's own scatter on a sample of rows
        rows = torch.arange(0, n, max(1, n // 2000), device=device)
        want = torch.zeros((rows.numel(), d), dtype=torch.float32, device=device)
        for i, r in enumerate(rows.tolist()):
            s, e = int(indptr[r].item()), int(indptr[r + 1].item())
            want[i, indices[s:e].long()] = values[s:e]
        assert torch.equal(dst[rows], want), "k_csr_rows disagrees with a scatter of the same rows"
        floor = 4 * n * d + 8 * nnz + 4 * (n + 1)
        med = statistics.median(t_kernel)
        say("%d x %d, density %g: nnz %d, dense %.3f GB, floor %.3f GB" % (n, d, density, nnz, 4e-9 * n * d, 1e-9 * floor))
        line("kernel", "k_csr_rows", t_kernel, extra="  %.2f TB/s of its floor at the median" % (floor / med * 1e-9))
        line("memset", "hipMemsetAsync of the same buffer", t_memset,
             extra="  %.2f TB/s written; kernel / memset = %.2f" % (4 * n * d / statistics.median(t_memset) * 1e-9, med / statistics.median(t_memset)))
        del dst, want
    say()
    say('(b) the class call, host clock: NNDescent(csr, metric="cosine") against NNDescent(csr.toarray()), n_neighbors = 15')

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for n, d, density in parse_sizes(args.class_sizes):
        indptr, indices, values = drawn.pop((n, d, density), None) or draw(n, d, density, seed=n % 1000 + d)
        csr = sp.csr_matrix((values.cpu().numpy(), indices.cpu().numpy(), indptr.cpu().numpy()), shape=(n, d))
        del indptr, indices, values
        drawn.clear()
        torch.cuda.empty_cache()
        dense = csr.toarray()
        legs = {"sparse": lambda: NNDescent(csr, metric="cosine", n_neighbors=15, random_state=1),
                "dense": lambda: NNDescent(dense, metric="cosine", n_neighbors=15, random_state=1)}
        graphs = {name: fn()._neighbor_graph for name, fn in legs.items()}  # the warm-up of each, and the comparison
        same = all(np.array_equal(a, b) for a, b in zip(graphs["sparse"], graphs["dense"]))
        del graphs
        times = {name: [] for name in legs}
        for rep in range(args.reps):
            for name in (("sparse", "dense") if rep % 2 == 0 else ("dense", "sparse")):
                ms, index = timed(legs[name])
                times[name].append(ms)
                del index
        say("%d x %d, density %g: CSR arrays %.3f GB, dense rows %.3f GB; graphs equal: %s"
            % (n, d, density, 1e-9 * (csr.data.nbytes + csr.indices.nbytes + csr.indptr.nbytes), 1e-9 * dense.nbytes, "yes" if same else "NO"))
        line("sparse", "NNDescent(csr)", times["sparse"])
        line("dense", "NNDescent(csr.toarray()), the baseline", times["dense"],
             extra="  sparse / dense = %.3f at the medians" % (statistics.median(times["sparse"]) / statistics.median(times["dense"])))
        del csr, dense
    log.close()


if __name__ == "__main__":
    main()
