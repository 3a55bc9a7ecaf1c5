"""What a boolean-metric build costs at 1 M x 128 on the device (k = 15), against the cosine build of the same float rows: one
process, the legs alternating, one warm-up of each, then REPS timed builds per leg; medians.

  jaccard  NNDescent(rows, metric="jaccard")   indicator rows, -log2(c / (c + ne)) in the epilogues
  dice     NNDescent(rows, metric="dice")      indicator rows, ne / (2c + ne)
  cosine   NNDescent(rows, metric="cosine")    the same float rows (0 / 1 values): the yardstick for what the epilogue costs

The rows are clustered binary rows made on the device: 256 prototypes of density 0.05 .. 0.3, every member a prototype with each bit
flipped with probability 0.02.  The clock is the host's, from a device synchronise to a device synchronise.  Per leg: build
time, the iterations the stop rule allowed, the builder's stage times (its counters: prep / forest / leaf seeding / descent with
sample, join, merge / finalize), and recall@10 on 1000 sampled rows via index.recall() (the truth: the exact search of the
same metric under (distance, id); with this many equal distances the count by id is a lower bound of the count by distance).
Run from the repository root:

    python tools/ab/boolean_metrics_timing.py [--n N] [--d D] [--reps R] [--legs jaccard,dice,cosine]
"""
import argparse
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="jaccard,dice,cosine")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    import torch

    from pynndescent_amd import NNDescent

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    dens = torch.rand(256, 1, generator=g, device=dev) * 0.25 + 0.05
    proto = torch.rand(256, args.d, generator=g, device=dev) < dens
    lab = torch.randint(0, 256, (args.n,), generator=g, device=dev)
    rows = (proto[lab] ^ (torch.rand(args.n, args.d, generator=g, device=dev) < 0.02)).float().contiguous()
    torch.cuda.synchronize()
    legs = args.legs.split(",")
    times = {leg: [] for leg in legs}
    last = {}
    for rep in range(args.reps + 1):  # repetition 0 warms every leg up
        for leg in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            index = NNDescent(rows, metric=leg, n_neighbors=15, n_trees=8, random_state=1234)
            torch.cuda.synchronize()
            if rep:
                times[leg].append(1e3 * (time.perf_counter() - t0))
            last[leg] = index
    print("n = %d, d = %d, k = 15, %d timed builds per leg (medians)" % (args.n, args.d, args.reps))
    for leg in legs:
        st = last[leg]._build_stats
        st = st if isinstance(st, dict) else st.as_dict()
        rec = last[leg].recall(k=10, n_rows=1000, random_state=7)
        print("%-8s build %9.2f ms (min %9.2f max %9.2f)  iterations %2d  recall@10 %.4f" % (
            leg, statistics.median(times[leg]), min(times[leg]), max(times[leg]), st["n_iters_run"], rec))
        print("         stages ms: prep %.2f forest %.2f leaf %.2f random %.2f descent %.2f (sample %.2f join %.2f merge %.2f) finalize %.2f; "
              "updates per iteration %s" % (st["ms_prep"], st["ms_forest"], st["ms_leaf_init"], st["ms_random_init"], st["ms_descent"],
                                            sum(st["ms_sample"]), sum(st["ms_join"]), sum(st["ms_merge"]), st["ms_finalize"], st["updates"]))
    if "cosine" in legs:
        for leg in legs:
            if leg != "cosine":
                print("%s / cosine: %.2f x" % (leg, statistics.median(times[leg]) / statistics.median(times["cosine"])))


if __name__ == "__main__":
    main()
