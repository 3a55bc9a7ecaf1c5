"""The cases of the step-exact descent tests (tests/test_descent_reference_cpu.py, tests/test_gpu_descent_exact.py) and
their ambiguity caps.

Which kernel a parameter range reaches (csrc/join.hip launch_join_xm, csrc/merge.hip nnd_launch_merge):
    k_local_join16              max_candidates <= 16, neighbour-list width ks = 16 / 32 / 48-64        k_merge_q     k <= 16
    k_local_join_w<32> staged   max_candidates 17-32 and k <= 32                                       k_merge       k 17-64
    k_local_join_w<32> unstaged NND_FLAG_TEST_JOIN_UNSTAGED, or k > 32                                 k_merge_wide  k 65-256
    k_local_join_w<64>          max_candidates 33-64
    the five blocked passes     max_candidates 65-128
Metric codes 2-5 select the XM instances; dp >= 128 the wide K blocking (DC = 64 in k_local_join16: three K blocks at d = 130).

Sizing n.  A launch has min(groups, CUs x workgroups-per-CU) workgroups of four waves; a wave walks several vertices with the
candidate ids prefetched two vertices ahead, so the pipeline reaches its steady state only where a wave gets at least three
vertices: n >= 3 x 4 x 256 x (workgroups per CU).  The workgroups per CU are bounded from above by what the launch asks of a CU
with 160 KB of LDS and 512 registers a lane and SIMD -- a bound that is no smaller than what the launcher's occupancy query
returns, so the n below are sufficient whatever that returns:
    k_local_join16, ks = 16:  7584 B of LDS a wave, 30.3 KB a workgroup -> at most 5           n >= 15360
    k_local_join16, ks = 32:  9632 B a wave, 38.5 KB a workgroup -> at most 4                  n >= 12288
    k_local_join16, ks = 48-64 (one instance, rows of 68 words): 13728 B a wave, 54.9 KB a workgroup -> at most 2
                                                                                               n >= 6144
    k_local_join_w<32> staged:   13072 B a wave, 52.3 KB a workgroup -> at most 3              n >= 9216
    k_local_join_w<32> unstaged: 5904 B a wave, 23.6 KB a workgroup -> at most 6               n >= 18432
    k_local_join_w<64> and the blocked passes: 4 x 8 accumulator tiles and two sets of 8 operand tiles are 256 registers a
        lane, which leaves room for two waves a SIMD -> at most 2                              n >= 6144
n is never a multiple of 64 (the last wave of a merge launch and the last workgroup of a join have idle lanes).

Lattice cases: euclidean, integer coordinates in [-60, 60]^16, the point set closed under negation (vstack([h, -h])): the
column mean is exactly 0, the prepared rows are the raw rows, |a|^2, |b|^2 and <a, b> are integers below 16 x 60^2 = 57600 and
every distance an integer below 4 x 57600 < 2^24 whatever the summation order.  Slots, merges and ties are decided on
(dist, id) keys: nothing is ambiguous, the cap is 0 and ids, distance bits, flags, c and the proposal counter must be equal.

Caps: at most 10 % of the rows of a float case may be ambiguous in any checked iteration, none on the lattice.
"""
from collections import namedtuple

import numpy as np

from oracle import oracle as O
from pynndescent_amd import _capi
from tests import metric_util as MU
from tests.util_data import clustered

UNSTAGED = _capi.NND_FLAG_TEST_JOIN_UNSTAGED
FLOAT_CAP, LATTICE_CAP = 0.10, 0.0


def iters(case):
    """The iterations to check: 0 (all new, every row dirty), 1 and 2 (mixed), and a late one with few dirty rows -- the 4th,
    or the 3rd where long rows or long candidate lists have the small sets converged by then (measured on an MI355X: with
    k or max_candidates >= 40 nothing is left to join in iteration 6, and little in iteration 4).

    Rows of 100 and more neighbours: the model walks 10 to 45 million pairs in EVERY iteration of such a case (the old lists
    stay full when nothing is new any more), seconds each.  They check two of the four: the float cases the first and the
    late one, lattice_k100_mc60 the two mixed ones bit for bit -- k_local_join_w<64> + k_merge_wide is checked in all four
    stages between it and k100_mc60, and the mixed stages of the blocked passes and of k_local_join_w<64> by the cases of
    shorter rows (k40_mc100, k50_mc50, k64_mc64 and their lattices), which check all four.  The other iterations still run."""
    if case.k >= 100:
        return (1, 2) if case.exact else (0, 3)
    return (0, 1, 2, 3 if max(case.k, case.mc) >= 40 and not case.exact else 4)


Case = namedtuple("Case", ["name", "metric", "k", "mc", "n", "d", "n_trees", "join_blocks", "flags", "exact", "seed", "doc"])

N16, N16B, N16C, NW32, NW32U, NW64 = 15601, 12301, 6401, 9601, 18451, 6401


def _c(name, metric, k, mc, n, d, doc, n_trees=2, join_blocks=1, flags=0, exact=False, seed=1):
    return Case(name, metric, k, mc, n, d, n_trees, join_blocks, flags, exact, seed, doc)


FLOAT = {c.name: c for c in [
    _c("k10_mc10", "euclidean", 10, 10, N16, 24, "k_local_join16 (ks = 16) + k_merge_q; rows that end before the 16th lane"),
    _c("k15_mc15", "euclidean", 15, 15, N16, 40, "k_local_join16 (ks = 16) + k_merge_q: the benchmark's shape"),
    _c("k16_mc16", "euclidean", 16, 16, N16, 24, "k_local_join16 (ks = 16) + k_merge_q; full candidate tiles, rows of exactly 16"),
    _c("k20_mc12", "euclidean", 20, 12, N16B, 24, "k_local_join16 (ks = 32: two chunks a membership test) + k_merge"),
    _c("k40_mc14", "euclidean", 40, 14, N16C, 24, "k_local_join16 (ks = 48: the instance of list widths 48-64, four chunks a "
       "membership test, a partly filled last chunk) + k_merge"),
    _c("k15_mc15_d130", "euclidean", 15, 15, N16, 130, "k_local_join16, dp = 132: three K blocks of 64 (DC > 1) + k_merge_q"),
    _c("k30_mc30", "euclidean", 30, 30, NW32, 24, "k_local_join_w<32> with the neighbour lists staged in LDS + k_merge"),
    _c("k30_mc30_unstaged", "euclidean", 30, 30, NW32U, 24, "k_local_join_w<32>, lists read from global memory (test flag) + k_merge",
       flags=UNSTAGED),
    _c("k40_mc20", "euclidean", 40, 20, NW32U, 40, "k_local_join_w<32> unstaged (k > 32) + k_merge"),
    _c("k50_mc50", "euclidean", 50, 50, NW64, 24, "k_local_join_w<64> + k_merge"),
    _c("k64_mc64", "euclidean", 64, 64, NW64, 24, "k_local_join_w<64>, every tile full + k_merge with every lane a list entry"),
    _c("k40_mc100", "euclidean", 40, 100, NW64, 24, "the five blocked passes (second blocks partly filled) + k_merge"),
    _c("k100_mc128", "euclidean", 100, 128, NW64, 24, "the five blocked passes, lists of 128 + k_merge_wide"),
    _c("k100_mc60", "euclidean", 100, 60, NW64, 40, "k_local_join_w<64> + k_merge_wide (two entries a lane)"),
    _c("k200_mc60", "euclidean", 200, 60, NW64, 24, "k_local_join_w<64> + k_merge_wide (four entries a lane)"),
    _c("cosine_k15", "cosine", 15, 15, N16, 24, "k_local_join16 on unit rows, -log2 conversion + k_merge_q"),
    _c("cosine_k30", "cosine", 30, 30, NW32, 40, "k_local_join_w<32> staged on unit rows + k_merge"),
    _c("dot_k15", "dot", 15, 15, N16, 24, "k_local_join16, XM instance (code 2; zero rows at FLT_MAX) + k_merge_q"),
    _c("inner_product_k15", "inner_product", 15, 15, N16, 24, "k_local_join16, XM instance (code 3; self pairs at 1 / |x|^2) + k_merge_q"),
    _c("correlation_k15", "correlation", 15, 15, N16, 24, "k_local_join16, XM instance (code 4; constant rows) + k_merge_q"),
    _c("hellinger_k15", "hellinger", 15, 15, N16, 24, "k_local_join16, XM instance (code 5) + k_merge_q"),
    _c("blocks3_k15", "euclidean", 15, 15, N16, 24, "three sub-steps without a forest: k_local_join16 + k_merge_q, thresholds and ids "
       "refreshed between them", n_trees=0, join_blocks=3),
    _c("blocks3_k100_mc60", "euclidean", 100, 60, NW64, 24, "three sub-steps without a forest: k_local_join_w<64> + k_merge_wide",
       n_trees=0, join_blocks=3),
]}

LATTICE = {c.name: c for c in [
    _c("lattice_k15", "euclidean", 15, 15, N16 + 1, 16, "k_local_join16 + k_merge_q, bit for bit", exact=True),
    _c("lattice_k40_mc14", "euclidean", 40, 14, N16C + 1, 16, "k_local_join16 (ks = 48: the instance of list widths 48-64) + k_merge, "
       "bit for bit", exact=True),
    _c("lattice_k30", "euclidean", 30, 30, NW32 + 1, 16, "k_local_join_w<32> staged + k_merge, bit for bit", exact=True),
    _c("lattice_k50", "euclidean", 50, 50, NW64 + 1, 16, "k_local_join_w<64> + k_merge, bit for bit", exact=True),
    _c("lattice_k40_mc100", "euclidean", 40, 100, NW64 + 1, 16, "the five blocked passes + k_merge, bit for bit", exact=True),
    _c("lattice_k100_mc60", "euclidean", 100, 60, NW64 + 1, 16, "k_local_join_w<64> + k_merge_wide, bit for bit", exact=True),
    _c("lattice_blocks3", "euclidean", 15, 15, N16 + 1, 16, "three sub-steps without a forest, bit for bit", exact=True, n_trees=0,
       join_blocks=3),
]}
ALL = dict(FLOAT, **LATTICE)
assert all(c.n % 64 for c in ALL.values())

_DATA = {}


def lattice_points(n, d=16, r=60, seed=7):
    assert n % 2 == 0 and ((d + 3) & ~3) * (2 * r) ** 2 < 2 ** 24
    h = np.random.RandomState(seed).randint(-r, r + 1, size=(n // 2, d))
    x = np.vstack([h, -h]).astype(np.float32)
    assert len(np.unique(x, axis=0)) == n, "duplicate lattice points"
    return np.ascontiguousarray(x)


def data(case):
    if case.name not in _DATA:
        if case.exact:
            x = lattice_points(case.n, case.d)
        elif case.metric == "hellinger":
            # non-negative rows that are NOT nearly parallel: shifted to positive (metric_util.metric_data) every <sqrt a, sqrt b>
            # is ~0.99 of the norms and -log2 of it cancels -- the a-priori radius of the Gram form then overlaps for 80 % of the
            # rows.  Clipped at 0 the rows keep their spread (and some rows are all zero: the FLT_MAX convention)
            x = np.maximum(clustered(case.n, case.d, 6, 30, seed=case.n % 89), np.float32(0.0))
            x[[7, 500, 1500]] = 0.0
        elif case.metric in MU.NEW_METRICS:
            x = MU.metric_data(case.metric, case.n, case.d, seed=11)[0]
            if case.metric == "dot":  # the class hands the build normalised rows
                nrm = np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
                x = np.where(nrm > 0, x / np.where(nrm > 0, nrm, 1.0), 0.0).astype(np.float32)
        else:
            x = clustered(case.n, case.d, 6, 30, seed=case.n % 89)
        x.setflags(write=False)
        _DATA[case.name] = x
    return _DATA[case.name]


def rng_state(case):
    return O.draw_rng_states(case.seed, max(case.n_trees, 1))[0]


def sort_rows(idx, dist, flags):
    """heap-ordered rows -> ascending by (dist, id), unfilled entries last."""
    key = np.where(idx >= 0, dist.astype(np.float64), np.inf)
    # (dist, id): a stable sort by distance of rows first ordered by id
    by_id = np.argsort(np.where(idx >= 0, idx, np.iinfo(np.int32).max), axis=1, kind="stable")
    idx, dist, flags, key = (np.take_along_axis(a, by_id, 1) for a in (idx, dist, flags, key))
    o = np.argsort(key, axis=1, kind="stable")
    idx, dist, flags = (np.take_along_axis(a, o, 1) for a in (idx, dist, flags))
    return idx, np.where(idx >= 0, dist, np.inf).astype(np.float32), np.where(idx >= 0, flags, 0).astype(np.uint8)


def front_filled(lists):
    """the reference's candidate lists are heaps with holes: the same ids, packed to the front (the kernels' convention)."""
    o = np.argsort(lists < 0, axis=1, kind="stable")
    return np.take_along_axis(lists, o, 1)


def cpu_state(case, x=None):
    """A state for the model without a GPU, from the reference algorithm: init_rp_tree + init_random for the rows and
    new_build_candidates for the lists (its distribution of candidates on the same data; ``x``: rows other than the case's).
    Returns (idx0, dist0, fl0, new, old)."""
    lib = O.load("strict")
    x = np.ascontiguousarray(data(case) if x is None else x)
    n, k = x.shape[0], case.k
    st, _, tree_states = O.draw_rng_states(case.seed, max(case.n_trees, 1))
    la = O.make_leaf_array(x, case.n_trees, O.default_leaf_size(k), tree_states, case.metric in ("cosine", "dot", "hellinger"), lib=lib)
    hi, hd, hf = O.init_rp_tree(x, k, case.metric, la, lib=lib)
    lib.orc_init_random(x, n, x.shape[1], O.METRICS[case.metric], hi, hd, hf, k, st.copy())
    idx0, dist0, fl0 = sort_rows(hi, hd, hf)
    new, old = candidates_cpu(case, idx0, fl0)
    return idx0, dist0, fl0, new, old


def candidates_cpu(case, idx0, fl0):
    lib = O.load("strict")
    n, k = idx0.shape
    new = np.empty((n, case.mc), np.int32)
    old = np.empty((n, case.mc), np.int32)
    lib.orc_new_build_candidates(np.ascontiguousarray(idx0).copy(), np.ascontiguousarray(fl0).copy(), n, k, case.mc,
                                 np.array([11, 22, 33], np.int64), 8, new, old)
    return front_filled(new), front_filled(old)
