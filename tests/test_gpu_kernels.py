"""Kernel-level parity tests on a real MI355X (each stage of the build through the C ABI)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.gpu_util import alt_dist_matrix, check_graph_invariants, make_builder
from tests.util_data import clustered, nn_data_like

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("d", [5, 40, 128, 200])
def test_mfma_gram_tile(metric, d):
    """The f32 MFMA Gram tile (operand and result lane maps) against float64 numpy, asymmetric row lists."""
    rs = np.random.RandomState(d)
    x = (rs.standard_normal((300, d)) * rs.uniform(0.5, 2.0, (1, d)) + 0.7).astype(np.float32)
    x[17] = 0.0
    b = make_builder(x, metric, k=10, n_trees=0)
    rows_a = rs.permutation(300)[:37]
    rows_b = np.concatenate([rs.permutation(300)[:51], [17, 17]])
    got = b.pairwise_gram(rows_a, rows_b)
    want = alt_dist_matrix(x, rows_a, rows_b, metric)
    fin = want < 1e30
    assert np.array_equal(got > 1e30, ~fin)
    scale = np.abs(want[fin]).max()
    np.testing.assert_allclose(got[fin], want[fin], rtol=2e-4, atol=2e-6 * scale)
    b.close()


@pytest.mark.parametrize("metric,n,d,k,T", [("euclidean", 5000, 24, 15, 4), ("cosine", 3000, 16, 10, 3),
                                            ("euclidean", 1002, 5, 30, 6)])
def test_forest_partitions(metric, n, d, k, T):
    x = clustered(n, d, 6, 30, seed=n) if d > 5 else nn_data_like()
    b = make_builder(x, metric, k=k, n_trees=T)
    b.make_forest()
    la = b.leaf_array()
    ls = O.default_leaf_size(k)
    assert la.shape[1] == ls
    ids = la[la >= 0]
    assert ids.shape[0] == T * n
    assert np.all(np.bincount(ids, minlength=n) == T)  # every tree holds every point exactly once
    lens = (la >= 0).sum(1)
    assert lens.max() <= ls and lens.min() >= 1
    # -1 padding only at the row tails
    assert np.all((la >= 0) == (np.arange(ls)[None, :] < lens[:, None]))
    # same leaf statistics as the reference algorithm (oracle): mean fill within 15 %
    _, _, ts = O.draw_rng_states(1, T)
    ola = O.make_leaf_array(x, T, ls, ts, O.ANGULAR[metric])
    ofill = (ola >= 0).sum(1).mean()
    assert abs(lens.mean() - ofill) <= 0.15 * ofill, (lens.mean(), ofill)
    # and the same locality: fraction of true 5-NN that share a leaf with their point
    ti, _ = O.brute_force_knn(x, 6, metric)

    def colocated(arr):
        hit = np.zeros(n)
        leaf_of = {}
        for row in arr:
            members = row[row >= 0]
            s = set(members.tolist())
            for p in members:
                hit[p] += sum(1 for q in ti[p, 1:] if q in s)
        return hit.sum() / (n * 5 * T)

    cg, co = colocated(la), colocated(ola)
    assert abs(cg - co) <= 0.04, (cg, co)
    b.close()


@pytest.mark.parametrize("metric,n,d,k,T", [("euclidean", 4000, 32, 15, 3), ("cosine", 2500, 20, 10, 2),
                                            ("euclidean", 1002, 5, 30, 2), ("euclidean", 1500, 130, 12, 2),
                                            # round 6: the sorting-network merges at their edges -- k = 16 (every lane of a 16-lane row
                                            # holds an entry), k = 17 / 20 / 32 (k_leaf_join_sym: both size classes, all 32 lanes), k = 8
                                            ("euclidean", 5000, 40, 16, 3), ("euclidean", 3000, 16, 17, 2), ("cosine", 3000, 24, 20, 2),
                                            ("euclidean", 6000, 32, 30, 3), ("euclidean", 4000, 24, 32, 2), ("cosine", 2000, 12, 8, 3)])
def test_leaf_init_is_exact_topk_of_leafmates(metric, n, d, k, T):
    """After init_from_leaves every row must hold exactly the k nearest of the point's leaf-mates
    (what sequential checked_flagged_heap_push over all leaf pairs produces, pynndescent_.py:73-185)."""
    x = clustered(n, d, 6, 25, seed=7) if d > 5 else nn_data_like()
    b = make_builder(x, metric, k=k, n_trees=T)
    b.make_forest()
    la = b.leaf_array()
    b.init_from_leaves()
    idx, dist, flags = b.graph()
    check_graph_invariants(x, metric, idx, dist, name="leaf_init")
    assert np.all(flags[idx >= 0] == 1)
    mates = [set() for _ in range(n)]
    for row in la:
        m = row[row >= 0]
        for p in m:
            mates[p].update(m.tolist())
    bad = 0
    for p in range(0, n, 7):
        cand = np.array(sorted(mates[p] - {p}))
        dd = alt_dist_matrix(x, [p], cand, metric)[0]
        kk = min(k, len(cand))
        kth = np.sort(dd)[kk - 1]
        got = idx[p][idx[p] >= 0]
        assert len(got) == kk, (p, len(got), kk)
        gd = alt_dist_matrix(x, [p], got, metric)[0]
        if not np.all(gd <= kth * (1 + 1e-4) + 1e-6):
            bad += 1
    assert bad == 0
    b.close()


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_random_init(metric):
    x = clustered(2000, 16, 5, 10, seed=5)
    b = make_builder(x, metric, k=12, n_trees=0)
    b.init_random()
    idx, dist, flags = b.graph()
    check_graph_invariants(x, metric, idx, dist, name="random_init")
    filled = (idx >= 0).sum(1)
    assert filled.min() >= 9 and filled.mean() > 11.8  # k draws, collisions are rare at n=2000
    assert np.all(flags[idx >= 0] == 1)
    b.close()


def test_init_from_graph():
    x = clustered(1500, 12, 4, 8, seed=9)
    ti, td = O.brute_force_knn(x, 8, "euclidean")
    g = ti.copy()
    g[:, 3] = g[:, 2]  # duplicate entries must be pushed once (utils.py:489-492)
    g[::5, 5] = -1
    b = make_builder(x, "euclidean", k=10, n_trees=0)
    b.init_from_graph(g)
    idx, dist, flags = b.graph()
    check_graph_invariants(x, "euclidean", idx, dist, name="init_graph")
    for r in range(0, 1500, 11):
        want = set(g[r][g[r] >= 0].tolist())
        assert set(idx[r][idx[r] >= 0].tolist()) == want
    b.close()


@pytest.mark.parametrize("k,mc", [(15, 15), (30, 30), (10, 6), (60, 60), (20, 40)])
def test_sample_candidates(k, mc):
    """Structural contract of new_build_candidates (utils.py:221-320)."""
    x = clustered(3000, 16, 5, 20, seed=11)
    b = make_builder(x, "euclidean", k=k, n_trees=3, mc=mc)
    b.make_forest()
    b.init_from_leaves()
    b.init_random()
    b.descent_iter()  # creates a mix of old and new entries
    idx0, _, fl0 = b.graph()
    b.sample_candidates()
    new, old = b.candidates()
    idx1, _, fl1 = b.graph()
    assert np.array_equal(idx0, idx1)
    n = x.shape[0]
    fwd = [dict() for _ in range(n)]
    rev_new = [set() for _ in range(n)]
    rev_old = [set() for _ in range(n)]
    for v in range(n):
        for j in range(k):
            u = idx0[v, j]
            if u >= 0:
                (rev_new if fl0[v, j] else rev_old)[u].add(v)
    n_new_total = 0
    for v in range(n):
        nv = new[v][new[v] >= 0]
        ov = old[v][old[v] >= 0]
        assert len(nv) == len(np.unique(nv)) and len(ov) == len(np.unique(ov))
        f_new = set(idx0[v][(idx0[v] >= 0) & (fl0[v] == 1)].tolist())
        f_old = set(idx0[v][(idx0[v] >= 0) & (fl0[v] == 0)].tolist())
        assert set(nv.tolist()) <= (f_new | rev_new[v]), v
        assert set(ov.tolist()) <= (f_old | rev_old[v]), v
        assert len(nv) >= min(mc, len(f_new)) and len(ov) >= min(mc, len(f_old))
        # lists are filled from the front
        assert np.all(new[v][: len(nv)] >= 0) and np.all(old[v][: len(ov)] >= 0)
        # flag reset: forward new entries that were sampled are old now, the others stay new (utils.py:311-318)
        for j in range(k):
            u = idx0[v, j]
            if u >= 0 and fl0[v, j] == 1:
                assert fl1[v, j] == (0 if u in set(nv.tolist()) else 1)
            elif u >= 0:
                assert fl1[v, j] == 0
        n_new_total += len(nv)
    assert n_new_total > 0
    b.close()


def _mix32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15); x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def _hash2(seed, a):
    return _mix32(np.uint32(seed) ^ _mix32(np.asarray(a, np.uint32) + np.uint32(0x9E3779B9)))


def _hash3(seed, a, b):
    return _mix32(_hash2(seed, a) ^ _mix32(np.asarray(b, np.uint32) * np.uint32(0x85EBCA6B) + np.uint32(0xC2B2AE35)))


def _expected_candidates(idx, fl, rng_state, it, mc, cap_new, cap_old):
    """Host model of new_build_candidates (utils.py:221-320) with the library's counter hashes as priorities
    (csrc/sample.hip): per (vertex, class) the max_candidates smallest (priority, id) keys of its forward edges and of
    the reverse offers it receives (a reverse offer that repeats a forward id of the list is not pushed, utils.py:427-430).
    Returns (new, old, exact_new, exact_old): exact_* is False where a bank received more offers than it has slots."""
    n, k = idx.shape
    r = [np.uint32(int(v) & 0xFFFFFFFF) for v in rng_state]
    with np.errstate(over="ignore"):
        seed = _mix32(r[0] ^ _mix32(r[1] + np.uint32(0x9E3779B9)) ^ _mix32(r[2] + np.uint32(0x7F4A7C15)))[()]
        it_seed = _hash2(seed ^ np.uint32(0x9E3779B9), np.uint32(it + 1))[()]
        vv, jj = np.nonzero(idx >= 0)
        uu = idx[vv, jj].astype(np.int64)
        cc = fl[vv, jj].astype(np.int64)
        fkey = (_hash3(it_seed, vv, uu).astype(np.uint64) << np.uint64(32)) | uu.astype(np.uint64)
        salt = _hash2(it_seed ^ np.uint32(0x3C6EF372), uu)
        rkey = (_mix32(vv.astype(np.uint32) ^ salt).astype(np.uint64) << np.uint64(32)) | vv.astype(np.uint64)
    # offers a bank receives (before the duplicate screen): what decides whether the bank is exact
    recv = np.zeros((n, 2), np.int64)
    np.add.at(recv, (uu, cc), 1)
    # a reverse offer v -> u (class c) is dropped when u's own list of class c holds the forward edge u -> v
    fwd_code = (vv.astype(np.int64) * n + uu) * 2 + cc
    rev_code = (uu * n + vv.astype(np.int64)) * 2 + cc
    keep = ~np.isin(rev_code, fwd_code)
    owner = np.concatenate([vv.astype(np.int64), uu[keep]])
    cls = np.concatenate([cc, cc[keep]])
    key = np.concatenate([fkey, rkey[keep]])
    order = np.lexsort((key, cls, owner))
    owner, cls, key = owner[order], cls[order], key[order]
    grp = owner * 2 + cls
    first = np.r_[True, grp[1:] != grp[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(len(grp)), 0))
    rank = np.arange(len(grp)) - start
    out = np.full((n, 2, mc), -1, np.int32)
    sel = rank < mc
    out[owner[sel], cls[sel], rank[sel]] = (key[sel] & np.uint64(0xFFFFFFFF)).astype(np.int32)
    return out[:, 1], out[:, 0], recv[:, 1] <= cap_new, recv[:, 0] <= cap_old


@pytest.mark.parametrize("n,k,mc", [(20000, 15, 15), (70000, 15, 15), (20000, 30, 30), (9000, 60, 60), (9000, 20, 40), (6000, 100, 50), (5000, 200, 60)])
def test_sampled_candidates_are_the_exact_priority_sample(n, k, mc):
    """The bucketed reverse pass (round 5) keeps EVERY reverse offer of a bank that receives no more offers than it has
    slots, as the reference's heaps do (utils.py:277-306): the candidate lists must equal, entry for entry, the
    max_candidates smallest (priority, id) keys of forward edges + reverse offers computed on the host with the same
    hashes -- on the first pass of a build (all edges new: the new class owns both banks), after one iteration (a mix),
    and after two (mostly old edges, many inactive vertices)."""
    x = clustered(n, 24, 6, 40, seed=n % 89)
    rng_state, _, _ = O.draw_rng_states(1, 3)
    b = make_builder(x, "euclidean", k=k, n_trees=3, mc=mc, seed=1)
    b.make_forest()
    b.init_from_leaves()
    b.init_random()
    rcap = 32 if mc <= 32 else 64
    checked = 0
    for it in range(3):
        idx0, _, fl0 = b.graph()
        b.sample_candidates()
        new, old = b.candidates()
        wide = it == 0 and rcap == 32 and k <= 64
        e_new, e_old, x_new, x_old = _expected_candidates(idx0, fl0, rng_state, it, mc, 2 * rcap if wide else rcap, rcap)
        act = new[:, 0] >= 0
        assert np.array_equal(act, e_new[:, 0] >= 0)
        rows = np.nonzero(x_new)[0]
        np.testing.assert_array_equal(new[rows], e_new[rows])
        rows = np.nonzero(x_old & act)[0]  # the old list of a vertex without new candidates is not defined (never read)
        np.testing.assert_array_equal(old[rows], e_old[rows])
        # how many banks are exact depends on the in-degrees (mean = k) against the slots per bank: nearly all at k = 15
        # with 32 slots; at k >= 30 a good part overflows into the hashed-minimum form (order independent, not compared)
        # (k = 200 against 64 slots: hardly any new-class bank is exact; the old-class banks of the first passes are)
        floor = 0.0 if k > 128 else 0.1
        assert x_new.mean() > (0.97 if k <= 15 else floor) and x_old.mean() > (0.9 if k <= 15 else floor), (x_new.mean(), x_old.mean())
        checked += int(x_new.sum()) + (int((x_old & act).sum()) if k > 128 else 0)
        b.descent_iter()  # (samples again from the state the call above left, joins, merges: the next state to test)
    assert checked > n
    b.close()


def test_sampling_with_hubs_uses_the_overflow_list_and_stays_exact_and_reproducible():
    """An init graph in which EVERY row points at 15 of the same 30 vertices (no forest: positions = ids, the hubs share bucket 0):
    each hub receives ~20 000 reverse offers, so (a) its banks overflow -- hashed minima over ALL of its offers, order independent --
    and (b) the 8 sub-regions of bucket 0 (1 024 records each) overflow and 98 % of its records travel on the overflow list
    (csrc/sample.hip k_rev_place / rv_each_record).  Every bank that did NOT overflow must still be the exact priority sample, the
    hubs' lists must hold max_candidates distinct sources that really offered, and a second run must give the same lists (the
    placement order of the records is not reproducible; the result has to be)."""
    n, k, mc = 40_000, 15, 15
    rs = np.random.RandomState(5)
    x = clustered(n, 24, 6, 40, seed=17)
    g = np.stack([rs.choice(30, k, replace=False) for _ in range(n)]).astype(np.int32)
    rng_state, _, _ = O.draw_rng_states(1, 1)
    runs = []
    for rep in range(2):
        b = make_builder(x, "euclidean", k=k, n_trees=0, mc=mc, seed=1)
        b.init_from_graph(g)
        idx0, _, fl0 = b.graph()
        b.sample_candidates()
        new, old = b.candidates()
        runs.append((new.copy(), old.copy()))
        if rep == 0:
            indeg = np.bincount(idx0[idx0 >= 0].ravel(), minlength=n)
            assert indeg[:30].min() > 8 * 1024  # more offers for ONE vertex than all sub-regions of its bucket hold
            e_new, e_old, x_new, x_old = _expected_candidates(idx0, fl0, rng_state, 0, mc, 64, 32)
            assert (~x_new[:30]).all() and x_new[30:].all()
            np.testing.assert_array_equal(new[30:], e_new[30:])
            src_of = [set(np.nonzero((idx0 == h).any(1))[0].tolist()) for h in range(30)]
            for h in range(30):
                row = new[h]
                assert (row >= 0).all() and len(set(row.tolist())) == mc
                fwd = set(idx0[h].tolist())
                assert all((int(v) in src_of[h]) or (int(v) in fwd) for v in row)
        b.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])


@pytest.mark.parametrize("k,mc", [(15, 15), (30, 30), (40, 50), (70, 65), (40, 100), (100, 128)])
def test_join_evaluates_every_candidate_pair_once(k, mc):
    """The pair set of the local join (pynndescent_.py:228-258): every new candidate against the new candidates from itself on
    (the kernels count the self pair) and against every old candidate.  The join's pair counter must equal that number computed
    from the candidate lists -- in particular for max_candidates > 64, where five passes of the 64-slot kernel walk blocks of
    the lists (join.hip launch_join_blocked): no block pair left out, none taken twice."""
    x = clustered(5000, 24, 6, 30, seed=31)
    b = make_builder(x, "euclidean", k=k, n_trees=2, mc=mc)
    b.make_forest()
    b.init_from_leaves()
    b.init_random()
    b.descent_iter()  # a mix of new and old entries
    b.descent_sample()
    new, old = b.candidates()
    b.descent_join()
    st = b.stats(raw=True)
    nn, no = (new >= 0).sum(1).astype(np.int64), (old >= 0).sum(1).astype(np.int64)
    expect = int((nn * (nn + 1) // 2 + nn * no)[nn > 0].sum())
    got = int(st.join_pairs[int(st.n_iters_run)])
    print("k=%d mc=%d: %d pairs, longest lists %d new / %d old" % (k, mc, got, nn.max(), no.max()))
    assert got == expect, (got, expect)
    if mc > 64:
        assert max(nn.max(), no.max()) > 64  # the second blocks are in use
    b.close()


@pytest.mark.parametrize("metric,k", [("euclidean", 15), ("cosine", 15), ("euclidean", 30), ("euclidean", 50)])
def test_descent_iterations_keep_invariants_and_improve(metric, k):
    x = clustered(4000, 24, 6, 30, seed=13)
    b = make_builder(x, metric, k=k, n_trees=2)
    b.make_forest()
    b.init_from_leaves()
    b.init_random()
    ti, _ = O.brute_force_knn(x, 10, metric)
    idx, dist, _ = b.graph()
    r_prev = O.recall(ti, idx)
    cs = []
    for it in range(4):
        c = b.descent_iter()
        cs.append(c)
        idx, dist, _ = b.graph()
        check_graph_invariants(x, metric, idx, dist, name="iter%d" % it)
        r = O.recall(ti, idx)
        assert r >= r_prev - 1e-9, (it, r_prev, r)
        r_prev = r
    st = b.stats()
    assert cs[0] > 0 and st["join_pairs"][0] > 0 and st["updates"][0] == cs[0]
    assert r_prev > 0.97, r_prev
    # every point is its own nearest neighbour at distance 0 (self pair, utils.py:619)
    assert np.mean(idx[:, 0] == np.arange(x.shape[0])) > 0.999
    fidx, fdist = b.finalize()
    assert np.mean(fidx[:, 0] == np.arange(x.shape[0])) > 0.999 and np.all(fdist[fidx[:, 0] == np.arange(x.shape[0]), 0] == 0)
    b.close()


@pytest.mark.parametrize("metric,n,d,k,T", [("euclidean", 200_000, 32, 15, 4), ("cosine", 150_000, 48, 10, 3)])
def test_forest_routing_pass(metric, n, d, k, T):
    """n >= 131072: the top of the trees is built from a sample and every point is ROUTED to its cell (rpforest.hip
    k_route) instead of taking part in level-synchronous passes.  Same contract as the whole-set build: every tree
    holds every point exactly once, leaves <= leaf_size, reference-like leaf statistics, bit-reproducible."""
    x = clustered(n, d, 8, 200, seed=n % 1000)
    b = make_builder(x, metric, k=k, n_trees=T)
    b.make_forest()
    st = b.stats()
    assert st["n_cells"] > 0, "routing pass did not run"
    la = b.leaf_array()
    ls = O.default_leaf_size(k)
    assert la.shape[1] == ls
    ids = la[la >= 0]
    assert ids.shape[0] == T * n
    assert np.all(np.bincount(ids, minlength=n) == T)
    lens = (la >= 0).sum(1)
    assert lens.max() <= ls and lens.min() >= 1
    assert np.all((la >= 0) == (np.arange(ls)[None, :] < lens[:, None]))
    # leaves are written in ascending id order (canonical: independent of the order in which points reached their cell)
    for row, m in zip(la[::97], lens[::97]):
        assert np.all(np.diff(row[:m]) > 0)
    _, _, ts = O.draw_rng_states(1, T)
    ola = O.make_leaf_array(x, T, ls, ts, O.ANGULAR[metric])
    ofill = (ola >= 0).sum(1).mean()
    assert abs(lens.mean() - ofill) <= 0.15 * ofill, (lens.mean(), ofill)
    # locality: fraction of true 5-NN of a sample of points that share a leaf with their point, vs the oracle's forest
    rows = np.random.RandomState(3).choice(n, 2000, replace=False)
    ti, _ = O.brute_force_knn(x, 6, metric, rows=rows)

    def colocated(arr):
        want = {int(p): set(ti[j, 1:].tolist()) for j, p in enumerate(rows)}
        hit = 0
        for row in arr:
            members = row[row >= 0]
            s = None
            for p in members:
                w = want.get(int(p))
                if w is not None:
                    if s is None:
                        s = set(members.tolist())
                    hit += len(w & s)
        return hit / (len(rows) * 5 * T)

    cg, co = colocated(la), colocated(ola)
    print("routing forest: leaves %d (oracle %d) mean fill %.1f (oracle %.1f) colocation %.4f (oracle %.4f) cells %d levels %d"
          % (la.shape[0], ola.shape[0], lens.mean(), ofill, cg, co, st["n_cells"], st["tree_levels"]))
    assert abs(cg - co) <= 0.04, (cg, co)
    b.make_forest()
    la2 = b.leaf_array()
    assert np.array_equal(la, la2), "forest not reproducible for a seed"
    b.close()


def test_repeated_builds_on_one_handle_are_identical():
    """The proposal / reverse-offer slot tables are memset only when a previous call may have left something in them
    (their consumers re-arm what they read): a second build on the same handle, and a build after a half-finished
    iteration (offers and proposals written, neither selected nor merged), must both reproduce the first build."""
    x = clustered(20000, 32, 8, 30, seed=3)
    b = make_builder(x, "euclidean", k=15, n_trees=4)

    def full():
        b.reset_graph()
        b.make_forest()
        b.init_from_leaves()
        b.init_random()
        b.descent()
        return b.finalize()

    i0, d0 = full()
    i1, d1 = full()  # both tables are known to be empty here: no memset
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(d0, d1)
    b.reset_graph()
    b.make_forest()
    b.init_from_leaves()
    b.init_random()
    b.descent_sample()
    b.descent_join()  # proposals stay in their slots: the next reset has to clear them
    i2, d2 = full()
    np.testing.assert_array_equal(i0, i2)
    np.testing.assert_array_equal(d0, d2)
    b.close()


def test_handle_lifecycle_park_take_release_rebuilds_identically():
    """Every device buffer of a handle has one owner (csrc/devmem.h), and one function arms a handle for a build: a build on
    a handle taken from the park, and one on a fresh handle after the parked one was released (for another geometry, and by
    nnd_release_pending), both reproduce the first build bit for bit."""
    from pynndescent_amd import _capi

    x = clustered(3000, 16, 4, 16, seed=1)

    def build(rows):
        b = make_builder(rows, "euclidean", k=10, n_trees=2)
        b.make_forest()
        b.init_from_leaves()
        b.init_random()
        b.descent()
        idx, dist = b.finalize()
        idx, dist = np.array(idx, copy=True), np.array(dist, copy=True)
        b.close()  # parks the handle
        return idx, dist

    i0, d0 = build(x)
    i1, d1 = build(x)  # same geometry, same seeds: the parked handle, re-armed
    np.testing.assert_array_equal(i0, i1)
    np.testing.assert_array_equal(d0, d1)
    i2, d2 = build(x[:2000])  # another geometry: the parked handle is released, a fresh one allocated
    check_graph_invariants(x[:2000], "euclidean", i2, d2, name="lifecycle n=2000")
    assert _capi.load_library().nnd_release_pending() == 0
    i3, d3 = build(x)  # nothing parked: fresh allocations
    np.testing.assert_array_equal(i0, i3)
    np.testing.assert_array_equal(d0, d3)


@pytest.mark.parametrize("k,mc", [(15, 15), (10, 10), (30, 30), (20, 12)])
def test_half_wave_select_equals_wave_select(k, mc):
    """k_sample_select_h (two vertices per wave) must produce exactly the lists and flag resets of k_sample_select."""
    x = clustered(6000, 24, 6, 25, seed=13)
    outs = []
    from pynndescent_amd import _capi

    for flags in (0, _capi.NND_FLAG_TEST_SELECT_WAVE):
        b = make_builder(x, "euclidean", k=k, n_trees=3, mc=mc, flags=flags)
        b.make_forest()
        b.init_from_leaves()
        b.init_random()
        # the first pass of a build: every edge new, the new class uses both slot banks (the WIDE forms of both kernels)
        b.sample_candidates()
        new0, old0 = b.candidates()
        _, _, fl0 = b.graph()
        assert (old0 == -1).all() and (new0[:, 0] >= 0).all()
        b.descent_iter()  # a mix of old and new entries
        b.sample_candidates()
        new, old = b.candidates()
        idx, _, fl = b.graph()
        # another sampling pass on the resulting state (mostly old edges, many inactive vertices)
        b.descent_iter()
        b.sample_candidates()
        new2, old2 = b.candidates()
        _, _, fl2 = b.graph()
        outs.append((new, old, idx, fl, new2, fl2, new0, fl0))
        b.close()
    for a, c in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, c)
    # the old lists of vertices without new candidates are not defined (the join skips them): compare where they are
    has_new = outs[0][0][:, 0] >= 0
    assert has_new.any()


@pytest.mark.parametrize("metric,n,d,k,mc", [("euclidean", 40000, 128, 30, 30), ("cosine", 25000, 64, 20, 20), ("euclidean", 30000, 33, 16, 32),
                                             ("euclidean", 20000, 100, 32, 17)])
def test_join_with_staged_neighbour_lists_equals_the_unstaged_join(metric, n, d, k, mc):
    """Round 6: k_local_join_w (17..32 candidates per class) stages the neighbour lists of a vertex's candidates in LDS by LDS-DMA
    when rows hold <= 32 neighbours; NND_FLAG_TEST_JOIN_UNSTAGED keeps the membership tests on global memory (rounds 3-5).  The
    proposals that leave a join are the same set either way, so whole builds are identical, entry for entry."""
    from pynndescent_amd import _capi

    x = clustered(n, d, 8, 30, seed=21)
    outs = []
    for flags in (0, _capi.NND_FLAG_TEST_JOIN_UNSTAGED):
        b = make_builder(x, metric, k=k, n_trees=4, mc=mc, flags=flags, join_blocks=0)
        b.make_forest()
        b.init_from_leaves()
        b.init_random()
        cs = [b.descent_iter() for _ in range(4)]
        idx, dist, fl = b.graph()
        outs.append((np.asarray(cs), idx, dist, fl))
        b.close()
    assert outs[0][0][0] > 0
    for a, c in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(a, c)


@pytest.mark.parametrize("metric,n,d,T", [("euclidean", 300000, 128, 8), ("cosine", 200000, 100, 5), ("euclidean", 180000, 40, 12)])
def test_coherent_routing_equals_plain_walk(metric, n, d, T):
    """The two-pass routing of the forest (top levels from LDS -> counting sort by bucket -> the bucket's subtree from
    LDS, rpforest.hip k_route_top / k_route_bucket) sends every point to the cell the one-walk kernel k_route sends it
    to: same splits, same coins (rp_trees.py:380-391).  The finishers are order independent, so the whole forest --
    the leaf array -- is identical."""
    from pynndescent_amd import _capi

    x = clustered(n, d, 16, 64, seed=23)
    leaves = []
    for flags in (0, _capi.NND_FLAG_TEST_ROUTE_PLAIN):
        b = make_builder(x, metric, k=15, n_trees=T, flags=flags)
        b.make_forest()
        la = b.leaf_array()
        assert b.stats()["n_cells"] > 0, "the routing forest did not run"
        leaves.append(la)
        b.close()
    assert leaves[0].shape == leaves[1].shape
    np.testing.assert_array_equal(leaves[0], leaves[1])
    # every tree is a partition of the points
    la = leaves[0]
    ids = la[la >= 0]
    assert ids.size == n * T and np.array_equal(np.bincount(ids, minlength=n), np.full(n, T))


@pytest.mark.parametrize("metric,n,d,k,T", [("euclidean", 6000, 32, 15, 4), ("cosine", 3000, 20, 10, 3),
                                            ("euclidean", 2500, 12, 30, 3)])
def test_leaf_array_seam_matches_reference_init_rp_tree(metric, n, d, k, T):
    """The `leaf_array` seam of nn_descent (pynndescent_.py:324-337): the ORACLE's forest (a restatement of the
    reference's make_forest + rptree_leaf_array) is handed to nnd_init_from_leaf_array; the k-lists must then hold what
    the reference's init_rp_tree leaves in its heaps on the SAME leaves -- compared exactly, row by row, as sets."""
    x = clustered(n, d, 6, 25, seed=n + k)
    _, _, ts = O.draw_rng_states(5, T)
    la = O.make_leaf_array(x, T, O.default_leaf_size(k), ts, O.ANGULAR[metric])
    b = make_builder(x, metric, k=k, n_trees=0)  # no forest of its own
    b.init_from_leaf_array(la)
    idx, dist, flags = b.graph()
    check_graph_invariants(x, metric, idx, dist, name="leaf_array_seam")
    assert np.all(flags[idx >= 0] == 1)
    oi, od, of = O.init_rp_tree(x, k, metric, la)
    same = 0
    for r in range(n):
        a, c = set(idx[r][idx[r] >= 0].tolist()), set(oi[r][oi[r] >= 0].tolist())
        if a == c:
            same += 1
            continue
        # rows may differ only through a tie (or an ulp) at the boundary distance: same sorted distances
        np.testing.assert_allclose(np.sort(dist[r][idx[r] >= 0]), np.sort(od[r][oi[r] >= 0]), rtol=2e-5, atol=1e-6)
    print("leaf_array seam %s: %d of %d rows identical as sets" % (metric, same, n))
    assert same >= 0.999 * n
    # leaves in an arbitrary ORDER (rounds are found by the library, not assumed to be trees): same result
    perm = np.random.RandomState(3).permutation(la.shape[0])
    b.reset_graph()
    b.init_from_leaf_array(la[perm])
    idx2, dist2, _ = b.graph()
    assert (np.sort(idx2, axis=1) == np.sort(idx, axis=1)).all(1).mean() >= 0.999
    b.close()


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_leaf_init_recall_gpu_forest_vs_reference_forest(metric):
    """Isolates the forest: recall of the k-lists right after leaf seeding, with the GPU's own forest (top of every tree
    drawn from a 1/8 sample at this size) against the reference algorithm's forest (oracle) through the SAME seeding
    kernel.  Both are random forests of the same family: the recalls must agree within 1.5 % (two-sided)."""
    n, d, k, T = 200_000, 48, 15, 8
    x = clustered(n, d, 10, 400, seed=17)
    rows = np.random.RandomState(0).choice(n, 2000, replace=False)
    ti, _ = O.brute_force_knn(x, 11, metric, rows=rows, kind="fast")
    b = make_builder(x, metric, k=k, n_trees=T)
    b.make_forest()
    assert b.stats()["n_cells"] > 0  # the routing forest (sampled tops) is what is being tested
    b.init_from_leaves()
    g_idx, _, _ = b.graph()
    _, _, ts = O.draw_rng_states(1, T)
    la = O.make_leaf_array(x, T, O.default_leaf_size(k), ts, O.ANGULAR[metric])
    b.reset_graph()
    b.init_from_leaf_array(la)
    o_idx, _, _ = b.graph()
    rg, ro = O.recall(ti, g_idx[rows]), O.recall(ti, o_idx[rows])
    print("recall@10 after leaf seeding (%s, %d trees): GPU forest %.4f, reference forest %.4f" % (metric, T, rg, ro))
    assert abs(rg - ro) <= 0.015
    b.close()


@pytest.mark.parametrize("k,mc", [(15, 15), (40, 40), (100, 60)])
def test_sampling_falls_back_to_hashed_slots_when_the_record_regions_cannot_be_allocated(k, mc):
    """Round-5 advisor item: the record regions of the bucketed transposition take 0.5 GB per million rows at k = 15 and
    several GB at wide rows; an allocation failure there must not fail the build.  NND_FLAG_TEST_SAMPLE_NOMEM makes the
    first allocation "fail": the handle switches to the hashed atomicMin slots (round 1-4 form) for good and builds a graph
    of the same quality as the default path (reference: new_build_candidates, utils.py:222-320)."""
    from pynndescent_amd import _capi

    x = clustered(20000, 32, 8, 64, seed=21)
    rows = np.random.RandomState(3).choice(x.shape[0], 1500, replace=False)
    ti, _ = O.brute_force_knn(x, 10, "euclidean", rows=rows)
    rec = []
    for flags in (0, _capi.NND_FLAG_TEST_SAMPLE_NOMEM):
        b = make_builder(x, "euclidean", k=k, n_trees=4, mc=mc, flags=flags)
        for _ in range(2):  # (a second build on the same handle: the switch is permanent)
            b.reset_graph()
            b.make_forest()
            b.init_from_leaves()
            b.init_random()
            b.descent()
            idx, dist = b.finalize()
        if k <= 15:
            check_graph_invariants(x, "euclidean", idx, dist, name="nomem flags=%d" % flags)
        assert (idx >= 0).all()
        rec.append(O.recall(ti, idx[rows]))
        b.close()
    print("k=%d mc=%d recall@10: default %.4f, hashed-slot fallback %.4f" % (k, mc, rec[0], rec[1]))
    assert abs(rec[0] - rec[1]) <= 0.01 and rec[1] >= 0.9


@pytest.mark.parametrize("k,mc,stage,share_tol,fill_tol,tv_tol", [(15, 15, "first", 0.03, 0.01, 0.03), (15, 15, "mixed", 0.006, 0.002, 0.01),
                                                                   (30, 30, "mixed", 0.02, 0.01, 0.06), (20, 10, "mixed", 0.03, 0.01, 0.03)])
def test_candidate_lists_have_the_reference_algorithms_distribution(k, mc, stage, share_tol, fill_tol, tv_tol):
    """Round-5 review: the exact-sample test above checks the kernel against a host model of the LIBRARY'S OWN hashes; this one
    compares the lists with what the REFERENCE ALGORITHM (the oracle's new_build_candidates, pinned bit-exact to utils.py:222-320)
    builds from the SAME graph state -- as distributions, the priorities being random on both sides: per-vertex fill of the new
    and old lists, the share of forward (own-row) entries in them, the histogram of the fills.
    Measured (round 6): where the lists are not full (k = mc = 15 after an iteration) every figure agrees to 0.002.  Two known
    deviations set the other tolerances: (1) FULL lists hold 2 points fewer forward entries than the reference's (0.757 vs 0.779
    on a first pass): the reference gives a mutual neighbour a second, order-dependent draw, the library keeps the forward draw
    (sample.hip, before nnd_offer_salt: the order-independent alternative was measured and has the worse graph); (2) k = 30: some
    of the 32-slot old-class banks overflow and fall back to hashed minima -- 0.3 % fewer old candidates, 0.8 points more
    forward entries among them."""
    n = 60000
    x = clustered(n, 32, 8, 64, seed=5)
    b = make_builder(x, "euclidean", k=k, n_trees=4, mc=mc)
    b.make_forest()
    b.init_from_leaves()
    b.init_random()
    if stage == "mixed":
        b.descent_iter()  # a mix of old and new entries, some vertices without any new edge
    idx0, _, fl0 = b.graph()
    b.sample_candidates()
    new, old = b.candidates()
    b.close()
    lib = O.load("strict")
    onew = np.empty((n, mc), np.int32)
    oold = np.empty((n, mc), np.int32)
    lib.orc_new_build_candidates(idx0.copy(), fl0.copy(), n, k, mc, np.array([11, 22, 33], np.int64), 8, onew, oold)

    def stats(lists, rows):
        fill = (lists[rows] >= 0).sum(1)
        fwd = (lists[rows][:, :, None] == idx0[rows][:, None, :]).any(2) & (lists[rows] >= 0)
        hist = np.bincount(fill, minlength=mc + 1) / float(len(rows))
        return fill.mean(), fwd.sum() / max(1, (lists[rows] >= 0).sum()), hist

    every = np.arange(n)
    # the join skips a vertex without new candidates, and the library does not build its old list: compare the old lists
    # where both sides have new candidates
    # (the reference's lists are HEAPS: slot 0 is the root, filled last -- "has a candidate" is any(), not [:, 0])
    joined = np.nonzero((new >= 0).any(1) & (onew >= 0).any(1))[0]
    assert len(joined) > 2000, len(joined)
    for name, g_l, o_l, rows in (("new", new, onew, every), ("old", old, oold, joined)):
        gm, gf, gh = stats(g_l, rows)
        om, of, oh = stats(o_l, rows)
        tv = 0.5 * np.abs(gh - oh).sum()
        print("%s lists (k=%d mc=%d %s): mean fill gpu %.3f reference %.3f; forward share gpu %.4f reference %.4f; fill histogram TV %.4f"
              % (name, k, mc, stage, gm, om, gf, of, tv))
        assert abs(gm - om) <= fill_tol * max(om, 1.0) + 0.01, (name, gm, om)
        assert abs(gf - of) <= share_tol, (name, gf, of)
        assert tv <= tv_tol, (name, tv)
    # the same vertices take part in the join (a vertex is active iff it has a new candidate)
    a_gpu, a_ref = int((new >= 0).any(1).sum()), int((onew >= 0).any(1).sum())
    print("vertices with a new candidate: gpu %d reference %d of %d" % (a_gpu, a_ref, n))
    assert abs(a_gpu - a_ref) <= 0.002 * n, (a_gpu, a_ref)
