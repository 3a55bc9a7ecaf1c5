"""The host model of leaf seeding (tests/leaf_reference.py) pinned without a GPU: against the oracle's init_rp_tree (the
reference's sequential checked_flagged_heap_push over all leaf pairs) on the same leaf arrays, its work list and counters
against hand-written expectations, the ambiguity caps of every case of tests/leaf_cases.py on the model alone, and the
sensitivity of the GPU test's comparison.  A wrong model fails HERE, not on the GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import descent_cases as DC
from tests import leaf_cases as LC
from tests import leaf_reference as LR
from tests.test_gpu_leaf_exact import _check

_RES = {}


def _model(name):
    """the model's result of a case, once per session (read-only)."""
    if name not in _RES:
        case = LC.ALL[name]
        _RES[name] = LR.reference_seed(LC.prepared(case), case.metric, case.k, LC.leaf_array(case))
    return _RES[name]


def _oracle(case, la):
    hi, hd, hf = O.init_rp_tree(np.ascontiguousarray(LC.data(case)), case.k, case.metric, la, lib=O.load("strict"))
    return DC.sort_rows(hi, hd, hf)


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", sorted(n for n, c in LC.LATTICE.items() if c.kind == "partition"))
def test_model_equals_sequential_pushes_on_the_lattice(name):
    """ids, distance bits and flags of every row without a tie at its k-th place."""
    case, res = LC.ALL[name], _model(name)
    oi, od, of = _oracle(case, LC.leaf_array(case))
    clear = res.ambiguous == 0
    assert np.array_equal(res.ids[clear], oi[clear])
    assert np.array_equal(np.where(res.ids >= 0, res.dists, np.inf).astype(np.float32)[clear], od[clear])
    assert np.array_equal(res.flags[clear], of[clear])
    differ = int((res.ids[~clear] != oi[~clear]).any(1).sum())
    print("%s: %d of %d rows tie at the k-th place, %d of them end differently under sequential pushes" % (name, int((~clear).sum()), case.n, differ))
    assert clear.mean() >= 1.0 - LC.LATTICE_CAP


@pytest.mark.parametrize("name", ["leaf_qw45_k15_d40", "leaf_sym610_k30_d24", "leaf_rb10_k64_d16", "leaf_wide10_k100_d40", "leaf_chain_k15",
                                  "leaf_garbage_k30"])
def test_model_holds_the_id_sets_of_sequential_pushes_on_float_data(name):
    case, res = LC.ALL[name], _model(name)
    oi, _, of = _oracle(case, LC.leaf_array(case))
    clear = res.ambiguous == 0
    assert np.array_equal(np.sort(res.ids[clear], axis=1), np.sort(oi[clear], axis=1))
    assert np.all(of[oi >= 0] == 1) and np.all(res.flags[res.ids >= 0] == 1)


def test_the_reference_does_not_cut_long_leaves_and_the_model_does():
    """The oracle pushes every pair of a 513-point leaf, the library only those inside a run of 256: where a point's nearest
    leaf-mates sit in another run the two MUST differ, so the cut cases are not compared with the oracle.  What is compared: the
    rows of the points outside the long leaves, and the model against the oracle on the array cut by hand."""
    case, res = LC.ALL["leaf_lattice_cut_k15"], _model("leaf_lattice_cut_k15")
    la = LC.leaf_array(case)
    oi, od, _ = _oracle(case, la)
    clear = res.ambiguous == 0
    long_rows = np.nonzero((la >= 0).sum(1) > 256)[0]
    assert [int((la[r] >= 0).sum()) for r in long_rows] == [257, 300, 512, 513]
    in_long = np.zeros(case.n, bool)
    in_long[la[long_rows][la[long_rows] >= 0]] = True
    assert (res.ids[clear & in_long] != oi[clear & in_long]).any(1).sum() > 100
    assert np.array_equal(res.ids[clear & ~in_long], oi[clear & ~in_long])
    by_hand = []
    for row in la:
        m = row[row >= 0]
        by_hand += [m[a:a + 256] for a in range(0, len(m), 256)]
    cut = np.full((len(by_hand), 256), -1, np.int32)
    for i, m in enumerate(by_hand):
        cut[i, :len(m)] = m
    ci, cd, _ = _oracle(case, cut)
    assert np.array_equal(res.ids[clear], ci[clear])
    assert np.array_equal(np.where(res.ids >= 0, res.dists, np.inf).astype(np.float32)[clear], cd[clear])


def test_a_candidate_exactly_at_the_worst_distance_is_a_tie_and_nothing_else_is():
    """k = 2 on a line: point 0 at the origin with mates at distances 1, 4, 4 (ids 1, 2, 3) -- the k-th and (k+1)-th distances are
    equal, the row is flagged; with the third mate at 9 nothing is."""
    h = np.array([[0, 0], [1, 0], [0, 2], [0, 3]], np.float32)
    x = np.vstack([h, -h])  # 0 origin, 1 (1, 0), 2 (0, 2), 3 (0, 3), 6 (0, -2)
    res = LR.reference_seed(x, "euclidean", 2, np.array([[0, 1, 2, 6]], np.int32), exact=True)
    assert res.ambiguous[0] == LR.R_TIE and res.ids[0].tolist() == [1, 2] and res.dists[0].tolist() == [1.0, 4.0]
    assert res.ambiguous.tolist() == [1, 1, 0, 0, 0, 0, 0, 0]  # row 1 sees 1, 5, 5: a tie too; rows 2 and 6 see 4, 5, 16
    res = LR.reference_seed(x, "euclidean", 2, np.array([[0, 1, 2, 3]], np.int32), exact=True)
    assert res.ambiguous[0] == 0 and res.ids[0].tolist() == [1, 2]
    assert res.ids[5].tolist() == [-1, -1] and np.isinf(res.dists[5]).all() and res.n_union[5] == 0


# ------------------------------------------------------------------------------------------------ the work list
def _runs(w):
    return [(p.tolist(), int(r)) for p, r in zip(w.pieces, w.rounds)]


def test_work_list_of_a_chain():
    """leaf i shares a point with leaf i + 1: one round each; a disjoint leaf goes back to round 0, a leaf that meets the chain's
    last leaf goes behind it."""
    la = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [7, 8, -1], [6, 9, -1]], np.int32)
    w = LR.work_list(la, 10)
    assert _runs(w) == [([0, 1, 2], 0), ([7, 8], 0), ([2, 3, 4], 1), ([4, 5, 6], 2), ([6, 9], 3)]
    assert (w.n_rounds, w.longest) == (4, 3) and w.leaves.tolist() == [0, 3, 1, 2, 4]
    case = LC.ALL["leaf_chain_k15"]
    w = _model(case.name).work
    assert w.n_rounds == case.rounds == 31 and [int(w.rounds[w.leaves == i][0]) for i in range(30)] == list(range(30))


def test_work_list_cuts_long_leaves_and_drops_runs_of_one():
    la = np.full((3, 600), -1, np.int32)
    la[0, :257], la[1, :513], la[2, :300] = np.arange(257), np.arange(300, 813), np.arange(900, 1200)
    w = LR.work_list(la, 1200)
    assert [len(p) for p in w.pieces] == [256, 256, 256, 256, 44] and w.rounds.tolist() == [0] * 5 and w.leaves.tolist() == [0, 1, 1, 2, 2]
    assert w.pieces[0].tolist() == list(range(256)) and w.pieces[2].tolist() == list(range(556, 812)) and w.longest == 256
    res = LR.reference_seed(np.zeros((1200, 4), np.float32), "euclidean", 4, la, exact=True)
    assert res.n_union[256] == 0 and res.n_union[812] == 0        # the points left alone
    assert res.n_union[0] == 255 and res.n_union[1199] == 43      # no pair across two runs of one leaf
    assert not np.isin(res.possible, [300 * 1200 + 556, 556 * 1200 + 300]).any()


def test_work_list_ends_a_row_at_its_first_negative_entry():
    la = np.array([[3, 4, -1, 7, 99], [-1, 5, 6, 7, 8], [5, -1, -1, -1, -1], [-1, -1, -1, -1, -1], [5, 6, -2, 6, 6]], np.int32)
    w = LR.work_list(la, 10)
    assert _runs(w) == [([3, 4], 0), ([5, 6], 0)] and w.leaves.tolist() == [0, 4]
    with pytest.raises(LR.LeafArrayError, match="leaf 1 holds point 10 but n = 10"):
        LR.work_list(np.array([[0, 1], [2, 10]], np.int32), 10)
    with pytest.raises(LR.LeafArrayError, match="point 2 occurs twice in leaf 1"):
        LR.work_list(np.array([[0, 1, -1], [2, 3, 2]], np.int32), 10)
    LR.work_list(np.array([[2, -1, 2], [2, 3, -1]], np.int32), 10)  # a one-point leaf leaves no mark


@pytest.mark.parametrize("name", sorted(LC.ALL))
def test_case_reaches_its_instances_in_its_rounds(name):
    case, res = LC.ALL[name], _model(name)
    assert tuple(f.name for f in res.forms) == case.forms and res.work.n_rounds == case.rounds and res.work.longest == case.longest
    lens = np.array([len(p) for p in res.work.pieces])
    for f in res.forms:  # every launch of a round has runs of its own, at both ends of its size class
        assert (lens == min(f.m_hi, case.longest)).any() and (lens == max(f.m_lo + 1, 2)).any(), f
    assert (lens < case.k + 1).mean() > 0.25 or case.kind != "partition"


def test_every_launched_instance_is_named_by_a_case():
    named = {f for c in LC.ALL.values() for f in c.forms}
    table = {f.name for k in (8, 16, 17, 32, 33, 64, 65, 256) for m in (2, 64, 65, 80, 81, 96, 97, 128, 129, 160, 161, 256) for f in LR.forms(k, m)}
    assert len(table) == 15 and named == table


# ------------------------------------------------------------------------------------------------ the counters
def test_counters_by_hand():
    """Two tiny arrays.  Runs of 17 and 40 points at k = 15, d = 24 (dp = 32: 8 k-steps): k_leaf_join<4,8,64,true> computes the
    upper triangle, 3 and 6 tiles.  Runs of 100 and 130 points at k = 40, d = 130 (dp = 160: 40 k-steps): k_leaf_join_rb<10,8>
    computes whole rows of tiles, 7 x 7 and 9 x 9."""
    assert LR.counters([17, 40, 1], 15, 24)[:3] == (17 * 16 // 2 + 40 * 39 // 2, 57, (3 + 6) * 8)
    assert LR.counters([100, 130], 40, 130)[:3] == (100 * 99 // 2 + 130 * 129 // 2, 230, (49 + 81) * 40)
    assert [f.name for f in LR.counters([100, 130], 40, 130)[3]] == [LC.RB10]
    # two size classes: the run of 65 goes to <5,8,64,true> (5 tile rows: 15 tiles), the run of 64 to <4,4,64,true> (10 tiles)
    assert LR.counters([64, 65], 16, 5)[2] == (10 + 15) * 8
    # the same runs under k = 30: sym<6> takes both
    assert LR.counters([64, 65], 30, 5)[2] == (10 + 15) * 8 and LR.counters([64, 97], 30, 5)[2] == (10 + 28) * 8
    # the library's forest hands the dispatch max(leaf_size, longest leaf): leaves of 60 under leaf_size 75 still take two launches
    assert [f.name for f in LR.counters([60, 30], 15, 5, longest=75)[3]] == [LC.QW44, LC.QW5]
    la = np.array([[0, 1, 2, 3, -1], [4, 5, -1, -1, -1], [6, -1, -1, -1, -1]], np.int32)
    res = LR.reference_seed(np.zeros((8, 3), np.float32), "euclidean", 2, la, exact=True)
    assert (res.leaf_pairs, res.leaf_rows, res.leaf_mfma) == (6 + 1, 6, 2 * 8)


# ------------------------------------------------------------------------------------------------ the caps
@pytest.mark.parametrize("name", sorted(LC.ALL))
def test_case_stays_inside_its_cap(name):
    case, res = LC.ALL[name], _model(name)
    share = float((res.ambiguous != 0).mean())
    filled = (res.ids >= 0).sum(1)
    print("%s (%s): %.2f %% of %d rows flagged %s; rows filled %d..%d, %.0f %% full" % (
        name, ", ".join(case.forms), 100 * share, case.n, np.bincount(res.ambiguous, minlength=4).tolist(), filled.min(), filled.max(),
        100 * (filled == case.k).mean()))
    assert share <= LC.cap(case)
    assert (res.n_union > case.k).any() and (res.n_union > 0).mean() > 0.99  # rows are contested, and nearly all are seeded


# ------------------------------------------------------------------------------------------------ the comparison's sensitivity
def _as_gpu(res):
    """the model's rows as a graph(): float32 distances, ordered by (float32 distance, id) as the kernels' keys are."""
    return tuple(a.copy() for a in DC.sort_rows(res.ids, np.where(res.ids >= 0, res.dists, np.inf).astype(np.float32), res.flags))


def _clear_row(res, k, want=lambda t: True):
    for t in np.nonzero((res.ambiguous == 0) & (res.n_union > k + 2))[0]:
        if want(int(t)):
            return int(t)
    raise AssertionError("no such row")


@pytest.mark.parametrize("name,change", [(n, c) for n in ("leaf_qw45_k15_d40", "leaf_lattice_sym_k30", "leaf_cut_k100", "leaf_lattice_cut_k15")
                                         for c in ("id", "distance", "flag", "order", "cross") if c != "cross" or LC.ALL[n].kind == "cut"])
def test_the_comparison_reports_one_wrong_entry_of_an_unflagged_row(name, change):
    """The model's own result passes; with ONE change it must fail, naming the row, which the model does not flag."""
    case, res = LC.ALL[name], _model(name)
    k, n = case.k, case.n
    _check(name, case, None, _as_gpu(res), res)
    gi, gd, gf = _as_gpu(res)
    if change == "id":  # the k-th entry swapped for the (k+1)-th mate
        t = _clear_row(res, k)
        mates, mid, _ = LR.row_mates(res, n, t)
        o = np.lexsort((mates, mid))
        gi[t, k - 1], gd[t, k - 1] = mates[o][k], mid[o][k]
    elif change == "distance":  # two radii off (a whole unit where the radius is 0)
        t = _clear_row(res, k)
        gd[t, k - 1] = np.float32(res.dists[t, k - 1] + max(2.0 * res.radius[t, k - 1], 1.0 if case.exact else 0.0))
        assert abs(float(gd[t, k - 1]) - res.dists[t, k - 1]) > res.radius[t, k - 1]
    elif change == "flag":
        t = _clear_row(res, k)
        gf[t, 3] = 0
    elif change == "order":
        t = _clear_row(res, k)
        gi[t, [2, 3]], gd[t, [2, 3]] = gi[t, [3, 2]], gd[t, [3, 2]]
    else:  # a pair across two runs of one leaf, at its true distance
        la = LC.leaf_array(case)
        long_leaf = la[np.nonzero((la >= 0).sum(1) == 513)[0][0]]
        first, second = long_leaf[:256], long_leaf[256:512]
        prep = LC.prepared(case)
        mid = prep.block(first[None, :], second[None, :])[0][0]
        th = res.dists[first, k - 1]
        ok = (res.ambiguous[first] == 0)[:, None] & (mid < 0.5 * th[:, None]) & ~(res.ids[first][:, :, None] == second[None, None, :]).any(1)
        i, j = np.argwhere(ok)[0]
        t, q, d = int(first[i]), int(second[j]), float(mid[i, j])
        at = int(np.searchsorted(res.dists[t], d))
        gi[t, at + 1:], gd[t, at + 1:], gf[t, at + 1:] = gi[t, at:-1].copy(), gd[t, at:-1].copy(), gf[t, at:-1].copy()
        gi[t, at], gd[t, at], gf[t, at] = q, d, 1
    assert res.ambiguous[t] == 0
    with pytest.raises(AssertionError, match=r": row %d \(clear\)" % t):
        _check(name, case, None, (gi, gd, gf), res)
