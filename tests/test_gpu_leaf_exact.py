"""Leaf seeding (csrc/leaf_join.hip with the merges of csrc/merge.h, through Builder.init_from_leaf_array and
Builder.init_from_leaves) against the step-exact host model (tests/leaf_reference.py), row by row.  Rows the model does not flag
must hold the model's id set, the model's flag per id and per id a stored distance within the model's a-priori radius (the same
bits on the lattice), ascending by (distance, id) and packed to the front, (empty, +inf) behind the last entry; flagged rows keep
the weak checks (sorted, unique, packed, ids from row U run-mates, the distance of the id, at least min(k, |union|) entries).
leaf_pairs and leaf_rows must be the model's, and leaf_mfma the model's count for the expected instances -- the assertion that
the named kernel family ran.  Seeding a fresh builder again must give the same bytes.

The cases, which instance each reaches and the ambiguity caps are in tests/leaf_cases.py; the model, the caps and the
sensitivity of ``_check`` are pinned without a GPU in tests/test_leaf_reference_cpu.py."""
import numpy as np
import pytest

from oracle import oracle as O
from pynndescent_amd import _capi
from tests import leaf_cases as LC
from tests import leaf_reference as LR

pytestmark = pytest.mark.gpu


def _by_id(ids, *cols):
    o = np.argsort(ids, axis=1, kind="stable")
    return [np.take_along_axis(a, o, 1) for a in (ids,) + cols]


def _describe(t, before, res, got):
    gi, gd, gf = got
    out = "row %d (%s), its runs (leaf, round, size) %s, %d in row U mates" % (
        t, LR.reason_text(int(res.ambiguous[t])), LR.row_leaves(res, t), int(res.n_union[t]))
    if before is not None:
        out += "\n    before   %s\n             %s" % (before[0][t].tolist(), before[1][t].tolist())
    return out + "\n    expected %s\n             %s flags %s\n    got      %s\n             %s flags %s" % (
        res.ids[t].tolist(), res.dists[t].tolist(), res.flags[t].tolist(), gi[t].tolist(), gd[t].tolist(), gf[t].tolist())


def _check(label, case, before, got, res):
    """the exact comparison of the unflagged rows and the weak checks of the flagged ones; returns max |err| / radius."""
    gi, gd, gf = got
    n, k = gi.shape
    filled = gi >= 0
    g64 = np.where(filled, gd.astype(np.float64), np.inf)
    bad = {}

    def fail(rows, why):
        for t in rows[:4]:
            bad.setdefault(int(t), why)

    # ---- every row: packed, ascending by (distance, id), (empty, +inf) behind the last entry ----
    fail(np.nonzero((filled[:, 1:] & ~filled[:, :-1]).any(1))[0], "row not packed")
    fail(np.nonzero((~filled & ~np.isposinf(gd)).any(1))[0], "an unfilled slot does not hold +inf")
    both_on = filled[:, 1:] & filled[:, :-1]
    with np.errstate(invalid="ignore"):  # (inf - inf behind the last entry)
        dd, di = np.diff(g64, axis=1), np.diff(gi.astype(np.int64), axis=1)
        fail(np.nonzero((both_on & ((dd < 0) | ((dd == 0) & (di <= 0)))).any(1))[0], "row not ascending by (distance, id)")
    clear = res.ambiguous == 0
    a_id, a_d, a_f = _by_id(gi, g64, gf)
    m_id, m_d, m_r, m_f = _by_id(res.ids, res.dists, res.radius, res.flags)
    same_ids = (a_id == m_id).all(1)
    fail(np.nonzero(clear & ~same_ids)[0], "ids differ")
    both = clear & same_ids
    fail(np.nonzero(both & ((a_f != m_f) & (m_id >= 0)).any(1))[0], "flags differ")
    fin = np.isfinite(m_d)
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(a_d - m_d), 0.0)
    off = (err > m_r) | (np.isfinite(a_d) != fin)
    fail(np.nonzero(both & off.any(1))[0], "a stored distance is outside the radius" if not case.exact else "distance bits differ")
    ins = both[:, None] & fin & (m_r > 0.0)
    ratio = float((err[ins] / m_r[ins]).max()) if ins.any() else 0.0
    # ---- flagged rows: unique, every id a run-mate or in the row before, every distance that of its id, enough entries ----
    for t in np.nonzero(~clear)[0]:
        row = gi[t][filled[t]]
        if len(set(row.tolist())) != len(row):
            fail([t], "ids not unique")
            continue
        if len(row) < min(k, int(res.n_union[t])):
            fail([t], "fewer entries than min(k, |row U mates|)")
            continue
        mates, mid, rad = LR.row_mates(res, n, t)
        prior = {} if before is None else {int(i): (float(np.float32(d)), int(f)) for i, d, f in zip(before[0][t], before[1][t], before[2][t]) if i >= 0}
        for j, i in enumerate(row.tolist()):
            if i in prior:
                if g64[t, j] != prior[i][0] or gf[t, j] != prior[i][1]:
                    fail([t], "a surviving entry changed its distance or flag")
                continue
            at = np.searchsorted(mates, i)
            if at >= len(mates) or mates[at] != i:
                fail([t], "an id that is no run-mate")
            elif not abs(g64[t, j] - mid[at]) <= rad[at] or gf[t, j] != 1:
                fail([t], "a distance is not that of its id, or the new flag is missing")
    assert not bad, "%s: rows differ from the model, first %d:\n%s" % (label, len(bad), "\n".join(
        why + ": " + _describe(t, before, res, got) for t, why in list(bad.items())[:6]))
    return ratio


def _seed(case, la, graph=None, **kw):
    b = LC.builder(case, **kw)
    try:
        before = None
        if graph is not None:
            b.init_from_graph(graph)
            before = b.graph()
        b.init_from_leaf_array(la)
        return before, b.graph(), b.stats()
    finally:
        b.close()


def _compare(label, case, la, before, got, st, longest=None):
    res = LR.reference_seed(LC.prepared(case), case.metric, case.k, la, before, longest=longest)
    share = float((res.ambiguous != 0).mean())
    names = [f.name for f in res.forms]
    print("%s (%s; %s): %.2f %% of %d rows flagged %s, %d runs in %d rounds, longest %d; pairs / rows / mfma gpu %s model %s" % (
        label, ", ".join(names), case.doc, 100 * share, case.n, np.bincount(res.ambiguous, minlength=4).tolist(), len(res.work.pieces),
        res.work.n_rounds, res.work.longest, (st["leaf_pairs"], st["leaf_rows"], st["leaf_mfma"]), (res.leaf_pairs, res.leaf_rows, res.leaf_mfma)))
    ratio = _check(label, case, before, got, res)
    print("%s: max |err| / radius %.3f" % (label, ratio))
    assert share <= LC.cap(case), "%s: %.2f %% of the rows are flagged, the cap is %.0f %%" % (label, 100 * share, 100 * LC.cap(case))
    assert (st["leaf_pairs"], st["leaf_rows"]) == (res.leaf_pairs, res.leaf_rows), label
    assert st["leaf_mfma"] == res.leaf_mfma, "%s: leaf_mfma %d, the model counts %d for %s" % (label, st["leaf_mfma"], res.leaf_mfma, names)
    return res


@pytest.mark.parametrize("name", sorted(LC.ALL))
def test_leaf_seeding_equals_the_model(name):
    case = LC.ALL[name]
    la = LC.leaf_array(case)
    _, got, st = _seed(case, la)
    res = _compare(name, case, la, None, got, st)
    assert tuple(f.name for f in res.forms) == case.forms and res.work.n_rounds == case.rounds
    _, again, _ = _seed(case, la)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), name + ": a second seeding of a fresh builder differs"


@pytest.mark.parametrize("name", LC.BEFORE)
def test_seeding_merges_into_rows_that_are_not_empty(name):
    """init_from_graph with a partial graph, then the leaves: survivors keep their stored distance and flag, the row before is part
    of the union, a run-mate that is in the row already is not inserted twice."""
    case = LC.ALL[name]
    la = LC.leaf_array(case)
    before, got, st = _seed(case, la, LC.partial_graph(case))
    assert (before[0] >= 0).any() and (before[0][::11] < 0).all()
    res = _compare(name + " on a partial graph", case, la, before, got, st)
    kept = (res.ids[:, :, None] == before[0][:, None, :]) & (res.ids[:, :, None] >= 0)
    assert kept.any() and not kept.any(2)[res.ids >= 0].all()  # both kinds of entry are in the result


def test_errors_leave_the_builder_usable():
    """a point >= n and a point twice in one leaf raise NNDError with the message the code sets (the model raises the same text);
    the builder then still seeds correctly from a valid array."""
    case = LC.ALL["leaf_qw45_k15_d40"]
    la = LC.leaf_array(case)
    b = LC.builder(case)
    try:
        for mutate in ((lambda a: a.__setitem__((5, 1), case.n)), (lambda a: a.__setitem__((9, 1), a[9, 0]))):
            wrong = np.array(la)
            mutate(wrong)
            with pytest.raises(LR.LeafArrayError) as want:
                LR.work_list(wrong, case.n)
            with pytest.raises(_capi.NNDError) as err:
                b.init_from_leaf_array(wrong)
            assert str(err.value) == str(want.value)
        assert (b.graph()[0] < 0).all()  # a refused array has touched nothing
        b.init_from_leaf_array(la)
        got, st = b.graph(), b.stats()
    finally:
        b.close()
    _compare("after two refused arrays", case, la, None, got, st)


def _forest_route(case, leaf_size, max_depth, n_trees=2):
    b = LC.builder(case, n_trees=n_trees, leaf_size=leaf_size, max_depth=max_depth)
    try:
        b.make_forest()
        la = b.leaf_array()
        b.init_from_leaves()
        return la, b.graph(), b.stats()
    finally:
        b.close()


def test_the_librarys_own_forest_with_leaves_longer_than_256():
    """make_forest with max_depth 3 leaves ~500 points a leaf; init_from_leaves cuts them into runs of 256 consecutive positions
    of ``perm`` -- the member order of leaf_array() (rpforest.hip k_fill_leaf_array), so the model cuts leaf_array() the same way."""
    case = LC.ALL["leaf_cut_k15"]
    la, got, st = _forest_route(case, O.default_leaf_size(case.k), 3)
    assert ((la >= 0).sum(1) > 256).any()
    res = _compare("forest with max_depth 3", case, la, None, got, st)
    assert res.work.longest == 256 and [f.name for f in res.forms] == [LC.RB16]


def test_the_librarys_own_forest_at_its_default_leaf_size():
    """k = 15 through make_forest and init_from_leaves: the ordinary route (no cut: the dispatch is handed max(leaf_size, longest
    leaf), rpforest.hip :2362-2367)."""
    case = LC.ALL["leaf_qw45_k15_d40"]
    ls = O.default_leaf_size(case.k)
    la, got, st = _forest_route(case, ls, 200, n_trees=3)
    longest = int((la >= 0).sum(1).max())
    assert longest <= 256
    res = _compare("forest at leaf_size %d" % ls, case, la, None, got, st, longest=max(ls, longest))
    assert [f.name for f in res.forms] == [LC.QW44, LC.QW5]
