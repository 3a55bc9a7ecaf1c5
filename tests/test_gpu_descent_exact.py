"""One nnd_descent_iter (csrc/join.hip + csrc/merge.hip through csrc/capi.hip descent_iter) against the step-exact host model
(tests/descent_reference.py), row by row.  Every checked iteration is compared with the model applied to the GPU's OWN graph()
before it and the candidate lists it used, so a deviation does not compound.  Rows the model does not flag must hold the
model's id set, the model's flag per id, and per id a stored distance within the model's a-priori radius (the same bits on the
lattice), ascending; flagged rows keep the weak checks (sorted, unique, ids from row U proposals, the distance of the id).
c and the proposal counter must be the model's: exactly on the lattice, within the number of unclear decisions on float data;
the pair counter always exactly.

The cases, which kernel form each reaches and the ambiguity caps are in tests/descent_cases.py; the model and the caps are
pinned without a GPU in tests/test_descent_reference_cpu.py."""
import numpy as np
import pytest

from tests import descent_cases as DC
from tests import descent_reference as DR
from tests.gpu_util import make_builder

pytestmark = pytest.mark.gpu


def _builder(case):
    b = make_builder(np.array(DC.data(case)), case.metric, k=case.k, n_trees=case.n_trees, mc=case.mc, seed=case.seed,
                     join_blocks=case.join_blocks, flags=case.flags)
    if case.n_trees:
        b.make_forest()
        b.init_from_leaves()
    b.init_random()
    return b


def _by_id(ids, *cols):
    o = np.argsort(ids, axis=1, kind="stable")
    return [np.take_along_axis(a, o, 1) for a in (ids,) + cols]


def _describe(t, n, s0, res, got):
    gi, gd, gf = got
    return ("row %d (%s)\n    before   %s\n             %s\n    partners %s\n    expected %s\n             %s flags %s\n    got      %s\n"
            "             %s flags %s" % (t, DR.reason_text(int(res.ambiguous[t])), s0[0][t].tolist(), s0[1][t].tolist(),
                                          DR.row_partners(res, n, t).tolist(), res.ids[t].tolist(), res.dists[t].tolist(),
                                          res.flags[t].tolist(), gi[t].tolist(), gd[t].tolist(), gf[t].tolist()))


def _check(label, case, prep, s0, got, res):
    """the exact comparison of the unflagged rows and the weak checks of the flagged ones; returns max |err| / radius."""
    gi, gd, gf = got
    n, k = gi.shape
    g64 = np.where(gi >= 0, gd.astype(np.float64), np.inf)
    bad = {}

    def fail(rows, why):
        for t in rows[:4]:
            bad.setdefault(int(t), why)

    order = np.where(np.isfinite(g64), g64, 1e39)
    fail(np.nonzero((np.diff(order, axis=1) < 0).any(1))[0], "row not ascending")
    assert np.all(np.isinf(gd[gi < 0])), label + ": an unfilled slot does not hold +inf"
    clear = res.ambiguous == 0
    a_id, a_d, a_f = _by_id(gi, g64, gf)
    m_id, m_d, m_r, m_f = _by_id(res.ids, res.dists, res.radius, res.flags)
    same_ids = (a_id == m_id).all(1)
    fail(np.nonzero(clear & ~same_ids)[0], "ids differ")
    both = clear & same_ids
    fail(np.nonzero(both & (a_f != m_f).any(1))[0], "flags differ")
    fin = np.isfinite(m_d)
    with np.errstate(invalid="ignore"):
        err = np.where(fin, np.abs(a_d - m_d), 0.0)
    off = (err > m_r) | (np.isfinite(a_d) != fin)
    fail(np.nonzero(both & off.any(1))[0], "a stored distance is outside the radius" if not case.exact else "distance bits differ")
    ins = both[:, None] & fin & (m_r > 0.0)
    ratio = float((err[ins] / m_r[ins]).max()) if ins.any() else 0.0
    # ---- flagged rows: sorted (above), unique, every id from row U partners, every distance that of its id ----
    for t in np.nonzero(~clear)[0]:
        row = gi[t][gi[t] >= 0]
        if len(set(row.tolist())) != len(row) or not np.all(gi[t][:len(row)] >= 0):
            fail([t], "ids not unique / not packed")
            continue
        before = {int(i): float(d) for i, d in zip(s0[0][t], s0[1][t]) if i >= 0}
        partners = set(DR.row_partners(res, n, t).tolist())
        fresh = np.array([i for i in row.tolist() if i not in before], np.int64)
        if not set(fresh.tolist()) <= partners:
            fail([t], "an id that no proposal carried")
            continue
        if any(g64[t, j] != before[int(i)] for j, i in enumerate(row.tolist()) if int(i) in before):
            fail([t], "a surviving entry changed its distance")
            continue
        if len(fresh):
            mid, rad = prep.block(np.array([[t]]), fresh[None, :])
            mid = np.where(fresh == t, prep.self_mid[t], mid[0, 0])
            rad = np.where(fresh == t, prep.self_rad[t], rad[0, 0])
            gdt = np.array([g64[t, j] for j, i in enumerate(row.tolist()) if int(i) not in before])
            if not np.all(np.abs(gdt - mid) <= rad):
                fail([t], "a distance is not that of its id")
    assert not bad, "%s: rows differ from the model, first %d:\n%s" % (label, len(bad), "\n".join(
        why + ": " + _describe(t, n, s0, res, got) for t, why in list(bad.items())[:6]))
    return ratio


@pytest.mark.parametrize("name", sorted(DC.ALL))
def test_descent_iteration_equals_the_model(name):
    """Iterations 0 (all new, every row dirty), 1, 2 and a late one (few dirty rows: descent_cases.iters) of one builder per case."""
    case = DC.ALL[name]
    cap = DC.LATTICE_CAP if case.exact else DC.FLOAT_CAP
    prep = DR.Prepared(DC.data(case), case.metric, case.exact)
    n = case.n
    b = _builder(case)
    try:
        for it in range(max(DC.iters(case)) + 1):
            if it not in DC.iters(case):
                b.descent_iter()
                continue
            s0 = b.graph()
            c = b.descent_iter()
            new, old = b.candidates()
            got = b.graph()
            st = b.stats(raw=True)
            res = DR.reference_iter(prep, case.metric, s0[0], s0[1], s0[2], new, old, case.k, DC.rng_state(case), it,
                                    case.join_blocks, exact=case.exact)
            label = "%s iteration %d" % (name, it)
            share = float((res.ambiguous != 0).mean())
            counters = (int(c), int(st.proposals[it]), int(st.join_pairs[it]))
            print("%s (%s): %.2f %% of %d rows ambiguous, %d unclear decisions; c / proposals / pairs gpu %s model %s; %d active vertices" % (
                label, case.doc, 100 * share, n, res.n_unclear, counters, (res.c, res.proposals, res.join_pairs), int((new[:, 0] >= 0).sum())))
            ratio = _check(label, case, prep, s0, got, res)
            print("%s: max |err| / radius %.3f" % (label, ratio))
            assert share <= cap, "%s: %.2f %% of the rows are ambiguous, the cap is %.0f %%" % (label, 100 * share, 100 * cap)
            slack = 0 if case.exact else res.n_unclear
            assert counters[2] == res.join_pairs, label
            assert abs(counters[0] - res.c) <= slack and abs(counters[1] - res.proposals) <= slack, (label, counters, res.c, res.proposals)
            assert int(st.updates[it]) == counters[0]
    finally:
        b.close()


@pytest.mark.parametrize("name", sorted(n for n, c in DC.LATTICE.items() if c.join_blocks == 1))
def test_join_alone_counts_the_models_proposals(name):
    """descent_sample + descent_join only, on the lattice, from the all-new state and after one iteration: the join's own
    counters must be the model's, which places a failure of the test above in the join or in the merge."""
    case = DC.ALL[name]
    prep = DR.Prepared(DC.data(case), case.metric, True)
    for stage in (0, 1):
        b = _builder(case)
        try:
            for _ in range(stage):
                b.descent_iter()
            s0 = b.graph()
            b.descent_sample()
            new, old = b.candidates()
            b.descent_join()
            st = b.stats(raw=True)
            it = int(st.n_iters_run)
            assert it == stage
            res = DR.reference_iter(prep, case.metric, s0[0], s0[1], s0[2], new, old, case.k, DC.rng_state(case), it, 1, exact=True)
            got = (int(st.proposals[it]), int(st.join_pairs[it]))
            print("%s join of iteration %d: proposals / pairs gpu %s model %s" % (name, it, got, (res.proposals, res.join_pairs)))
            assert got == (res.proposals, res.join_pairs)
        finally:
            b.close()
