"""The host model of one NN-descent iteration (tests/descent_reference.py) pinned without a GPU: against the oracle's
checked_flagged_heap_push (bit-exact to reference utils.py:471-533) applied to the same proposals, against a scalar, pair by
pair restatement of the join and its slots, and the ambiguity caps of every case of tests/descent_cases.py on states the
reference algorithm produces.  A wrong model fails HERE, not on the GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import descent_cases as DC
from tests import descent_reference as DR
from tests.search_reference import hash2, searcher_seed

SMALL = DC.Case("lattice_small", "euclidean", 15, 15, 2002, 16, 2, 1, 0, True, 1, "the scalar restatement's case")
SMALL_FLOAT = DC.Case("float_small", "euclidean", 15, 15, 2001, 24, 2, 1, 0, False, 1, "the sequential-push pin's float case")


@pytest.fixture(scope="module")
def states():
    """(case, state after the reference's initialisation, state after the model's first iteration on it) per small case."""
    out = {}
    for case in (SMALL, SMALL_FLOAT):
        s0 = DC.cpu_state(case)
        r0 = _run(case, s0, 0)
        idx1, d1, f1 = r0.ids, r0.dists.astype(np.float32), r0.flags
        s1 = (idx1, d1, f1) + DC.candidates_cpu(case, idx1, f1)  # a mix of new and old entries, old lists in use
        out[case.name] = (case, s0, s1)
    return out


def _run(case, state, it, x=None, **kw):
    idx0, dist0, fl0, new, old = state
    return DR.reference_iter(DC.data(case) if x is None else x, case.metric, idx0, dist0, fl0, new, old, case.k, DC.rng_state(case), it,
                             kw.pop("join_blocks", case.join_blocks), exact=case.exact, **kw)


def _scalar_iteration(case, state, it, slots):
    """The join and the slots one pair at a time, in plain Python on difference-form float64 distances (exact on the lattice):
    {target: {slot or source: (d, source)}}, the proposal count and the pair count."""
    idx0, dist0, fl0, new, old = state
    x = DC.data(case).astype(np.float64)
    n, k = idx0.shape
    th = np.where(idx0[:, k - 1] >= 0, dist0[:, k - 1].astype(np.float64), np.inf)
    rows = [set(r[r >= 0].tolist()) for r in idx0]
    seed = hash2(searcher_seed(DC.rng_state(case)) ^ 0x2545F491, it)
    table, proposals, pairs = {}, 0, 0

    def propose(t, s, d):
        nonlocal proposals
        if d < th[t] and s not in rows[t]:
            proposals += 1
            bank = table.setdefault(t, {})
            key = (hash2(seed, s) & 63) if slots else s
            if key not in bank or (d, s) < bank[key]:
                bank[key] = (d, s)

    for v in range(n):
        nv, ov = new[v][new[v] >= 0].tolist(), old[v][old[v] >= 0].tolist()
        for i, p in enumerate(nv):
            for q in nv[i:] + ov:
                pairs += 1
                if p == q:
                    propose(p, p, 0.0)
                    continue
                d = float(((x[p] - x[q]) ** 2).sum())
                propose(p, q, d)
                propose(q, p, d)
    return table, proposals, pairs


@pytest.mark.parametrize("slots", [64, None])
@pytest.mark.parametrize("stage", [0, 1])
def test_model_equals_the_pair_by_pair_restatement(states, stage, slots):
    """ids, distances, flags and all three counters of the vectorised model against a scalar join + top-k by brute force, on the
    lattice (every comparison exact), from an all-new state and from a mixed one, with the 64 hashed slots and without."""
    case, s0, s1 = states["lattice_small"]
    state = (s0, s1)[stage]
    res = _run(case, state, stage, slots=slots)
    table, proposals, pairs = _scalar_iteration(case, state, stage, slots)
    assert (res.proposals, res.join_pairs) == (proposals, pairs)
    assert res.c == sum(len(b) for b in table.values()) and not res.ambiguous.any()
    idx0, dist0, fl0, new, _ = state
    fl_s = DR.post_sampling_flags(idx0, fl0, new)
    for t in range(idx0.shape[0]):
        have = [(float(dist0[t, j]), int(idx0[t, j]), int(fl_s[t, j])) for j in range(case.k) if idx0[t, j] >= 0]
        want = sorted(have + [(d, s, 1) for d, s in table.get(t, {}).values()])[:case.k]
        m = len(want)
        assert res.ids[t, :m].tolist() == [w[1] for w in want] and (res.ids[t, m:] == -1).all(), t
        assert res.dists[t, :m].tolist() == [w[0] for w in want] and res.flags[t, :m].tolist() == [w[2] for w in want], t
    if stage == 1:
        assert (state[4][:, 0] >= 0).any()  # the old lists took part


@pytest.mark.parametrize("name", ["lattice_small", "float_small"])
@pytest.mark.parametrize("stage", [0, 1])
def test_model_without_slots_equals_sequential_checked_heap_pushes(states, name, stage):
    """slots=None, one sub-step: a row of the model must hold the ids that checked_flagged_heap_push leaves when the same
    partners are pushed one by one into the same row -- in ascending and in descending id order.  Rows where the model reports
    equal distances on both sides of the k-th place depend on the push order and are exempt, as are the float rows it
    flags; both are counted."""
    lib = O.load("strict")
    case, s0, s1 = states[name]
    state = (s0, s1)[stage]
    idx0, dist0, fl0, new, old = state
    res = _run(case, state, stage, slots=None)
    prep = DR.Prepared(DC.data(case), case.metric, case.exact)
    n, k = idx0.shape
    exempt = res.tie | (res.ambiguous != 0)
    checked = quiet = 0
    for t in range(n):
        if res.ambiguous[t]:
            continue
        partners = DR.row_partners(res, n, t)
        if len(partners) == 0:
            assert np.array_equal(res.ids[t], idx0[t])
            quiet += 1
            continue
        mid, _ = prep.block(np.array([[t]]), partners[None, :])
        d = np.where(partners == t, prep.self_mid[t], mid[0, 0]).astype(np.float32)
        # what the model lets through would be pushed: strictly below the row's worst distance, not in the row (utils.py:484-492)
        # -- asserted on the tie rows too, where a proposal AT the threshold would otherwise hide behind the exemption
        worst = dist0[t, k - 1] if idx0[t, k - 1] >= 0 else np.float32(np.inf)
        assert np.all(d < worst) and not set(partners.tolist()) & set(idx0[t].tolist()), (t, worst, d.tolist())
        if exempt[t]:
            continue
        for order in (np.arange(len(partners)), np.arange(len(partners))[::-1]):
            hi = np.ascontiguousarray(idx0[t][::-1])   # descending distances: a valid max-heap, unfilled (-1, inf) first
            hd = np.ascontiguousarray(dist0[t][::-1])
            hf = np.zeros(k, np.uint8)
            for j in order:
                lib.orc_checked_flagged_heap_push(hd, hi, hf, k, float(d[j]), int(partners[j]), 1)
            assert set(hi[hi >= 0].tolist()) == set(res.ids[t][res.ids[t] >= 0].tolist()), (t, partners.tolist())
        checked += 1
    print("%s stage %d: %d rows pinned, %d without a proposal, %d exempt (%d ties at the k-th place)" % (
        name, stage, checked, quiet, int(exempt.sum()), int(res.tie.sum())))
    assert checked > 200 and checked + quiet > n // 4


def test_slot_collisions_are_modelled_and_the_farther_key_loses(states):
    """With 64 slots a first iteration loses proposals: every loser's (d, source) key is larger than the winner's of its slot, no
    loser is inserted by that slot, and c counts the winners only."""
    case, s0, _ = states["lattice_small"]
    res, free = _run(case, s0, 0), _run(case, s0, 0, slots=None)
    assert len(res.lost) > 0 and res.c + len(res.lost) == free.c and res.proposals == free.proposals
    t, ws, wd, ls, ld = res.lost.T
    assert np.all((wd < ld) | ((wd == ld) & (ws < ls)))
    seed = hash2(searcher_seed(DC.rng_state(case)) ^ 0x2545F491, 0)
    assert all((hash2(seed, int(a)) & 63) == (hash2(seed, int(b)) & 63) for a, b in zip(ws[:200], ls[:200]))
    lost_rows = np.unique(t.astype(np.int64))
    differ = sum(set(res.ids[r].tolist()) != set(free.ids[r].tolist()) for r in lost_rows)
    print("%d proposals lost in %d rows, %d rows end differently" % (len(res.lost), len(lost_rows), differ))
    assert differ > 0


def test_sub_steps_refresh_thresholds_and_ids():
    """join_blocks = 3 on a state without a forest: the second sub-step sees the rows the first one merged (fewer proposals
    pass than against the first snapshot), and one sub-step of the whole range is the plain iteration."""
    case = DC.Case("blocks_small", "euclidean", 15, 15, 2002, 16, 0, 3, 0, True, 1, "")
    x = DC.lattice_points(case.n)
    state = DC.cpu_state(case, x)
    one, three = _run(case, state, 0, x, join_blocks=1), _run(case, state, 0, x)
    assert one.join_pairs == three.join_pairs and three.proposals < one.proposals
    assert not np.array_equal(one.ids, three.ids)


def test_a_proposal_exactly_at_the_threshold_is_refused():
    """The test is d < th, strictly.  Six points on two axes, k = 2, every row its own point and one more; vertex 0 joins the
    new candidates 0 = (1, 0) and 4 = (3, 0), 4 apart.  Row 0 ends at distance 4: nothing may be proposed.  With row 0 ending
    at 16 instead, 4 is proposed and takes the second place."""
    x = np.array([[1, 0], [-1, 0], [0, 1], [0, -1], [3, 0], [-3, 0]], np.float32)
    new = np.full((6, 2), -1, np.int32)
    new[0] = [0, 4]
    old = np.full((6, 2), -1, np.int32)
    idx0 = np.array([[0, 1], [1, 0], [2, 3], [3, 2], [4, 0], [5, 1]], np.int32)
    dist0 = np.array([[0, 4]] * 6, np.float32)
    fl0 = np.zeros((6, 2), np.uint8)

    def run():
        return DR.reference_iter(x, "euclidean", idx0, dist0, fl0, new, old, 2, DC.rng_state(SMALL), 0, 1, exact=True)
    res = run()
    assert res.join_pairs == 3 and (res.proposals, res.c) == (0, 0) and not res.ambiguous.any()
    assert np.array_equal(res.ids, idx0) and np.array_equal(res.dists, dist0)
    idx0[0, 1], dist0[0, 1] = 5, 16.0
    res = run()
    assert (res.proposals, res.c) == (1, 1) and res.ids[0].tolist() == [0, 4] and res.dists[0].tolist() == [0.0, 4.0]
    assert res.flags[0].tolist() == [0, 1] and np.array_equal(res.ids[1:], idx0[1:])


@pytest.mark.parametrize("name", sorted(DC.ALL))
def test_case_stays_inside_its_ambiguity_cap(name):
    """Every case on the reference algorithm's own first state (init_rp_tree + init_random, new_build_candidates): at most
    10 % of the rows ambiguous on float data, none on the lattice."""
    case = DC.ALL[name]
    res = _run(case, DC.cpu_state(case), 0)
    share = float((res.ambiguous != 0).mean())
    print("%s: %.2f %% of %d rows ambiguous (%s), c = %d, %d proposals, %d lost to collisions" % (
        name, 100 * share, case.n, np.bincount(res.ambiguous, minlength=8).tolist(), res.c, res.proposals, len(res.lost)))
    assert res.c > 0 and res.proposals >= res.c
    assert share <= (DC.LATTICE_CAP if case.exact else DC.FLOAT_CAP)
