"""A step-exact restatement of leaf seeding (csrc/leaf_join.hip with the merges of csrc/merge.h) in float64 numpy: test
infrastructure, in the style of tests/descent_reference.py, whose ``Prepared`` supplies the prepared rows, the Gram-form
distance with its a-priori float32 radius and the FLT_MAX conventions.

What is restated, and from where:
  * the work list.  nnd_launch_leaf_init_array (leaf_join.hip :829-886): a row of the leaf array ends at its first negative
    entry (:840); an id >= n and an id twice in one leaf are errors with the messages of :841 and :848; a leaf of fewer than two
    points is skipped BEFORE it touches the round bookkeeping (:844); the round of a leaf is the first round after the last one
    that used any of its points (:845-851); the leaf is cut into runs of LEAF_MAX = 256 consecutive positions and a run of one
    point is dropped (:852-857) -- pairs across two runs of one leaf are never evaluated.  nnd_launch_leaf_init (:778-818), the
    library's own forest, cuts the same way when a leaf is longer than 256 (the kernels drop a run of one point themselves,
    ``m < 2``) and takes one round per tree; its members come in the order of ``perm``, which is the order of
    Builder.leaf_array() (rpforest.hip k_fill_leaf_array), so ``work_list(b.leaf_array())`` is its work list too.
  * the pairs.  One workgroup (k_leaf_join, k_leaf_join_sym) or one workgroup per block of 64 rows (k_leaf_join_rb) per run:
    every member p is offered (q, d(p, q)) for every other member q of the run (``c != i``: self is never a candidate), d the
    Gram form on the prepared rows (metric.h nnd_gram_to_dist; the quarter-wave forms take the squared norms from the diagonal
    of the same Gram block, which stays inside the same radius).
  * the merges (merge.h nnd_merge_row_regs :43-181, nnd_merge_rows_q16b :357-447, nnd_merge_rows_q32b :485-576,
    nnd_merge_row_lds :589-674): a candidate enters iff d < worst(row) STRICTLY, on the distance alone, and its id is not in the
    row; the row becomes the k smallest (dist, id) keys of row U entered candidates, ascending, packed to the front; entered
    candidates carry the new flag, survivors keep theirs; unfilled slots are (empty, +inf).  The register and LDS forms test
    against the worst distance at the start of the row's merge, the queue forms against a threshold that tightens batch by
    batch, rounds run launch after launch -- none of which shows in the result, EXCEPT at a tie (below).

The final rows are therefore a function of the work list alone: per point the k smallest keys over row-before U all
run-mates of all rounds.  Every distance strictly below the k-th smallest distance D of that union always enters (a
threshold is the k-th smallest distance of a SUBSET of the union, so it is never below D); the remaining places go to
entries AT distance D, and if the union holds more of those than places are left, which of them stay depends on the order
of batches, rounds and lanes.  That is the one ambiguity:
  * R_TIE: the k-th and the (k+1)-th smallest distances of the union are equal (exact values: the lattice, stored distances of
    the rows before, FLT_MAX);
  * R_BOUNDARY: the largest upper end (mid + radius) of the k kept entries reaches the smallest lower end of a dropped one and
    one of the two is inexact.
Rows that come in (``before``) carry the kernel's own float32 distances: radius 0, flags as stored.  A run-mate that is in the
row before is the row's entry, not a candidate.

Counters (run_leaf_rounds zeroes them once per call; leaf_join.hip :369-373, :528-534, :695-698): leaf_pairs = sum m (m - 1) / 2
and leaf_rows = sum m over the runs; leaf_mfma = sum tiles(m) * (dp / 4) with dp = d rounded up to 32 and nt = ceil(m / 16) tile
rows: nt (nt + 1) / 2 for the forms that compute the upper triangle (k_leaf_join with the whole block in LDS, k_leaf_join_sym),
nt * nt for k_leaf_join_rb (its row blocks add trows * nt each and the trows of a leaf's blocks add up to nt).  ``forms(k,
longest)`` restates the table of csrc/leaf_plan.h (nnd_leaf_plan), by which run_leaf_rounds launches: tests/test_leaf_plan_cpu.py
compares the two over every (k, longest); the longest run of the whole call selects the launches of every round.
"""
from collections import namedtuple

import numpy as np

from tests.descent_reference import Prepared

LEAF_MAX = 256
R_TIE, R_BOUNDARY = 1, 2
REASONS = {R_TIE: "equal distances at the k-th place", R_BOUNDARY: "k-th place inside the radius"}

WorkList = namedtuple("WorkList", [
    "pieces",      # list of int64 arrays: the members of every run, in work-list order (round by round)
    "rounds",      # (n_pieces,) the round of every run
    "leaves",      # (n_pieces,) the leaf-array row every run was cut from
    "n_rounds", "longest",
])
Form = namedtuple("Form", ["name", "tiles", "m_lo", "m_hi"])  # tiles: "tri" | "full"; takes the runs with m_lo < m <= m_hi
LeafResult = namedtuple("LeafResult", [
    "ids", "dists", "radius", "flags",  # (n, k): rows ascending by (d, id); unfilled -1 / inf / 0 / 0
    "ambiguous",                        # (n,) uint8: bit set of R_* reasons
    "n_union",                          # (n,) entries of row-before U run-mates
    "possible", "p_mid", "p_rad",       # sorted int64 codes p * n + q of every (point, run-mate) pair, with its distance
    "leaf_pairs", "leaf_rows", "leaf_mfma", "forms", "work",
])


class LeafArrayError(ValueError):
    """the two error returns of nnd_launch_leaf_init_array, with the message the code sets."""


def reason_text(bits):
    return ", ".join(t for b, t in REASONS.items() if bits & b) or "clear"


# ------------------------------------------------------------------------------------------------ the work list
def work_list(leaf_array, n):
    la = np.asarray(leaf_array, np.int64)
    assert la.ndim == 2
    seen = np.zeros(n, np.int64)
    pieces, rounds, leaves = [], [], []
    n_rounds = longest = 0
    for l, row in enumerate(la):
        neg = np.nonzero(row < 0)[0]
        mem = row[:neg[0]] if len(neg) else row
        if (mem >= n).any():
            raise LeafArrayError("nnd_init_from_leaf_array: leaf %d holds point %d but n = %d" % (l, int(mem[mem >= n][0]), n))
        if len(mem) < 2:
            continue
        r = int(seen[mem].max())
        for p in mem:  # in member order: the second occurrence is the one reported
            if seen[p] == r + 1:
                raise LeafArrayError("nnd_init_from_leaf_array: point %d occurs twice in leaf %d" % (int(p), l))
            seen[p] = r + 1
        n_rounds = max(n_rounds, r + 1)
        for a in range(0, len(mem), LEAF_MAX):
            piece = mem[a:a + LEAF_MAX]
            if len(piece) < 2:
                continue
            pieces.append(piece)
            rounds.append(r)
            leaves.append(l)
            longest = max(longest, len(piece))
    o = np.argsort(np.asarray(rounds, np.int64), kind="stable")  # the counting sort by round
    return WorkList([pieces[i] for i in o], np.asarray(rounds, np.int64)[o], np.asarray(leaves, np.int64)[o], n_rounds, longest)


# ------------------------------------------------------------------------------------------------ the dispatch table
def forms(k, longest):
    """The launches of one round (csrc/leaf_plan.h nnd_leaf_plan) for rows of k neighbours when the longest run has ``longest``
    points.  The names are the kernels' without their first template argument, the metric family (metric.h nnd_metric_family):
    a form has one instance for the boolean metrics and one for all others, and the table is the same for both."""
    if k > 64:
        nt = 8 if longest <= 128 else (10 if longest <= 160 else 16)
        return [Form("k_leaf_join_rb<%d,8,true>" % nt, "full", 0, nt * 16)]
    qw = k <= 16
    if not qw and k <= 32 and longest <= 160:
        out = [Form("k_leaf_join_sym<6,8>", "tri", 0, 96)]
        if longest > 96:
            out.append(Form("k_leaf_join_sym<10,8>", "tri", 96, 160))
        return out
    if longest <= 64:
        return [Form("k_leaf_join<4,8,64%s>" % (",true" if qw else ""), "tri", 0, 64)]
    if longest <= 80 and qw:
        return [Form("k_leaf_join<4,4,64,true>", "tri", 0, 64), Form("k_leaf_join<5,8,64,true>", "tri", 64, 80)]
    if longest <= 80:
        return [Form("k_leaf_join<5,8,64>", "tri", 0, 80)]
    if longest <= 96:
        return [Form("k_leaf_join<6,8,64%s>" % (",true" if qw else ""), "tri", 0, 96)]
    nt = 8 if longest <= 128 else (10 if longest <= 160 else 16)
    return [Form("k_leaf_join_rb<%d,8>" % nt, "full", 0, nt * 16)]


def counters(lengths, k, d, longest=None):
    """(leaf_pairs, leaf_rows, leaf_mfma, forms) of one call for runs of the given lengths.  ``longest``: what the dispatch is
    handed where that is not the longest run (the library's own forest hands it max(leaf_size, longest leaf) unless it cuts)."""
    m = np.asarray(lengths, np.int64)
    m = m[m >= 2]
    fs = forms(k, int(m.max()) if longest is None else int(longest)) if len(m) else []
    nt = (m + 15) >> 4
    steps = ((d + 31) & ~31) >> 2
    mfma, taken = 0, np.zeros(len(m), np.int64)
    for f in fs:
        sel = (m > f.m_lo) & (m <= f.m_hi)
        taken += sel
        mfma += int(((nt * (nt + 1) // 2 if f.tiles == "tri" else nt * nt)[sel]).sum()) * steps
    assert (taken == 1).all(), "every run belongs to exactly one launch of its round"
    return int((m * (m - 1) // 2).sum()), int(m.sum()), mfma, fs


# ------------------------------------------------------------------------------------------------ the seeding
def reference_seed(data, metric, k, leaf_array, before=None, *, exact=False, longest=None):
    """Leaf seeding of ``leaf_array`` (int32 (n_leaves, width), -1 padded) into rows that hold ``before`` = (ids, dists, flags)
    as Builder.graph() returns them (None: empty rows).  Returns a LeafResult; raises LeafArrayError where the library does."""
    prep = data if isinstance(data, Prepared) else Prepared(data, metric, exact)
    n, k = prep.n, int(k)
    work = work_list(leaf_array, n)
    lens = np.array([len(p) for p in work.pieces], np.int64)
    pairs, rows, mfma, fs = counters(lens, k, prep.d, longest)

    # ---- every (point, run-mate) pair of every run, one m x m block per run (runs of one length in one call) ----
    P, Q, M, R = [], [], [], []
    for m in np.unique(lens):
        grp = np.stack([work.pieces[i] for i in np.nonzero(lens == m)[0]])
        for s in range(0, len(grp), max(1, 2_000_000 // int(m * m))):
            g = grp[s:s + max(1, 2_000_000 // int(m * m))]
            mid, rad = prep.block(g, g)
            off = ~np.eye(int(m), dtype=bool)[None].repeat(len(g), 0)
            P.append(np.broadcast_to(g[:, :, None], mid.shape)[off])
            Q.append(np.broadcast_to(g[:, None, :], mid.shape)[off])
            M.append(mid[off])
            R.append(rad[off])
    if P:
        P, Q, M, R = (np.concatenate(a) for a in (P, Q, M, R))
        code, first = np.unique(P * n + Q, return_index=True)  # a pair met in several rounds carries one value
        M, R = M[first], R[first]
    else:
        code, M, R = np.zeros(0, np.int64), np.zeros(0), np.zeros(0)
    possible, p_mid, p_rad = code, M, R

    # ---- the union per point: the row before first (its entries are not candidates again), then the mates ----
    F = np.ones(len(code), np.uint8)
    if before is not None:
        b_id, b_d, b_f = (np.asarray(a) for a in before)
        assert b_id.shape == (n, k)
        on = b_id >= 0
        b_code = (np.arange(n, dtype=np.int64)[:, None] * n + b_id)[on]
        keep = ~np.isin(code, b_code)
        # an entry of the row before that is a run-mate too keeps its stored value, but if the merges push it out it is offered
        # again at its Gram-form value: at the k-th place it is as inexact as that
        at = np.minimum(np.searchsorted(code, b_code), max(len(code) - 1, 0))
        b_rad = np.where(code[at] == b_code, R[at], 0.0) if len(code) else np.zeros(len(b_code))
        code = np.concatenate([b_code, code[keep]])
        M = np.concatenate([b_d[on].astype(np.float32).astype(np.float64), M[keep]])
        R = np.concatenate([b_rad, R[keep]])
        F = np.concatenate([b_f[on].astype(np.uint8), F[keep]])
    T, S = code // n, code % n
    o = np.lexsort((S, M, T))  # by point, then by (d, id)
    T, S, M, R, F = T[o], S[o], M[o], R[o], F[o]
    cnt = np.bincount(T, minlength=n)
    start = np.cumsum(cnt) - cnt
    pos = np.arange(len(T)) - start[T]
    kept = pos < k
    ids = np.full((n, k), -1, np.int64)
    d_mid = np.full((n, k), np.inf)
    d_rad = np.zeros((n, k))
    flags = np.zeros((n, k), np.uint8)
    ids[T[kept], pos[kept]], d_mid[T[kept], pos[kept]], d_rad[T[kept], pos[kept]], flags[T[kept], pos[kept]] = S[kept], M[kept], R[kept], F[kept]

    # ---- the k-th place ----
    amb = np.zeros(n, np.uint8)
    drop = ~kept
    if drop.any():
        def seg(op, init, sel, val):
            out = np.full(n, init)
            op.at(out, T[sel], val[sel])
            return out
        mid_k, mid_d = seg(np.maximum, -np.inf, kept, M), seg(np.minimum, np.inf, drop, M)
        amb[mid_k == mid_d] |= R_TIE
        hi, lo, inexact = M + R, M - R, R > 0.0
        for k_sel, d_sel in ((kept, drop & inexact), (kept & inexact, drop)):
            un = seg(np.maximum, -np.inf, k_sel, hi) >= seg(np.minimum, np.inf, d_sel, lo)
            amb[un] |= R_BOUNDARY
    return LeafResult(ids.astype(np.int32), d_mid, d_rad, flags, amb, cnt, possible, p_mid, p_rad, pairs, rows, mfma, fs, work)


def row_mates(res, n, t):
    """(ids, mid, radius) of every run-mate of point t over all rounds (ascending ids)."""
    lo, hi = np.searchsorted(res.possible, [t * n, (t + 1) * n])
    return res.possible[lo:hi] - t * n, res.p_mid[lo:hi], res.p_rad[lo:hi]


def row_leaves(res, t):
    """[(leaf-array row, round, run length)] of the runs that hold point t."""
    w = res.work
    return [(int(w.leaves[i]), int(w.rounds[i]), len(p)) for i, p in enumerate(w.pieces) if (p == t).any()]
