"""A step-exact restatement of one NN-descent iteration (local join + proposal merge) in float64 numpy: test infrastructure.

What is restated, and from where:
  * csrc/capi.hip descent_iter: ``join_blocks`` sub-steps, sub-step b joins the vertices [n b / nb, n (b + 1) / nb)
    of the visiting order and is followed by a merge of EVERY row that has pending proposals; counters are zeroed once per
    iteration and read at its end.  The visiting order is the first tree's, so sub-steps are modelled for builders without a
    forest only (position = id).
  * csrc/join.hip (k_local_join16 :232-362, k_local_join_w :700-824, launch_join_blocked :918-925): a vertex joins iff its new
    list is not empty (slot 0 tells: lists are filled from the front).  Pairs go BY SLOT: new slot i against new slots
    jj >= i (the self pair included) and against every old slot (:334, :794).  A pair of equal ids takes nnd_self_dist and
    proposes to p only (:336-341, :796-798).  Endpoint t takes source s iff d < th[t] strictly, th being the row's k-th stored
    distance (+inf while the row is not full), and s is not among the row's ids (klist_has / list_has / list_has_lds).  The
    join writes nothing to the k-lists: it reads a snapshot.
  * the proposal slots (:294-313, :674-683, launch_join16_t :422): slot = hash2(hash2(seed ^ 0x2545F491, iter), s) & 63 of the
    SOURCE, 64-bit atomicMin on (dist_bits << 32 | s): per (target, slot) the smallest (d, s) stays.
  * csrc/merge.hip k_merge / k_merge_q / k_merge_wide with csrc/merge.h nnd_merge_row_regs (:43-181), nnd_merge_rows_q16_regs
    (:216-278), nnd_merge_row_lds (:589-674): row' = the k smallest (d, id) keys of row U slot winners; inserted entries carry
    the new flag, survivors keep theirs (the flag the sampling left: tests/test_gpu_kernels.py test_sample_candidates).
  * counters: CNT_PROPOSALS (join.hip :303, :314, :677, :682) counts every (pair, endpoint) whose push would succeed on the
    snapshot, repeats of one (target, source) from different vertices included.  CNT_ACCEPT -- the iteration's ``c`` -- is what
    the merges RETURN (merge.h :103/:180 ``pushed``, :247, :673 ``nv``): the slot winners that beat the row's worst distance as
    the merge found it and were not in the row, i.e. the pushes that succeed on the snapshot AFTER slot collisions, also those
    that a nearer winner of the same merge then pushes beyond the k-th place.  It is not the number of entries that end up in a
    list.

Arithmetic.  The kernels evaluate a Gram form on the PREPARED rows (csrc/prep.hip): sqeuclidean rows centred on the column mean
(the mean of all rows while n < 65536) and |a|^2 + |b|^2 - 2 <a, b> over dp = d rounded up to 4 terms; unit rows and the
metric's conversion for cosine / dot / correlation / hellinger; raw rows and 1 / <a, b> for inner product.  The model evaluates
the same form in float64 and attaches an a-priori float32 radius to every value, never a measured one:
  * sqeuclidean: (dp + 8) 2^-24 (|a| + |b|)^2.  dp u |a|^2 and dp u |b|^2 for the two norms, 2 dp u |a||b| for the Gram value
    (u = 2^-24; any summation order), 4 u (|a| + |b|)^2 for the three roundings of the combination, and the rounding of the
    centred rows themselves (|fl(x - m) - (x - m)| <= u |x - m| per component, which moves the distance by at most
    2 u (|a| + |b|) |a - b| <= 2 u (|a| + |b|)^2; an error of the mean itself is a translation and moves nothing).
  * the others: gamma = (dp + 4) 2^-24 times sum |a_i b_i| on the Gram value, the same gamma relative for the two
    normalisations, carried through the monotone conversion by evaluating it at both ends, plus 4 float32 ulps of the result
    (tests/search_reference.py _Distances, the same rule).
  * exact=True (the lattice): integer coordinates, the point set closed under negation (column mean exactly 0) and
    dp (2R)^2 < 2^24 -- every partial sum of every summation order is an exact integer: radius 0, nothing is ambiguous.
Stored distances of the rows that come in (``dist0``) are the kernel's own float32 values: radius 0.

Ambiguity (narrow on purpose).  A ROW is ambiguous iff one of ITS OWN decisions was taken on overlapping intervals: a
d < th test of a proposal to it, a collision of two different sources in one of its slots, the keys on either side of its
k-th place after a merge.  The order of the neighbours inside a row is not a decision.
"""
from collections import namedtuple

import numpy as np

from tests.gpu_util import self_dist
from tests.search_reference import FLT_MAX, METRIC_CODE, U24, _ulp32, _unit_rows, hash2, searcher_seed

METRIC_NAME = {0: "euclidean", 1: "cosine", 2: "dot", 3: "inner_product", 4: "correlation", 5: "hellinger"}
R_THRESHOLD, R_COLLISION, R_BOUNDARY = 1, 2, 4
REASONS = {R_THRESHOLD: "d vs threshold", R_COLLISION: "slot collision", R_BOUNDARY: "k-th place"}

IterResult = namedtuple("IterResult", [
    "ids", "dists", "radius", "flags",      # (n, k): the rows after the iteration, ascending by (d, id); unfilled -1 / inf / 0 / 0
    "ambiguous",                            # (n,) uint8: bit set of R_* reasons, 0 = every decision of the row was clear
    "c", "proposals", "join_pairs",         # the counters as the code defines them
    "n_unclear",                            # decisions taken on overlapping intervals (bounds the counters' deviation)
    "possible",                             # sorted int64 codes target * n + source: every source that MAY have reached target
    "lost",                                 # (target, winner source, winner d, loser source, loser d) of every slot collision
    "tie",                                  # (n,) bool: equal distances on both sides of the k-th place in a merge (sequential
                                            # pushes of the same proposals depend on their order there; the kernels do not)
])


def reason_text(bits):
    return ", ".join(t for b, t in REASONS.items() if bits & b) or "clear"


# ------------------------------------------------------------------------------------------------ distances
class Prepared:
    """The prepared rows of csrc/prep.hip in float64 and the Gram-form distance of join.hip with its a-priori radius."""

    def __init__(self, data, metric, exact=False):
        self.code = METRIC_CODE[metric] if isinstance(metric, str) else int(metric)
        self.exact = exact
        x = np.asarray(data, np.float32).astype(np.float64)
        self.n, self.d = x.shape
        assert self.n < 65536, "the column mean is the mean of ALL rows only below 65536 rows (prep.hip NND_MEAN_ROWS)"
        dp = (self.d + 3) & ~3
        self.g_euclid = 0.0 if exact else (dp + 8) * U24
        self.gamma = 0.0 if exact else (dp + 4) * U24
        m = self.code
        if m == 0:
            self.rows = x - x.mean(0)
            if exact:
                assert not self.rows.any() or np.array_equal(self.rows, x), "lattice: the column mean must be exactly 0"
            self.nrm = (self.rows * self.rows).sum(1)
            self.nz = self.nrm > 0.0
        elif m == 3:
            self.rows = x
            self.nrm = (x * x).sum(1)
            self.nz = self.nrm > 0.0
        else:
            t = x if m in (1, 2) else (x - x.mean(1, keepdims=True) if m == 4 else np.sqrt(x))
            self.rows, self.nz = _unit_rows(t)
            self.nrm = self.nz.astype(np.float64)
        self.len = np.sqrt(self.nrm)
        self.absrows = None if m == 0 else np.abs(self.rows)
        # d(x, x) as the kernels set it (nnd_self_dist); inner product: 1 / |x|^2 from the float32 norm
        self.self_mid = self_dist(METRIC_NAME[m], x)
        self.self_rad = np.zeros(self.n)
        if m == 3 and not exact:
            fin = self.self_mid < FLT_MAX
            self.self_rad = np.where(fin, self.gamma * self.self_mid + 4.0 * _ulp32(self.self_mid), 0.0)

    def _finish(self, mid, lo, hi):
        if not self.exact:
            lo = np.where(lo < FLT_MAX, np.maximum(lo - 4.0 * _ulp32(lo), 0.0), lo)
            hi = np.where(hi < FLT_MAX, hi + 4.0 * _ulp32(hi), hi)
        return mid, np.maximum(hi - mid, mid - lo)

    def block(self, a_ids, b_ids):
        """(mid, radius) of the distances of rows a_ids (nv, A) to rows b_ids (nv, B): two (nv, A, B) float64 arrays."""
        m = self.code
        ra, rb = self.rows[a_ids], self.rows[b_ids]
        g = ra @ rb.transpose(0, 2, 1)
        if m == 0:
            mid = np.maximum(self.nrm[a_ids][:, :, None] + self.nrm[b_ids][:, None, :] - 2.0 * g, 0.0)
            if self.exact:
                return mid, np.zeros_like(mid)
            return mid, self.g_euclid * (self.len[a_ids][:, :, None] + self.len[b_ids][:, None, :]) ** 2
        dg = self.gamma * (self.absrows[a_ids] @ self.absrows[b_ids].transpose(0, 2, 1))
        za, zb = ~self.nz[a_ids][:, :, None], ~self.nz[b_ids][:, None, :]
        if m == 3:  # 1 / <a, b> for a positive product (nnd_gram_to_dist)
            def f(v):
                with np.errstate(divide="ignore"):
                    return np.where(v > 0.0, np.minimum(1.0 / np.where(v > 0.0, v, 1.0), FLT_MAX), FLT_MAX)
            return self._finish(f(g), f(g + dg), f(g - dg))
        dg = dg + self.gamma * np.abs(g)  # gamma / 2 relative on each of the two normalisations
        if m == 4:  # 1 - <a, b> on centred unit rows; two zero rows: 0
            mid, lo, hi = np.maximum(1.0 - g, 0.0), np.maximum(1.0 - g - dg, 0.0), np.maximum(1.0 - g + dg, 0.0)
            both = za & zb
            mid, lo, hi = np.where(both, 0.0, mid), np.where(both, 0.0, lo), np.where(both, 0.0, hi)
            return self._finish(mid, lo, hi)

        def f(v):  # cosine / dot / hellinger: -log2 <a, b> on unit rows
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(v > 0.0, np.maximum(-np.log2(np.where(v > 0.0, v, 1.0)), 0.0), FLT_MAX)
        mid, lo, hi = f(g), f(g + dg), f(g - dg)
        dead = za | zb
        mid, lo, hi = np.where(dead, FLT_MAX, mid), np.where(dead, FLT_MAX, lo), np.where(dead, FLT_MAX, hi)
        if m != 2:  # two zero rows are at distance 0 (not under dot)
            both = za & zb
            mid, lo, hi = np.where(both, 0.0, mid), np.where(both, 0.0, lo), np.where(both, 0.0, hi)
        return self._finish(mid, lo, hi)


def post_sampling_flags(idx0, fl0, new):
    """The flags the sampling leaves (utils.py:311-318, test_sample_candidates): a new forward entry that was sampled into the
    vertex's new list is old now, every other entry keeps its flag."""
    out = np.asarray(fl0, np.uint8).copy()
    n = idx0.shape[0]
    for s in range(0, n, 4096):
        i0, nw = idx0[s:s + 4096], new[s:s + 4096]
        sampled = ((i0[:, :, None] == nw[:, None, :]) & (i0[:, :, None] >= 0)).any(2)
        out[s:s + 4096][sampled] = 0
    return out


def _less(mid, rad, th, th_rad):
    """(mid < th, the two intervals overlap and are not both exact)."""
    unclear = (mid - rad < th + th_rad) & (mid + rad >= th - th_rad) & ((rad > 0.0) | (th_rad > 0.0))
    return mid < th, unclear


# ------------------------------------------------------------------------------------------------ the iteration
def reference_iter(data, metric, idx0, dist0, fl0, new, old, k, rng_state, it, join_blocks=1, *, exact=False, slots=64,
                   budget=3_000_000):
    """One nnd_descent_iter.  ``idx0, dist0, fl0``: b.graph() before the iteration; ``new, old``: b.candidates() after it (the
    lists it used); ``rng_state``: the builder's int64[3]; ``it``: the iteration's number.  ``slots=None``: no slot
    collisions, every proposal reaches the merge (the CPU pin against sequential pushes).  Returns an IterResult."""
    prep = data if isinstance(data, Prepared) else Prepared(data, metric, exact)
    n, k = prep.n, int(k)
    assert idx0.shape == (n, k) and join_blocks >= 1
    ids = np.asarray(idx0, np.int64).copy()
    d_mid = np.where(ids >= 0, np.asarray(dist0, np.float32).astype(np.float64), np.inf)
    d_rad = np.zeros((n, k))
    flags = np.where(ids >= 0, post_sampling_flags(idx0, fl0, new), 0).astype(np.uint8)
    new, old = np.asarray(new, np.int64), np.asarray(old, np.int64)
    slot_seed = hash2(searcher_seed(rng_state) ^ 0x2545F491, int(it))  # join.hip :422 (common.h nnd_seed_of = searcher_seed)
    slot_of = np.array([hash2(slot_seed, s) & 63 for s in range(n)], np.int64) if slots is not None else None
    assert slots in (None, 64)
    amb = np.zeros(n, np.uint8)
    tie = np.zeros(n, bool)
    c = proposals = join_pairs = n_unclear = 0
    possible, lost = [], []

    for b in range(join_blocks):
        v0, v1 = n * b // join_blocks, n * (b + 1) // join_blocks
        th, th_rad = d_mid[:, k - 1].copy(), d_rad[:, k - 1].copy()  # +inf while the row is not full
        member = np.zeros((n * n + 7) // 8, np.uint8)  # a bit per code target * n + id of the snapshot
        mc_ = (np.arange(n)[:, None] * n + ids)[ids >= 0]
        np.bitwise_or.at(member, mc_ >> 3, (1 << (mc_ & 7)).astype(np.uint8))
        vs = v0 + np.nonzero(new[v0:v1, 0] >= 0)[0]
        C, M, R, OK, UN = [], [], [], [], []
        # chunks of about ``budget`` pairs, the vertices with the longest new lists first: a chunk is as wide as its own
        # longest lists, so the short new lists of a late iteration do not pay for the longest one
        ext_n, ext_o = (((l[vs] >= 0) * np.arange(1, l.shape[1] + 1)).max(1) for l in (new, old))
        o = np.argsort(-ext_n, kind="stable")
        vs, ext_n, ext_o = vs[o], ext_n[o], ext_o[o]
        s1 = 0
        while s1 < len(vs):
            s0, mn = s1, int(ext_n[s1])
            s1 = s0 + max(1, budget // (mn * (mn + int(ext_o[s0:].max()))))
            v, mo = vs[s0:s1], int(ext_o[s0:s1].max())
            tri = np.arange(mn + mo)[None, :] >= np.arange(mn)[:, None]  # jj >= MCP || jj >= i
            cn, ca = new[v, :mn], np.concatenate([new[v, :mn], old[v, :mo]], 1)
            valid = (cn >= 0)[:, :, None] & (ca >= 0)[:, None, :] & tri[None]
            join_pairs += int(valid.sum())
            pn, pa = np.maximum(cn, 0), np.maximum(ca, 0)
            mid, rad = prep.block(pn, pa)
            # only the pairs that can pass a test are looked at one by one, per endpoint: p <- q on p's threshold, q <- p on
            # q's (not for equal ids, which take the self distance and propose to p only).  The filter is inclusive: the
            # strict test itself is _less alone
            up, lo = th + th_rad, mid - rad
            same3 = pn[:, :, None] == pa[:, None, :]
            for first in (True, False):
                if first:
                    m = valid & ((lo <= up[pn][:, :, None]) | same3)
                    t3, s3 = pn[:, :, None], pa[:, None, :]
                else:
                    m = valid & (lo <= up[pa][:, None, :]) & ~same3
                    t3, s3 = pa[:, None, :], pn[:, :, None]
                tgt, src = np.broadcast_to(t3, m.shape)[m], np.broadcast_to(s3, m.shape)[m]
                md, rd = mid[m], rad[m]
                if first:
                    same = tgt == src
                    md[same], rd[same] = prep.self_mid[tgt[same]], prep.self_rad[tgt[same]]
                ok, un = _less(md, rd, th[tgt], th_rad[tgt])
                cd = tgt * n + src
                keep = (member[cd >> 3] >> (cd & 7).astype(np.uint8)) & 1 == 0  # the source is not among the row's ids
                keep &= ok | un
                C.append(cd[keep]); M.append(md[keep]); R.append(rd[keep]); OK.append(ok[keep]); UN.append(un[keep])
        if not C:
            continue
        code, M, R, OK, UN = (np.concatenate(a) for a in (C, M, R, OK, UN))
        possible.append(np.unique(code))
        # a row that an earlier sub-step left ambiguous may meet this one with another threshold and other ids: whatever is
        # proposed to it now is unclear for the counters
        n_unclear += int((amb[code // n] != 0).sum())
        amb[code[UN] // n] |= R_THRESHOLD
        n_unclear += int(UN.sum())
        code, M, R = code[OK], M[OK], R[OK]
        proposals += len(code)
        if len(code) == 0:  # a late iteration: vertices joined, nothing passed
            continue
        code, first = np.unique(code, return_index=True)  # repeats of one (target, source) carry one value: one key
        T, S, M, R = code // n, code % n, M[first], R[first]
        if slots is not None:
            # (T, S) ascend here; a stable sort by (target, slot) keeps the sources of a slot ascending, so the first of the
            # entries at the slot's smallest distance is its smallest (d, s) key
            grp = T * 64 + slot_of[S]
            o = np.argsort(grp, kind="stable")
            T, S, M, R, grp = T[o], S[o], M[o], R[o], grp[o]
            head = np.r_[True, grp[1:] != grp[:-1]]
            starts, gid = np.flatnonzero(head), np.cumsum(head) - 1
            at_min = M == np.minimum.reduceat(M, starts)[gid]
            w = np.minimum.reduceat(np.where(at_min, np.arange(len(M)), len(M)), starts)[gid]  # the slot's winner, for every member
            lose = w != np.arange(len(M))
            if lose.any():
                lost.append(np.stack([T[lose], S[w[lose]], M[w[lose]], S[lose], M[lose]], 1))
                un = lose & (M - R <= M[w] + R[w]) & ((R > 0.0) | (R[w] > 0.0))
                amb[T[un]] |= R_COLLISION
                n_unclear += int(un.sum())
            T, S, M, R = T[~lose], S[~lose], M[~lose], R[~lose]
        c += len(T)
        # ---- merge: the k smallest (d, id) of row U winners, for every row that has a winner (T ascends) ----
        rows, cnt = np.unique(T, return_counts=True)
        ri = np.repeat(np.arange(len(rows)), cnt)
        pos = k + np.arange(len(T)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        width = k + int(cnt.max())
        e_id = np.full((len(rows), width), -1, np.int64)
        e_mid = np.full((len(rows), width), np.inf)
        e_rad = np.zeros((len(rows), width))
        e_fl = np.zeros((len(rows), width), np.uint8)
        e_id[:, :k], e_mid[:, :k], e_rad[:, :k], e_fl[:, :k] = ids[rows], d_mid[rows], d_rad[rows], flags[rows]
        e_id[ri, pos], e_mid[ri, pos], e_rad[ri, pos], e_fl[ri, pos] = S, M, R, 1
        o = np.argsort(e_mid + 1j * e_id, axis=1)  # complex keys order by (real, imag) = (d, id); unfilled (inf, -1) last
        e_id, e_mid, e_rad, e_fl = (np.take_along_axis(a, o, 1) for a in (e_id, e_mid, e_rad, e_fl))
        on = e_id >= 0
        kept, drop = on[:, :k], on[:, k:]
        # the keys on either side of the k-th place: the largest upper end kept against the smallest lower end dropped,
        # where at least one of the two is inexact
        hi, lo = e_mid + e_rad, e_mid - e_rad
        for k_sel, d_sel in ((kept, drop & (e_rad[:, k:] > 0.0)), (kept & (e_rad[:, :k] > 0.0), drop)):
            un = np.where(k_sel, hi[:, :k], -np.inf).max(1) >= np.where(d_sel, lo[:, k:], np.inf).min(1)
            amb[rows[un]] |= R_BOUNDARY
            n_unclear += int(un.sum())
        tie[rows[np.where(kept, e_mid[:, :k], -np.inf).max(1) == np.where(drop, e_mid[:, k:], np.inf).min(1)]] = True
        ids[rows], d_mid[rows], d_rad[rows], flags[rows] = e_id[:, :k], e_mid[:, :k], e_rad[:, :k], e_fl[:, :k]

    possible = np.unique(np.concatenate(possible)) if possible else np.zeros(0, np.int64)
    lost = np.concatenate(lost) if lost else np.zeros((0, 5))
    return IterResult(ids.astype(np.int32), d_mid, d_rad, flags, amb, c, proposals, join_pairs, n_unclear, possible, lost, tie)


def row_partners(res, n, t):
    """the sources that may have reached row t in the iteration (ascending ids)."""
    lo, hi = np.searchsorted(res.possible, [t * n, (t + 1) * n])
    return res.possible[lo:hi] - t * n
