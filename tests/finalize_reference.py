"""Host model of the distances and the row order that finalize hands back (csrc/finalize.hip, header), for the codes 0
(sqeuclidean) and 1 (cosine, as -log2 of it) on rows of whole 16-byte chunks (d % 4 == 0), k <= 64.

Every float64 operation of the device path is restated here one rounding at a time:

  * 16 lanes split a pair of rows by chunks of four floats: lane l takes the chunks t = 4 l + 64 i, i = 0, 1, ..;
  * a chunk's four terms join as s = p1 (one multiplication), then s = fma(., ., s) for p0, p2, p3 in that order, and
    the lane's sum takes s by one addition.  Code 0: p_j = (a_j - b_j)^2 on the rounded float64 difference.  Code 1: three
    sums, of a_j b_j, a_j a_j and b_j b_j;
  * the 16 lanes' sums join by the xor butterfly with the offsets 8, 4, 2, 1: v[l] += v[l ^ o], all lanes at once;
  * code 0: the value is float32 of that sum.  Code 1: metric.h nnd_ref_dist on the three sums -- 0 for two zero rows,
    FLT_MAX for one zero row or <a, b> <= 0, else max(log2(sqrt(|a|^2 |b|^2) / <a, b>), 0), and float32 of that.

Subtraction, multiplication, addition, division and square root are numpy's / Python's float64 operations (IEEE, correctly
rounded, as the device's); the fused multiply-add is computed on exact integers and rounded once (Python 3.10 has no
math.fma).  log2 is the one operation that is not correctly rounded on either side (each within 1 ulp of float64), so it
fixes the float32 handed back unless the float64 value lies within 8 ulp of the midpoint of two float32 values: the model
raises ``AmbiguousLog2`` for such a pair instead of guessing (1 pair in 10^7; a test's fixed inputs either have one or not).

Rows come back ordered by (float32 bits of the distance, index), empty slots last as (-1, +inf).

``fma_order`` and ``butterfly`` exist for tests/test_finalize_reference_cpu.py, which plants a wrong order and shows that
the comparison notices."""
import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
FMA_ORDER = (0, 2, 3)     # after p1
BUTTERFLY = (8, 4, 2, 1)


class AmbiguousLog2(Exception):
    pass


def _split(v):
    """finite float -> (m, e) with v == m * 2**e, m an integer"""
    m, e = math.frexp(v)
    return int(m * 9007199254740992.0), e - 53


def fma(a, b, c):
    """a * b + c with one rounding (round to nearest even), on exact integers"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    ma, ea = _split(a)
    mb, eb = _split(b)
    mc, ec = _split(c)
    p, ep = ma * mb, ea + eb
    if p == 0 or mc == 0:
        return a * b + c if p == 0 else _round(p, ep)
    e = min(ep, ec)
    return _round((p << (ep - e)) + (mc << (ec - e)), e)


def _round(m, e):
    if m == 0:
        return 0.0
    return math.ldexp(float(m), e)  # int -> float rounds to nearest even; ldexp is exact above the subnormal range


def _chunk(a, b, order):
    """one chunk of <a, b>: a, b sequences of four floats (float64 values)"""
    s = a[1] * b[1]
    for j in order:
        s = fma(a[j], b[j], s)
    return s


def _lane_sums(a, b, kind, order):
    """the 16 lanes' sums for rows a, b (float64 arrays of length d): kind 'sq' | 'dot'"""
    d = a.shape[0]
    if kind == "sq":
        a = a - b  # float64 differences, one rounding each
        b = a
    al, bl = a.tolist(), b.tolist()
    out = [0.0] * 16
    for lane in range(16):
        acc = 0.0
        for t in range(4 * lane, d, 64):
            acc = acc + _chunk(al[t:t + 4], bl[t:t + 4], order)
        out[lane] = acc
    return out


def _butterfly(v, offsets):
    v = list(v)
    for o in offsets:
        v = [v[l] + v[l ^ o] for l in range(16)]
    assert all(math.isnan(x) or x == v[0] for x in v)  # addition commutes: every lane ends on the same value
    return v[0]


def _cosine_value(dt, ax, ay):
    if ax == 0.0 and ay == 0.0:
        return np.float32(0.0)
    if ax == 0.0 or ay == 0.0 or dt <= 0.0:
        return np.float32(FLT_MAX)
    r = math.log2(math.sqrt(ax * ay) / dt)
    if not r > 0.0:
        return np.float32(0.0)
    f = np.float32(r)
    # the float32 neighbours' midpoints: r must stay clear of them by more than both sides' log2 error
    for other in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
        mid = 0.5 * (float(f) + float(other))
        if abs(r - mid) <= 8.0 * math.ulp(r):
            raise AmbiguousLog2("log2 value %r within 8 ulp of the float32 midpoint %r" % (r, mid))
    return f


class Model:
    """Distances of one point set; per-row sums of code 1 are computed once."""

    def __init__(self, x, metric, fma_order=FMA_ORDER, butterfly=BUTTERFLY):
        x = np.asarray(x, np.float32)
        assert x.ndim == 2 and x.shape[1] % 4 == 0 and metric in (0, 1)
        self.x64 = x.astype(np.float64)
        self.metric, self.order, self.offsets = metric, tuple(fma_order), tuple(butterfly)
        self._norm = {}

    def _sum(self, a, b, kind):
        return _butterfly(_lane_sums(a, b, kind, self.order), self.offsets)

    def norm(self, i):
        if i not in self._norm:
            self._norm[i] = self._sum(self.x64[i], self.x64[i], "dot")
        return self._norm[i]

    def value(self, i, j):
        """the float32 handed back for the pair (row i, neighbour j)"""
        a, b = self.x64[i], self.x64[j]
        if self.metric == 0:
            return np.float32(self._sum(a, b, "sq"))
        return _cosine_value(self._sum(a, b, "dot"), self.norm(i), self.norm(j))

    def rows(self, graph):
        """graph: int (n, k), -1 = empty slot, ids unique within a row -> (idx int32 (n, k), dist float32 (n, k))"""
        graph = np.asarray(graph)
        n, k = graph.shape
        idx = np.full((n, k), -1, np.int32)
        dist = np.full((n, k), np.inf, np.float32)
        for i in range(n):
            ent = []
            for j in graph[i].tolist():
                if j >= 0:
                    v = self.value(i, j)
                    ent.append((int(np.asarray(v, np.float32).view(np.uint32)), j, v))
            ent.sort(key=lambda t: (t[0], t[1]))
            for c, (_, j, v) in enumerate(ent):
                idx[i, c], dist[i, c] = j, v
        return idx, dist


def finalize_rows(x, graph, metric, **kw):
    return Model(x, metric, **kw).rows(graph)


# Inputs on which a wrong order shows in the float32 handed back (sqeuclidean, neighbour = the zero row).  u = 2^-52, the
# float64 ulp at 1; s is a float32 with s^2 = 0.3 u: two such terms survive an addition to 1 only if they are joined first.
_S = np.float32(math.sqrt(0.3) * 2.0 ** -26)


def sensitive_fma_rows():
    """d = 4, lane 0 only.  p1 = p0 = 0.3 u, p2 = 1, p3 = 2^-24: the pinned order sums 0.6 u first, 1 + 0.6 u rounds to
    1 + u, and 1 + 2^-24 + u lies above the float32 tie -> 1 + 2^-23; with p0 and p2 swapped both small terms are lost and
    the tie 1 + 2^-24 rounds to even -> 1."""
    x = np.zeros((2, 4), np.float32)
    x[0] = [_S, _S, 1.0, 2.0 ** -12]
    return x


def sensitive_butterfly_rows():
    """d = 64, one chunk per lane with one non-zero entry: lane sums P0 = 1, P8 = 2^-24, P1 = P9 = 0.3 u.  Offsets 8, 4, 2, 1
    join P1 + P9 = 0.6 u before it meets 1 + 2^-24 -> 1 + 2^-23; offsets 1, 2, 4, 8 lose P1 in 1 + 0.3 u -> 1."""
    x = np.zeros((2, 64), np.float32)
    x[0, 0], x[0, 32], x[0, 4], x[0, 36] = 1.0, 2.0 ** -12, _S, _S
    return x
