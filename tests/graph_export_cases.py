"""The cases of the graph export's width tests (tests/test_graph_export_cpu.py, tests/test_gpu_graph_export_widths.py) and
what each is claimed to reach in csrc/csr_graph.hip.

The staged length of a row of the symmetric form is k plus its in-degree off the diagonal (csr_stretch); k_csr_sym_merge picks
    csr_union_row<1,16>   length <= 16          csr_union_row<2,64>   65..128
    csr_union_row<1,32>   17..32                csr_union_row<4,64>   129..256
    csr_union_row<1,64>   33..64                csr_union_row<8,64>   257..512          k_csr_sym_merge_long   > 512
and launch_write_rows picks k_csr_write_rows<KU, W, IdT> by k: <1,16> k <= 16, <1,32> 17..32, <1,64> 33..64, <2,64> 65..128,
<4,64> 129..256.  Random k-lists reach the middle of that table only, so the symmetric cases here are designed: named rows
get an exact staged length (both sides of every threshold, and long rows whose length is no power of two), and a designated row
points back at one of its sources where the twin pair -- the same column twice, adjacent after the sort -- has to straddle two
registers of a lane (sorted positions 64 u - 1, 64 u) or two 256-key pieces of the long-row collapse.

tests/test_graph_export_cpu.py asserts, without a GPU, that every case reaches what it is written for.
"""
from collections import namedtuple

import numpy as np

from tests.graph_export_util import random_klists, symmetric_values

MERGE_INSTANCES = (16, 32, 64, 128, 256, 512, "long")
BOUNDARY_LENGTHS = (16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513)
WRITE_INSTANCES = ((1, 16), (1, 32), (1, 64), (2, 64), (4, 64))
LONG_GRID = 256  # the workgroups of k_csr_sym_merge_long's launch (csr_build)
SUBNORMAL_BITS = np.uint32(71362)  # 1e-40 as float32: 71362 x 2^-149


# ------------------------------------------------------------------------------------------------ what a row reaches
def _valid(ids, n):
    ids = np.asarray(ids).astype(np.int64)
    return ids, (ids >= 0) & (ids < n)


def stretch_lengths(ids, n, k, drop_self=False):
    """The staged length of every row of the symmetric form: k plus the number of places (i, j), 0 <= j < n, j != i, that name
    the row (csr_stretch over k_csr_sym_count's counts).  ``drop_self`` does not change it: the diagonal never has a reverse."""
    ids, ok = _valid(ids, n)
    assert ids.shape == (n, k)
    off = ok & (ids != np.arange(n, dtype=np.int64)[:, None])
    return k + np.bincount(ids[off], minlength=n).astype(np.int64)


def merge_instance(length):
    """W * KU of the csr_union_row instance, or "long": the thresholds of k_csr_sym_merge."""
    for cap in MERGE_INSTANCES[:-1]:
        if length <= cap:
            return cap
    return "long"


def write_instance(k):
    """(KU, W) of k_csr_write_rows as launch_write_rows picks them."""
    assert 1 <= k <= 256
    return (1, 16) if k <= 16 else (1, 32) if k <= 32 else (1, 64) if k <= 64 else (2, 64) if k <= 128 else (4, 64)


def instance_counts(ids, n, k):
    """Rows per merge instance, in the order of MERGE_INSTANCES."""
    inst = [merge_instance(int(v)) for v in stretch_lengths(ids, n, k)]
    return [inst.count(i) for i in MERGE_INSTANCES]


def sorted_stretch(ids, vals, n, row):
    """(columns, value bits) of the filled keys of the row's stretch -- its own places and its reverse edges -- in the merge's
    order: by (column, value bits)."""
    ids, ok = _valid(ids, n)
    bits = np.ascontiguousarray(vals, dtype=np.float32).view(np.uint32)
    own = ok[row]
    src, place = np.nonzero(ok & (ids == row))
    rev = src != row
    cols = np.concatenate([ids[row][own], src[rev]])
    vbits = np.concatenate([bits[row][own], bits[src[rev], place[rev]]])
    order = np.lexsort((vbits, cols))
    return cols[order], vbits[order]


def twin_positions(ids, vals, n, row):
    """The positions p, in the row's sorted stretch, at which a column occurs twice (at p and p + 1)."""
    cols, _ = sorted_stretch(ids, vals, n, row)
    return np.nonzero(cols[1:] == cols[:-1])[0].tolist()


def mutual_pairs(ids, n, rows):
    """The pairs (r, s), r in ``rows``, s != r, of which each lists the other."""
    ids, ok = _valid(ids, n)
    out = []
    for r in rows:
        listed = set(ids[r][ok[r]].tolist()) - {r}
        src = np.nonzero((ok & (ids == r)).any(axis=1))[0]
        out += [(int(r), int(s)) for s in src if int(s) in listed]
    return out


# ------------------------------------------------------------------------------------------------ the designed generator
def designed_klists(n, k, lengths, mutual=(), seed=0, id_dtype=np.int32, empty=0.1, diagonal=0.3):
    """(n, k) ids, no id twice in a row, in which row r has exactly the staged length ``lengths[r]`` and every other row a
    random in-degree.

    The sources of a designated row are undesignated rows (the least loaded ones, so no source runs out of places), and the
    random places of the undesignated rows name undesignated rows only: nothing else reaches a designated row.  A designated
    row keeps two -1 places and holds no diagonal; about ``diagonal`` of the other rows do, and ``empty`` of their random places
    are -1.  Every row is shuffled.  ``mutual``: (row, position) -- the designated row lists one of its sources, the one whose
    column then stands twice at the sorted positions position, position + 1 of the row's stretch (a negative position counts
    from the end of the filled keys: -2 is the last two); such a row lists no other source of its own."""
    rs = np.random.RandomState(seed)
    rows = sorted(int(r) for r in lengths)
    designated = np.zeros(n, bool)
    designated[rows] = True
    free = np.nonzero(~designated)[0]
    load = np.zeros(n, np.int64)
    sources = {}
    for r in sorted(rows, key=lambda r: -lengths[r]):
        d = int(lengths[r]) - k
        assert 0 <= d <= free.shape[0], "row %d: length %d is out of reach" % (r, lengths[r])
        order = free[np.lexsort((rs.random_sample(free.shape[0]), load[free]))]  # the least loaded first, ties at random
        sources[r] = np.sort(order[:d])
        load[sources[r]] += 1
    assert load.max() < k
    want = {}
    for r, p in mutual:
        assert designated[r]
        want.setdefault(int(r), []).append(int(p))
    ids = np.full((n, k), -1, np.int64)
    for r in rows:
        s, ps = sources[r], want.get(r, [])
        n_empty = 2 if k - len(ps) >= 3 else 0
        n_fwd = k - len(ps) - n_empty
        if not ps:
            row = rs.permutation(free)[:n_fwd]  # (may name a source of its own: a twin somewhere)
        else:
            others = np.setdiff1d(free, s)
            assert others.shape[0] >= n_fwd
            for _ in range(1000):
                fwd = np.sort(rs.permutation(others)[:n_fwd])
                cols = np.union1d(s, fwd)
                filled = cols.shape[0] + len(ps)
                at = [p if p >= 0 else filled + p for p in ps]
                pick = [p - t for t, p in enumerate(sorted(at))]  # t twins stand in front of the t-th
                if len(set(pick)) == len(pick) and all(0 <= c < cols.shape[0] for c in pick) and np.isin(cols[pick], s).all():
                    break
            else:
                raise AssertionError("row %d: no draw puts a source at %s" % (r, ps))
            row = np.concatenate([fwd, cols[pick]])
        ids[r, : row.shape[0]] = row
        ids[r] = ids[r][rs.permutation(k)]
    targets = [[] for _ in range(n)]
    for r in rows:
        for s in sources[r]:
            targets[s].append(r)
    for i in free:
        room = k - len(targets[i])
        fill = rs.permutation(free)
        fill = fill[fill != i][:room]
        fill[rs.random_sample(fill.shape[0]) < empty] = -1
        if room and rs.random_sample() < diagonal:
            fill[0] = i
        row = np.concatenate([np.asarray(targets[i], np.int64), fill])
        ids[i, : row.shape[0]] = row
        ids[i] = ids[i][rs.permutation(k)]
    return ids.astype(id_dtype)


# ------------------------------------------------------------------------------------------------ values
def _pair_hash(ids, seed):
    ids = np.asarray(ids).astype(np.int64)
    i = np.repeat(np.arange(ids.shape[0], dtype=np.int64)[:, None], ids.shape[1], axis=1)
    lo, hi = np.minimum(i, ids).view(np.uint64), np.maximum(i, ids).view(np.uint64)
    h = lo * np.uint64(2654435761) + hi * np.uint64(40503) + np.uint64(12345 + 97 * seed)  # (wraps)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    return i, ids, lo, hi, h


def signed_values(ids, seed, differ=()):
    """Values of every sign, a function of the unordered pair: 0.0 on the diagonal and on a sixteenth of the pairs, a subnormal
    (1e-40) and 3e38 on a sixteenth each, else a normal in 0.01 .. 4.01, the nonzero ones negative on half of the pairs.  No NaN.

    On a tenth of the pairs -- so on a tenth of the mutual ones, where it shows -- the direction i > j differs from i < j: one
    ulp further from zero, or the other sign, or -0.0 against +0.0 (a third each).  ``differ``: pairs (i, j) that are put among
    those with a nonzero normal, alternately of the other sign and, negative, one ulp further from zero: the two forms in which
    the smaller float is the one with the LARGER bit pattern, which the merge's sort puts second (csr_min_with_twin's `after`)."""
    i, j, lo, hi, h = _pair_hash(ids, seed)
    cat = (h & np.uint64(15)).astype(np.int64)
    mag = (0.01 + ((h >> np.uint64(8)) & np.uint64(0xFFFFF)).astype(np.float64) / 2 ** 20 * 4.0).astype(np.float32)
    negative = ((h >> np.uint64(4)) & np.uint64(1)).astype(bool)
    chosen = ((h >> np.uint64(32)) % np.uint64(10)) == 0
    kind = ((h >> np.uint64(40)) % np.uint64(3)).astype(np.int64)
    if len(differ):
        d = np.asarray(differ, np.int64).reshape(-1, 2)
        codes = np.unique(np.minimum(d[:, 0], d[:, 1]) * 2 ** 32 + np.maximum(d[:, 0], d[:, 1]))
        code = lo.view(np.int64) * 2 ** 32 + hi.view(np.int64)
        at = np.minimum(np.searchsorted(codes, code), codes.shape[0] - 1)
        forced = (codes[at] == code) & (j >= 0)
        odd = (at & 1).astype(bool)
        cat = np.where(forced, 8, cat)
        chosen = chosen | forced
        kind = np.where(forced, np.where(odd, 0, 1), kind)
        negative = np.where(forced & odd, True, negative)
    # (assembled as bit patterns: the same values in a process whose host arithmetic flushes subnormals to zero)
    sign = np.uint32(0x80000000)
    b = np.where(cat == 0, np.uint32(0), np.where(cat == 1, SUBNORMAL_BITS, np.where(cat == 2, np.float32(3e38).view(np.uint32), mag.view(np.uint32))))
    b = np.where(negative & (cat != 0), b | sign, b).astype(np.uint32)
    upper = chosen & (i > j)
    b = np.where(upper & (kind == 0), b + np.uint32(1), b)  # one ulp further from zero, whatever the sign
    b = np.where(upper & (kind == 1), b ^ sign, b)
    b = np.where(chosen & (kind == 2), np.where(i > j, sign, np.uint32(0)), b)
    b = np.where(i == j, np.uint32(0), b).astype(np.uint32)
    assert ((b & np.uint32(0x7F800000)) != np.uint32(0x7F800000)).all()  # finite
    return b.view(np.float32)


# ------------------------------------------------------------------------------------------------ the symmetric cases
SymCase = namedtuple("SymCase", ["name", "n", "k", "id_dtype", "lengths", "mutual", "doc"])

_B_LENGTHS = (15, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 767, 768, 1024, 1025, 2500)
_B_ROW = {length: 100 + 37 * i for i, length in enumerate(_B_LENGTHS)}
_W_LENGTHS = (128, 129, 256, 257, 512, 513, 700)
_W_ROW = {length: 50 + 83 * i for i, length in enumerate(_W_LENGTHS)}

SYMMETRIC = {c.name: c for c in [
    SymCase("boundaries_k15", 3000, 15, np.int32, {r: length for length, r in _B_ROW.items()},
            ((_B_ROW[128], 63),                                          # <2,64>: key[0] lane 63 / key[1] lane 0
             (_B_ROW[256], 127),                                         # <4,64>: key[1] / key[2]
             (_B_ROW[257], 63),                                          # <8,64>
             (_B_ROW[512], 63), (_B_ROW[512], 255), (_B_ROW[512], 447),  # <8,64>: key[0]/[1], key[3]/[4], key[6]/[7]
             (_B_ROW[1025], 255), (_B_ROW[1025], 511),                   # long: the first and second piece boundary
             (_B_ROW[2500], 255), (_B_ROW[2500], 511), (_B_ROW[2500], 1279),
             (_B_ROW[767], -2)),                                         # long: the last two filled keys
            "both sides of every threshold of k_csr_sym_merge; long rows of 513, 767, 768, 1024, 1025 and 2500 keys; twins across "
            "registers and across pieces"),
    SymCase("wide_k100", 700, 100, np.int64, {r: length for length, r in _W_ROW.items()}, (),
            "k > 64: a staging stretch that begins with 100 fixed slots; k_csr_sym_count<int64_t>, k_csr_sym_scatter<int64_t>"),
    SymCase("many_long_k256", 800, 256, np.int32, None, (),
            "every place filled at k = 256: rows on <8,64> and more long rows than k_csr_sym_merge_long has workgroups"),
    SymCase("tiny_k1", 40, 1, np.int32, None, (), "every row names row 0: one stretch of 40 (in-degree above k), the others of 1"),
]}

_LISTS, _VALUES = {}, {}


def sym_lists(name):
    """The ids of a symmetric case (built once, read-only)."""
    if name not in _LISTS:
        c = SYMMETRIC[name]
        if name == "many_long_k256":
            ids = random_klists(800, 256, 800, seed=1, empty=0.0, empty_rows=0.0)[0]
        elif name == "tiny_k1":
            ids = np.zeros((c.n, 1), np.int32)
        else:
            ids = designed_klists(c.n, c.k, c.lengths, c.mutual, seed=len(name), id_dtype=c.id_dtype)
        assert ids.shape == (c.n, c.k) and ids.dtype == c.id_dtype
        ids.setflags(write=False)
        _LISTS[name] = ids
    return _LISTS[name]


def designed_pairs(name):
    """The mutual pairs of the rows of a case that were given twin positions."""
    c = SYMMETRIC[name]
    return mutual_pairs(sym_lists(name), c.n, sorted({r for r, _ in c.mutual}))


VALUE_SETS = ("symmetric", "signed")


def sym_values(name, which):
    if (name, which) not in _VALUES:
        ids = sym_lists(name)
        vals = symmetric_values(ids) if which == "symmetric" else signed_values(ids, seed=3, differ=designed_pairs(name))
        vals.setflags(write=False)
        _VALUES[name, which] = vals
    return _VALUES[name, which]


# ------------------------------------------------------------------------------------------------ the directed cases
DIRECTED = [  # (m, k, n, id dtype, empty share)
    (1, 17, 40, np.int32, 0.15),     # W = 32, a single row: the second half of the wave idle
    (7, 32, 40, np.int32, 0.15),     # W = 32, odd m
    (131, 17, 200, np.int32, 0.15),  # W = 32, odd m, more than one workgroup
    (5, 16, 30, np.int32, 0.15),     # W = 16, m % 4 = 1
    (129, 33, 200, np.int32, 0.15),  # <1,64> just past the threshold
    (37, 9, 60, np.int64, 0.15),     # int64 ids, one case per instance
    (45, 24, 80, np.int64, 0.15),
    (70, 50, 120, np.int64, 0.15),
    (66, 100, 300, np.int64, 0.15),
    (35, 200, 500, np.int64, 0.15),
    (33, 256, 400, np.int32, 0.0),   # every place of every row filled
    (64, 128, 128, np.int32, 0.0),   # k = n: every row names every column
]


def directed_lists(m, k, n, id_dtype, empty):
    """ids and values of a directed case: random_klists with whole rows emptied where there are enough rows, and a third of
    the values negative."""
    ids, vals = random_klists(m, k, n, seed=m * 1000 + k, empty=empty, empty_rows=0.1 if empty and m >= 30 else 0.0, id_dtype=id_dtype)
    vals = np.where(np.random.RandomState(k).random_sample(vals.shape) < 1 / 3, -vals, vals).astype(np.float32)
    return ids, vals
