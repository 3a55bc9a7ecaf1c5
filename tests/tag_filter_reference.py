"""The tagged walk (csrc/query.hip, k_query's Q_FILT_TAGS instances) as a step-exact model: tests/filter_reference.py with a different allow array
per query -- ``allowed_i = (tags & masks[i]) != 0``.  Every query keeps its place in the batch: the kernel's seed for a query
(ties in the tree descent, the random start vertices) is keyed by the query's number.  Test infrastructure.

Tags are in the SEARCHER's numbering (the numbering of the cases' data rows)."""
import numpy as np

from tests import filter_reference as FR
from tests import search_reference as SR

N_TAGS = 3
SELECTIVITIES = (0.5, 0.1, 0.02)  # of tag 0, 1, 2; bit 63 rides on tag 0's rows


def case_tags(n):
    """The tag words every tagged test uses for a case of n rows: tag t on about SELECTIVITIES[t] of the rows, drawn independently
    (so some rows carry none: word 0), and bit 63 on every other row of tag 0."""
    rs = np.random.RandomState(11)
    tags = np.zeros(n, np.uint64)
    for t, sel in enumerate(SELECTIVITIES):
        tags[rs.random_sample(n) < sel] |= np.uint64(1) << np.uint64(t)
    with_zero = np.flatnonzero(tags & np.uint64(1))
    tags[with_zero[::2]] |= np.uint64(1) << np.uint64(63)
    return tags


def case_masks(nq):
    """Query i takes mask 1 << (i % N_TAGS); every seventh query a two-bit mask (tags 1 and 2), and query 1 the mask whose only
    bit is 63."""
    masks = np.uint64(1) << (np.arange(nq) % N_TAGS).astype(np.uint64)
    masks[3::7] = np.uint64(0b110)
    if nq > 1:
        masks[1] = np.uint64(1) << np.uint64(63)
    return masks


def allowed_of(tags, mask):
    return (np.asarray(tags).view(np.uint64) & np.uint64(mask)) != 0


def run_walk(walk, tags, masks, queries, k, k_out=None):
    """One query after the other on the filtered walk ``walk``, each under its own allow array, each in its place."""
    out = []
    for qi, q in enumerate(np.asarray(queries)):
        walk.allowed = allowed_of(tags, masks[qi])
        walk.k = int(k)
        walk.run(qi, q)
        out.append(walk.finish(k_out))
    return out


def reference_search(tags, masks, data, indptr, indices, tree, metric, min_distance, n_neighbors, queries, k, epsilon, seed_state=None, *,
                     exact=False, codes=None, values=None, rerank_k=None, trace=False):
    """``filter_reference.reference_search`` with the allow array of query i being ``(tags & masks[i]) != 0``."""
    code = SR.METRIC_CODE[metric] if isinstance(metric, str) else int(metric)
    data = np.asarray(data)
    dist = SR._Distances(data, code, exact, codes, values)
    walk = FR._FilteredWalk(np.zeros(data.shape[0], bool), data.shape[0], np.asarray(indptr, np.int64), np.asarray(indices, np.int64), tree,
                            dist, min_distance, int(n_neighbors), int(k), epsilon, SR.searcher_seed(seed_state), trace)
    return run_walk(walk, tags, masks, queries, k, rerank_k if codes is not None else None)


_CACHE = {}


def get(name, masks=None):
    """(case, tags, masks, tagged reference results) of a case of tests/search_cases.py; ``masks`` None: ``case_masks``, else one
    mask word for every query.  Computed once per process."""
    from tests import search_cases as SC

    key = (name, None if masks is None else int(masks))
    if key not in _CACHE:
        c, _ = SC.get(name)
        tags = case_tags(c.data.shape[0])
        m = case_masks(len(c.queries)) if masks is None else np.full(len(c.queries), masks, np.uint64)
        if c.values is not None:
            res = reference_search(tags, m, c.data, c.indptr, c.indices, c.tree, c.metric, c.min_distance, c.n_neighbors, c.queries,
                                   c.search_k, c.epsilon, c.rng_state, exact=True, codes=c.codes, values=c.values, rerank_k=c.k)
        else:
            res = reference_search(tags, m, c.data, c.indptr, c.indices, c.tree, c.metric, c.min_distance, c.n_neighbors, c.queries, c.k,
                                   c.epsilon, c.rng_state, exact=c.exact)
        _CACHE[key] = (c, tags, m, res)
    return _CACHE[key]
