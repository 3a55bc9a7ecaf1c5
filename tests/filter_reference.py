"""The filtered walk (csrc/query.hip, k_query's Q_FILT_ALLOW instances) as a step-exact model: tests/search_reference.py with one rule added --
a vertex enters the walk's result list only if it is allowed.  Everything else is the unfiltered walk: the descent, the seeds,
the visited set, every accepted candidate pushed to the frontier, the bound taken from the (allowed-only) result list and +inf
while that list is short, the stop rule.  Test infrastructure.

Masks are in the SEARCHER's numbering (the numbering of the cases' data rows)."""
import numpy as np

from tests import search_reference as SR

FRACTIONS = (0.5, 0.1)


def case_mask(n, frac):
    """The allow mask every filtered test uses for a case of n rows."""
    return np.random.RandomState(7).random_sample(n) < frac


class _FilteredWalk(SR._Walk):
    def __init__(self, allowed, *args):
        super().__init__(*args)
        self.allowed = np.asarray(allowed, bool)

    def result_push(self, c):
        if not self.allowed[c[3]]:
            return
        super().result_push(c)

    def finish(self, k_out=None):
        # the "boundary tie" count compares the list with everything that could have entered it: the allowed vertices seen
        keep = [self.allowed[ids] for ids in self.seen_ids]
        self.seen_mid = [m[a] for m, a in zip(self.seen_mid, keep)]
        self.seen_ids = [i[a] for i, a in zip(self.seen_ids, keep)]
        return super().finish(k_out)


def reference_search(allowed, data, indptr, indices, tree, metric, min_distance, n_neighbors, queries, k, epsilon, seed_state=None, *,
                     exact=False, codes=None, values=None, rerank_k=None, trace=False):
    """``search_reference.reference_search`` under the allow mask ``allowed`` (n, bool): one SearchResult per query.  With
    ``trace=True`` the trace's ``seen_ids`` / ``seen_mid`` hold the ALLOWED vertices whose distance was computed; ``visited``
    holds every vertex the walk marked, allowed or not."""
    code = SR.METRIC_CODE[metric] if isinstance(metric, str) else int(metric)
    data = np.asarray(data)
    dist = SR._Distances(data, code, exact, codes, values)
    walk = _FilteredWalk(allowed, data.shape[0], np.asarray(indptr, np.int64), np.asarray(indices, np.int64), tree, dist, min_distance,
                         int(n_neighbors), int(k), epsilon, SR.searcher_seed(seed_state), trace)
    out = []
    for qi, q in enumerate(np.asarray(queries)):
        walk.k = int(k)
        walk.run(qi, q)
        out.append(walk.finish(rerank_k if codes is not None else None))
    return out


_CACHE = {}


def get(name, frac, trace=False):
    """(case, allow mask, filtered reference results) of a case of tests/search_cases.py at ``frac``; frac None: all rows
    allowed.  Computed once per process."""
    from tests import search_cases as SC

    key = (name, frac, trace)
    if key not in _CACHE:
        c, _ = SC.get(name)
        mask = np.ones(c.data.shape[0], bool) if frac is None else case_mask(c.data.shape[0], frac)
        if c.values is not None:
            res = reference_search(mask, c.data, c.indptr, c.indices, c.tree, c.metric, c.min_distance, c.n_neighbors, c.queries, c.search_k,
                                   c.epsilon, c.rng_state, exact=True, codes=c.codes, values=c.values, rerank_k=c.k, trace=trace)
        else:
            res = reference_search(mask, c.data, c.indptr, c.indices, c.tree, c.metric, c.min_distance, c.n_neighbors, c.queries, c.k,
                                   c.epsilon, c.rng_state, exact=c.exact, trace=trace)
        _CACHE[key] = (c, mask, res)
    return _CACHE[key]


# the cases of the filtered tests: (name, frac).  routing_wide is left out (under a filter it visits all 20 000 vertices and
# flags 0.85 of its queries and more); the float cases are used at 0.5 only (at 0.1 up to 0.67 of their queries are flagged).
def lattice_names():
    from tests import search_cases as SC

    return sorted(n for n in SC.LATTICE if not n.startswith("routing"))


def all_cases():
    from tests import search_cases as SC

    out = [(n, f) for n in lattice_names() + sorted(SC.Q8) for f in FRACTIONS]
    out += [(n, 0.5) for n in sorted(SC.FLOAT)]
    return out


LATTICE_CAP, FLOAT_CAP = 0.25, 0.35  # the largest share of flagged queries per case (measured: 0.17 and 0.27)
