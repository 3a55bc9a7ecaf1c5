"""Metric code 6 (proxy_inner_product) for the step-exact descent model (tests/descent_reference.py, used unchanged): the
prepared rows and the Gram-form distance of the build kernels with its a-priori radius, the cases that reach every kernel family
with that code, and a builder (the oracle, and with it tests/gpu_util.py make_builder, does not know the code).  Test helpers."""
from collections import namedtuple

import numpy as np

from oracle import oracle as O
from pynndescent_amd import _capi
from tests import descent_cases as DC
from tests import descent_reference as DR
from tests import metric_util as MU
from tests import proxy_util as PU


class ProxyPrepared(DR.Prepared):
    """Rows as given and nrm = |x|^2, like inner product (csrc/prep.hip); distances by metric.h nnd_proxy_ip_dist."""

    def __init__(self, data, exact=False):
        assert not exact, "the proxy has a log2 and two roots: no lattice makes it exact"
        super().__init__(data, "inner_product", False)
        self.code = PU.CODE
        # d(x, x) as the kernels set it (nnd_self_dist): 1 / |x| from the float32 norm by one hardware inverse root
        with np.errstate(divide="ignore"):
            self.self_mid = np.where(self.nrm > 0.0, np.minimum(1.0 / np.sqrt(np.where(self.nrm > 0.0, self.nrm, 1.0)), PU.FLT_MAX), PU.FLT_MAX)
        fin = self.self_mid < PU.FLT_MAX
        self.self_rad = np.where(fin, self.gamma * self.self_mid + 4.0 * PU._ulp32(self.self_mid), 0.0)

    def block(self, a_ids, b_ids):
        ra, rb = self.rows[a_ids], self.rows[b_ids]
        g = ra @ rb.transpose(0, 2, 1)
        dg = self.gamma * (self.absrows[a_ids] @ self.absrows[b_ids].transpose(0, 2, 1))
        mid, lo, hi = PU.proxy_interval(g, dg, self.nrm[a_ids][:, :, None], self.nrm[b_ids][:, None, :], self.gamma)
        return mid, np.maximum(hi - mid, mid - lo)


Case = namedtuple("Case", ["name", "k", "mc", "n", "d", "n_trees", "join_blocks", "flags", "exact", "seed", "iters", "doc"])

# the smallest n of tests/descent_cases.py at which each join kernel reaches its steady state (its "Sizing n")
CASES = {c.name: c for c in [
    Case("proxy_k15_mc15", 15, 15, DC.N16, 24, 2, 1, 0, False, 1, (0, 1),
         "k_leaf_join + k_local_join16 (the code-6 instance) + k_merge_q"),
    Case("proxy_k30_mc30", 30, 30, DC.NW32, 24, 2, 1, 0, False, 1, (0, 1),
         "k_leaf_join_sym + k_local_join_w<32> staged + k_merge"),
    Case("proxy_k100_mc60", 100, 60, DC.NW64, 24, 2, 1, 0, False, 1, (0,),
         "k_leaf_join_rb wide + k_local_join_w<64> + k_merge_wide"),
]}
_DATA = {}


def data(case):
    """The inner-product fixture rows (clustered, shifted by 0.5: mostly positive products, some negative) with three zero rows."""
    if case.name not in _DATA:
        x = MU.metric_data("inner_product", case.n, case.d, seed=11)[0]
        x[[7, 500, 1500]] = 0.0
        x.setflags(write=False)
        _DATA[case.name] = x
    return _DATA[case.name]


def rng_state(case):
    return O.draw_rng_states(case.seed, max(case.n_trees, 1))[0]


def make_builder(x, k=15, n_trees=2, leaf_size=None, mc=None, n_iters=None, delta=0.001, seed=1, join_blocks=1, flags=0):
    """tests/gpu_util.py make_builder for metric code 6."""
    n, d = x.shape
    state, _, tree_states = O.draw_rng_states(seed, max(n_trees, 1))
    b = _capi.Builder(n, d, PU.CODE, k, n_trees, O.default_leaf_size(k) if leaf_size is None else leaf_size, 200,
                      min(60, k) if mc is None else mc, O.default_n_iters(n) if n_iters is None else n_iters, delta, state,
                      tree_states[0], join_blocks=join_blocks, flags=flags)
    b.set_data_host(np.ascontiguousarray(x, np.float32))
    return b
