"""Same bits, one library per run: a SHA-256 digest of NNDescent(...).neighbor_graph (dtype, shape and bytes of both arrays)
for the smallest shapes that reach every branch of the handle's plan (csrc/plan.h) and of its lifetime code (csrc/handle.hip,
csrc/transfer.hip).  Run once per library, each in a fresh process; PYNND_AMD_LIB selects the library:

    PYNND_AMD_LIB=<parent build> python tools/ab/api_split_bits.py > parent.txt
    python tools/ab/api_split_bits.py > new.txt
    python tools/ab/api_split_bits.py --compare parent.txt new.txt > profiles/api_split_bits.txt
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
        h.update(("%s %s " % (a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:32]


def rows(n, d, seed):
    return np.random.RandomState(seed).standard_normal((n, d)).astype(np.float32)


def via_nnd_build(_capi, x, k, n_trees, seed):
    """nnd_build: host buffers in and out (create, nnd_h2d_parallel, build, nnd_d2h_parallel, destroy in one call)"""
    lib = _capi.load_library()
    n, d = x.shape
    p = _capi.NNDParams()
    p.n, p.dim, p.metric, p.n_neighbors, p.n_trees, p.leaf_size = n, d, 0, k, n_trees, max(10, k)
    p.max_depth, p.max_candidates, p.n_iters, p.delta, p.device, p.join_blocks = 200, min(60, k), 10, 0.001, 0, 0
    for i in range(3):
        p.rng_state[i], p.tree_rng[i] = seed + i, 7 * seed + i
    idx, dist = np.empty((n, k), np.int32), np.empty((n, k), np.float32)
    err = C.create_string_buffer(512)
    rc = lib.nnd_build(C.byref(p), x.ctypes.data_as(C.c_void_p), None, None, 0, idx.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p),
                       None, err, 512)
    if rc != 0:
        raise RuntimeError(err.value.decode())
    return idx, dist


def run():
    import torch

    from pynndescent_amd import NNDescent, _capi

    def graph(x, **kw):
        kw.setdefault("n_neighbors", 10)
        kw.setdefault("random_state", 7)
        return NNDescent(x, metric="euclidean", **kw)

    def show(name, what, *arrays):
        print("%s\t%s\t%s" % (name, what, digest(*arrays)), flush=True)

    x = rows(3000, 17, 1)
    a = graph(x)
    show("a", "n 3000, d 17, k 10: no routing", *a.neighbor_graph)
    show("b", "a with k 70: wide rows, three sub-steps", *graph(x, n_neighbors=70).neighbor_graph)
    show("c", "a with max_candidates 65: blocked join, mcp 128", *graph(x, max_candidates=65).neighbor_graph)
    xd = rows(131072, 8, 2)
    show("d", "n 131072, d 8, k 10, 2 trees: routing on", *graph(xd, n_trees=2).neighbor_graph)
    show("e", "d with n 131071: routing off", *graph(xd[:131071], n_trees=2).neighbor_graph)
    graph(x, random_state=11)
    show("f", "a twice in a row, seeds 11 and 12, second build: a re-armed parked handle", *graph(x, random_state=12).neighbor_graph)
    show("g", "then a with d 24: the parked handle of another geometry released", *graph(rows(3000, 24, 3)).neighbor_graph)
    show("h", "a from a float16 device tensor", *graph(torch.from_numpy(x).to("cuda:0", torch.float16)).neighbor_graph)
    show("i", "a with init_graph from a's result", *graph(x, init_graph=a.neighbor_graph[0]).neighbor_graph)
    a.update(xs_fresh=rows(100, 17, 4))
    show("j", "a.update() with 100 fresh rows", *a.neighbor_graph)
    show("k", "a through nnd_build: the copies below their staging thresholds", *via_nnd_build(_capi, x, 10, 4, 5))
    show("l", "1 M x 128 float32 through nnd_build: the staged copies", *via_nnd_build(_capi, rows(1000000, 128, 6), 15, 8, 9))


def compare(parent_path, new_path):
    parent, new = ([ln.rstrip("\n").split("\t") for ln in open(p) if ln.count("\t") == 2] for p in (parent_path, new_path))
    assert [r[:2] for r in parent] == [r[:2] for r in new], "the two runs list different cases"
    print("%-4s %-80s %-32s %-32s" % ("case", "what", "parent", "new"))
    equal = 0
    for (name, what, dp), (_, _, dn) in zip(parent, new):
        equal += dp == dn
        print("%-4s %-80s %s %s %s" % (name, what, dp, dn, "equal" if dp == dn else "DIFFERENT"))
    print("\n%d of %d digests equal." % (equal, len(parent)))
    return 0 if equal == len(parent) else 1


if __name__ == "__main__":
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1:2] == ["--compare"] else run())
