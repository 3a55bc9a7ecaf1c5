"""Graph export on the GPU, instance by instance (csrc/csr_graph.hip): every sort width of the symmetric merge, the long-row
kernel at several lengths and with more rows than workgroups, every k_csr_write_rows instance with both id types, the row
stride, ids outside [0, n) and values of every sign -- each against the host model of tests/graph_export_util.py bit for bit.
What a case reaches is asserted without a GPU in tests/test_graph_export_cpu.py; the cases are tests/graph_export_cases.py."""
import numpy as np
import pytest

from pynndescent_amd import _capi
from tests import graph_export_cases as GC
from tests.graph_export_util import assert_same_csr, model_csr

pytestmark = pytest.mark.gpu

FORMS = [(mode, drop_self) for mode in ("distance", "connectivity") for drop_self in (False, True)]


def _long_rows(ids, n, k):
    return GC.instance_counts(ids, n, k)[-1]


# ------------------------------------------------------------------------------------------------ 1. symmetric form
@pytest.mark.parametrize("which", GC.VALUE_SETS)
@pytest.mark.parametrize("name", sorted(GC.SYMMETRIC))
def test_symmetric_case_equals_the_model(name, which):
    case, ids, vals = GC.SYMMETRIC[name], GC.sym_lists(name), GC.sym_values(name, which)
    counts = GC.instance_counts(ids, case.n, case.k)
    print("%s: rows per merge instance %s = %s" % (name, list(GC.MERGE_INSTANCES), counts))
    for mode, drop_self in FORMS:
        got = _capi.graph_csr(ids, vals, case.n, mode=mode, symmetric=True, drop_self=drop_self, want_long_rows=True)
        assert_same_csr(got[:3], model_csr(ids, vals, case.n, mode=mode, symmetric=True, drop_self=drop_self))
        assert got[3] == counts[-1], (mode, drop_self)


@pytest.mark.parametrize("name", ["boundaries_k15", "many_long_k256"])
def test_symmetric_case_is_deterministic(name):
    case, ids, vals = GC.SYMMETRIC[name], GC.sym_lists(name), GC.sym_values(name, "signed")
    first = _capi.graph_csr(ids, vals, case.n, symmetric=True, want_long_rows=True)
    second = _capi.graph_csr(ids, vals, case.n, symmetric=True, want_long_rows=True)  # (the scatter order may differ between runs)
    for a, b in zip(first[:3], second[:3]):
        assert a.tobytes() == b.tobytes()
    assert first[3] == second[3] == _long_rows(ids, case.n, case.k)


# ------------------------------------------------------------------------------------------------ 2. directed form
@pytest.mark.parametrize("m,k,n,id_dtype,empty", GC.DIRECTED, ids=["%dx%d_%s" % (c[0], c[1], np.dtype(c[3]).name) for c in GC.DIRECTED])
def test_directed_case_equals_the_model(m, k, n, id_dtype, empty):
    ids, vals = GC.directed_lists(m, k, n, id_dtype, empty)
    print("k = %d, %s: k_csr_write_rows<%d, %d>" % ((k, ids.dtype.name) + GC.write_instance(k)))
    for mode, drop_self in FORMS:
        assert_same_csr(_capi.graph_csr(ids, vals, n, mode=mode, drop_self=drop_self), model_csr(ids, vals, n, mode=mode, drop_self=drop_self))
    if not empty:
        assert _capi.graph_csr(ids, vals, n)[0].tolist() == list(range(0, m * k + 1, k))  # every place of every row is filled


# ------------------------------------------------------------------------------------------------ 3. row stride
def _device_csr(ids, vals, k, n, **kwargs):
    """_capi.DeviceCsr on the first k columns of the (m, ld) host arrays, uploaded as they are; the three arrays and long_rows."""
    import torch

    t_ids, t_vals = torch.from_numpy(np.ascontiguousarray(ids)).cuda(), torch.from_numpy(np.ascontiguousarray(vals)).cuda()
    torch.cuda.synchronize()
    m, ld = ids.shape
    csr = _capi.DeviceCsr(0, 0, t_ids.data_ptr(), t_ids.element_size(), t_vals.data_ptr(), m, k, ld, n, **kwargs)
    assert csr.nnz > 0
    parts = tuple(torch.as_tensor(b, device=t_ids.device).cpu().numpy() for b in (csr.indptr, csr.indices, csr.data))
    return parts + (csr.long_rows,)


def _padded(ids, vals, ld, n):
    """(m, ld) arrays whose columns from k on hold ids that are valid columns and values that are NaN."""
    m, k = ids.shape
    rs = np.random.RandomState(ld)
    wide_ids = np.concatenate([ids, rs.randint(0, n, size=(m, ld - k)).astype(ids.dtype)], axis=1)
    wide_vals = np.concatenate([vals, np.full((m, ld - k), np.nan, np.float32)], axis=1)
    return wide_ids, wide_vals


@pytest.mark.parametrize("m,k,n,id_dtype", [(131, 16, 200, np.int32), (131, 17, 200, np.int64), (129, 33, 200, np.int32), (66, 100, 300, np.int64),
                                            (35, 200, 500, np.int32)])
def test_directed_form_reads_k_columns_of_a_wider_row(m, k, n, id_dtype):
    ids, vals = GC.directed_lists(m, k, n, id_dtype, 0.15)
    for ld in (k + 3, 2 * k):
        wide_ids, wide_vals = _padded(ids, vals, ld, n)
        for mode, drop_self in (("distance", False), ("distance", True)):
            got = _device_csr(wide_ids, wide_vals, k, n, mode=mode, drop_self=drop_self)
            assert not np.isnan(got[2]).any()
            assert_same_csr(got[:3], model_csr(ids, vals, n, mode=mode, drop_self=drop_self))


@pytest.mark.parametrize("name", ["boundaries_k15", "wide_k100"])
def test_symmetric_form_reads_k_columns_of_a_wider_row(name):
    case, ids, vals = GC.SYMMETRIC[name], GC.sym_lists(name), GC.sym_values(name, "signed")
    want = model_csr(ids, vals, case.n, symmetric=True)
    for ld in (case.k + 3, 2 * case.k):
        wide_ids, wide_vals = _padded(ids, vals, ld, case.n)
        got = _device_csr(wide_ids, wide_vals, case.k, case.n, symmetric=True)
        assert not np.isnan(got[2]).any()
        assert_same_csr(got[:3], want)
        assert got[3] == _long_rows(ids, case.n, case.k)


# ------------------------------------------------------------------------------------------------ 4. ids that name no column
def _with_strays(ids, n, seed):
    """A tenth of the places overwritten with ids outside [0, n), and row 1 holding nothing else; returns (ids, the same lists
    with those places -1).  Every kernel reads an id through csr_col alone, which checks it against n before it is used."""
    rs = np.random.RandomState(seed)
    strays = [n, n + 5, 2 ** 31 - 1, -7]
    if ids.dtype == np.int64:
        strays += [2 ** 32 + 3, -2 ** 40]  # (2^32 + 3: column 3 after a narrowing cast)
    strays = np.asarray(strays, ids.dtype)
    hit = rs.random_sample(ids.shape) < 0.1
    hit[1] = True
    out = np.where(hit, strays[rs.randint(0, strays.shape[0], size=ids.shape)], ids).astype(ids.dtype)
    assert all((out == s).any() for s in strays)
    return out, np.where(hit, -1, ids).astype(ids.dtype)


@pytest.mark.parametrize("m,k,n,id_dtype", [(131, 17, 200, np.int32), (66, 100, 300, np.int64)])
def test_directed_form_takes_an_id_outside_the_columns_as_empty(m, k, n, id_dtype):
    ids, vals = GC.directed_lists(m, k, n, id_dtype, 0.15)
    ids, cleaned = _with_strays(ids, n, seed=k)
    for drop_self in (False, True):
        got = _capi.graph_csr(ids, vals, n, drop_self=drop_self)
        assert_same_csr(got, model_csr(cleaned, vals, n, drop_self=drop_self))
        assert_same_csr(got, model_csr(ids, vals, n, drop_self=drop_self))
        assert got[0][2] == got[0][1]  # row 1 is empty


@pytest.mark.parametrize("name", ["boundaries_k15", "wide_k100"])
def test_symmetric_form_takes_an_id_outside_the_columns_as_empty(name):
    case, vals = GC.SYMMETRIC[name], GC.sym_values(name, "signed")
    ids, cleaned = _with_strays(GC.sym_lists(name), case.n, seed=case.k)
    for drop_self in (False, True):
        got = _capi.graph_csr(ids, vals, case.n, symmetric=True, drop_self=drop_self, want_long_rows=True)
        assert_same_csr(got[:3], model_csr(cleaned, vals, case.n, symmetric=True, drop_self=drop_self))
        assert got[3] == _long_rows(cleaned, case.n, case.k)


# ------------------------------------------------------------------------------------------------ 5. class level, wide lists
WN, WK = 600, 70


@pytest.fixture(scope="module")
def wide_indexes():
    """(host index, device index) with n_neighbors = 70 on the same 600 x 8 rows."""
    import torch

    from pynndescent_amd import NNDescent

    x = np.random.RandomState(9).standard_normal((WN, 8)).astype(np.float32)
    return NNDescent(x, n_neighbors=WK, random_state=0), NNDescent(torch.from_numpy(x).cuda(), n_neighbors=WK, random_state=0)


def _lists(index):
    ids, vals = index.neighbor_graph
    if hasattr(ids, "cpu"):
        ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
    return ids, vals.astype(np.float32)


def _check_wide(index, parts):
    ids, vals = _lists(index)
    assert ids.shape == (WN, WK)
    assert_same_csr(parts(index.kneighbors_graph()), model_csr(ids, vals, WN))
    assert_same_csr(parts(index.kneighbors_graph(k=20)), model_csr(ids[:, :20], vals[:, :20], WN))
    assert_same_csr(parts(index.kneighbors_graph(symmetric=True)), model_csr(ids, vals, WN, symmetric=True))
    assert_same_csr(parts(index.kneighbors_graph(k=20, symmetric=True)), model_csr(ids[:, :20], vals[:, :20], WN, symmetric=True))


def test_kneighbors_graph_of_a_host_index_with_wide_lists(wide_indexes):
    _check_wide(wide_indexes[0], lambda a: (a.indptr, a.indices, a.data))


def test_kneighbors_graph_of_a_device_index_with_wide_lists(wide_indexes):
    # (k = 20 reads the first 20 columns of the graph's rows of 70 where they lie: ld = 70)
    _check_wide(wide_indexes[1], lambda t: (t.crow_indices().cpu().numpy(), t.col_indices().cpu().numpy(), t.values().cpu().numpy()))
