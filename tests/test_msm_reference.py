"""tests/_numpy_msm.py -- the plain reference tests/test_gpu_msm_oracle.py holds the MSM
kernels to -- pinned itself: to the real reference's recorded outputs
(tests/golden/msm_golden.npz, trim_golden.npz) and to the scipy construction the
reference uses, on every generated case of moderate size.  And the host-side argument
handling of assigns_to_counts, which needs no device."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _numpy_msm as nm  # noqa: E402


def _dense(coo, K):
    r, c, v = coo
    out = np.zeros((K, K), dtype=np.int64)
    out[r, c] = v
    return out


def _split(A):
    A = np.asarray(A)
    return A.reshape(-1), np.full(A.shape[0], A.shape[1], dtype=np.int64)


@pytest.fixture(scope="module")
def M(golden_dir):
    return np.load(os.path.join(golden_dir, "msm_golden.npz"))


def test_counts_ref_equals_the_reference_recorded_counts(M, golden_dir):
    flat, lengths = _split(M["assigns"])
    for lag in (1, 5):
        for sw in (0, 1):
            got = nm.counts_ref(flat, lengths, lag, bool(sw), 60)
            np.testing.assert_array_equal(_dense(got, 60),
                                          M["counts_lag%d_sw%d" % (lag, sw)])
            sp = nm.counts_ref_sparse(flat, lengths, lag, bool(sw), 60)
            for a, b in zip(got, sp):
                np.testing.assert_array_equal(a, b)
    lens = M["rag_lengths"]
    rag = np.concatenate([M["assigns"][i, :n] for i, n in enumerate(lens)])
    np.testing.assert_array_equal(_dense(nm.counts_ref(rag, lens, 3, True, 60), 60),
                                  M["rag_counts_lag3"])
    G = np.load(os.path.join(golden_dir, "trim_golden.npz"))
    flat, lengths = _split(G["assigns"])
    np.testing.assert_array_equal(_dense(nm.counts_ref(flat, lengths, 1, True, 40), 40),
                                  G["counts"])


def _scipy_counts(case):
    """the reference's construction (transition_matrices.py:156-170, :310-321): one COO
    entry of 1 per transition, summed by scipy"""
    rows, cols = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    lag = case.lag
    for a in np.split(case.flat, np.cumsum(case.lengths)[:-1]):
        a = a[np.where(a != -1)]
        if case.sliding:
            rows.append(a[:-lag:1])
            cols.append(a[lag::1])
        else:
            rows.append(a[:-lag:lag])
            cols.append(a[lag::lag])
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    C = scipy.sparse.coo_matrix((np.ones(len(rows), dtype=np.int64), (rows, cols)),
                                shape=(case.K, case.K)).tocsr()
    C.sum_duplicates()
    C.sort_indices()
    return C.tocoo()


@pytest.mark.parametrize("name", nm.case_names(large=False))
def test_counts_ref_equals_scipy_on_the_case_grid(name):
    case = nm.make_case(name)
    r, c, v = nm.counts_ref(case.flat, case.lengths, case.lag, case.sliding, case.K)
    assert r.dtype == c.dtype == v.dtype == np.int64
    want = _scipy_counts(case)
    np.testing.assert_array_equal(r, want.row)
    np.testing.assert_array_equal(c, want.col)
    np.testing.assert_array_equal(v, want.data)
    # sorted by (row, col), no duplicates, no stored zero
    cell = r * case.K + c
    assert np.all(np.diff(cell) > 0) and np.all(v > 0)
    sp = nm.counts_ref_sparse(case.flat, case.lengths, case.lag, case.sliding, case.K)
    for a, b in zip((r, c, v), sp):
        np.testing.assert_array_equal(a, b)


def test_the_case_grid_is_seeded_and_the_huge_case_hits_its_cells():
    a, b = nm.make_case("lag7_sw0"), nm.make_case("lag7_sw0")
    np.testing.assert_array_equal(a.flat, b.flat)
    empty = [n for n in nm.case_names(large=False)
             if len(nm.reference_of(nm.make_case(n))[0]) == 0]
    assert sorted(empty) == sorted(nm.NO_TRANSITIONS)
    case = nm.make_case("K46341")
    r, c, v = nm.reference_of(case)
    K = case.K
    cells = set(zip(r.tolist(), c.tolist()))
    assert {(46340, 41707), (46340, 41708), (46340, 46340), (0, 46340),
            (46340, 0)} <= cells
    assert (r * K + c).max() > 2 ** 31 and int(v.sum()) == len(case.flat) - 3
    # the cells made for the last two slots of the LDS table do hash there
    case = nm.make_case("lds_probe_wraps")
    r, c, v = nm.reference_of(case)
    slots = (((r * 300 + c) * 2654435761) % 2 ** 32) >> 19
    assert len(r) == 10 and set(slots.tolist()) == {8190, 8191}


def test_rownorm_ref_reproduces_the_reference_recorded_probabilities(M):
    C = scipy.sparse.csr_matrix(M["counts_lag1_sw1"]).astype(np.float64)
    C.sort_indices()
    for counts, key in ((C, "norm_T"), (scipy.sparse.csr_matrix(C + C.T), "transpose_T")):
        counts.sort_indices()
        bit, truth = nm.rownorm_ref(counts.indptr, counts.data)
        T = scipy.sparse.csr_matrix((bit, counts.indices, counts.indptr),
                                    shape=counts.shape)
        np.testing.assert_array_equal(np.asarray(T.todense()), M[key])
        assert np.all(np.abs(bit - truth) <= 2.0 ** -52 * truth)
    # rows that are empty, a sum of stored zeros, a subnormal sum
    indptr = np.array([0, 0, 2, 4, 6])
    data = np.array([0.0, 0.0, 1.0, 3.0, 5e-324, 5e-324])
    with np.errstate(all="ignore"):
        bit, truth = nm.rownorm_ref(indptr, data)
    np.testing.assert_array_equal(bit, [0, 0, 0.25, 0.75, np.inf, np.inf])
    np.testing.assert_array_equal(truth.astype(np.float64), [0, 0, 0.25, 0.75, 0.5, 0.5])
    np.testing.assert_array_equal(nm.rowsums_ref(indptr, data), [0, 0, 4, 1e-323])


# ---- host logic of assigns_to_counts: nothing here reaches the library -------------------
@pytest.fixture
def no_library(monkeypatch):
    from enspara_amd import _lib

    def load():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("lag", ["n", 2 ** 31 - 1, 2 ** 32 + 1, 2 ** 40])
def test_a_lag_no_trajectory_spans_gives_the_empty_matrix(no_library, lag):
    from enspara_amd.msm import assigns_to_counts
    from enspara_amd import ra
    a = np.random.RandomState(3).randint(5, size=(4, 100))
    lag = 100 if lag == "n" else lag
    for assigns in (a, ra.RaggedArray(a.reshape(-1), lengths=[100, 0, 60, 100, 40, 100])):
        for sliding in (True, False):
            for K in (None, 9):
                C = assigns_to_counts(assigns, lag_time=lag, max_n_states=K,
                                      sliding_window=sliding)
                want = 9 if K else 5
                assert scipy.sparse.isspmatrix_coo(C) and C.shape == (want, want)
                assert C.nnz == 0 and np.issubdtype(C.dtype, np.integer)


def test_a_lag_no_trajectory_spans_over_resident_labels(no_library):
    """the FrameStore branch: anything with msm_counts and n"""
    from enspara_amd.msm import assigns_to_counts

    class Store:
        n = 300

        def msm_counts(self, *a, **k):
            raise AssertionError("the library was asked for")
    for lag in (200, 2 ** 31 - 1, 2 ** 32 + 1, 2 ** 40):
        C = assigns_to_counts(Store(), lag, max_n_states=7, lengths=[100, 0, 200])
        assert C.shape == (7, 7) and C.nnz == 0 and np.issubdtype(C.dtype, np.integer)


def test_a_state_count_beyond_int32_raises(no_library):
    from enspara_amd.exception import DataInvalid
    from enspara_amd.msm import assigns_to_counts
    a = np.array([[0, 1, 2, 1, 0]])

    class Store:
        n = 5

        def msm_counts(self, *a, **k):
            raise AssertionError("the library was asked for")
    for K in (2 ** 31, 2 ** 32 + 3, 2 ** 40):
        with pytest.raises(DataInvalid):
            assigns_to_counts(a, lag_time=1, max_n_states=K)
        with pytest.raises(DataInvalid):
            assigns_to_counts(Store(), 1, max_n_states=K, lengths=[5])
