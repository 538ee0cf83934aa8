"""The MSM count and row-normalise kernels (enspara_amd/csrc/ek_msm.hip) through the C
ABI against the plain numpy reference of tests/_numpy_msm.py (itself pinned to the
real reference's outputs and to scipy by tests/test_msm_reference.py), at the shapes
where hand-written integer kernels go wrong: frame counts round the 1024 of a
compaction workgroup, -1 runs across and over whole workgroups, trajectory starts on
and off the histogram's 4096-position blocks, 15 to 18 starts inside one block (16 are
staged in LDS, a position behind them searches), lags that leave the block, both window
forms, cells in the table's corners and beyond 2^31, and both histogram forms
(EK_MSM_HIST_LDS is read once per process: the second form runs in one child).

No expected value here comes from a device call: every `want` is numpy's.

The row normalisation is compared bit for bit with the sequential float64 formula
(builders.py:188-196 through scipy's CSR row sum), and with the same in long double
to a bound that follows from its operations: len - 1 additions of positive terms, one
reciprocal, one product, each within u = 2^-53 -> (len + 2) u relative."""
import ctypes as C
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]     # (the child process runs this file)
import _numpy_msm as nm  # noqa: E402
from enspara_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
SENTINEL = -77


@functools.lru_cache(maxsize=None)
def _want(name):
    """(case, reference COO): numpy only"""
    case = nm.make_case(name)
    return case, nm.reference_of(case)


def _abi_counts(flat, lengths, lag, sliding, K, capacity=None, pad=0):
    """ek_msm_counts -> (rc, nnz, rows, cols, counts); the arrays are `pad` entries
    longer than the capacity handed over and pre-filled with SENTINEL"""
    L = _lib.load()
    flat = np.ascontiguousarray(flat, dtype=np.int32)
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    cap = max(1, min(len(flat), K * K)) if capacity is None else capacity
    rows = np.full(cap + pad, SENTINEL, dtype=np.int32)
    cols = np.full(cap + pad, SENTINEL, dtype=np.int32)
    vals = np.full(cap + pad, SENTINEL, dtype=np.int64)
    nnz = C.c_int64(SENTINEL)
    rc = L.ek_msm_counts(0, _lib.i32p(flat), _lib.i64p(lengths), len(lengths), lag,
                         1 if sliding else 0, K, cap, _lib.i32p(rows), _lib.i32p(cols),
                         _lib.i64p(vals), C.byref(nnz))
    return rc, nnz.value, rows, cols, vals


def _assert_coo(got, want, what):
    rc, nnz, rows, cols, vals = got
    r, c, v = want
    assert rc == _lib.EK_OK, (what, rc, _lib.load().ek_last_error())
    assert nnz == len(r), (what, nnz, len(r))
    # entry by entry: the (row, col) order of the output is part of the contract
    np.testing.assert_array_equal(rows[:nnz], r, err_msg=what)
    np.testing.assert_array_equal(cols[:nnz], c, err_msg=what)
    np.testing.assert_array_equal(vals[:nnz], v, err_msg=what)


def _huge_table_fits():
    import torch
    return torch.cuda.mem_get_info()[0] >= 12e9


# states outside [0, K): (name, flat, lengths, lag, sliding, K), each must give EK_EARG
def _bad_state_cases():
    out = []
    for bad, tag in ((5, "K"), (-2, "minus2")):
        out.append(("from_%s" % tag, [0, 1, bad, 1, 0, 2], [6], 1, True, 5))
        out.append(("to_only_%s" % tag, [0, 1, 1, 2, 3, bad], [6], 1, True, 5))
        out.append(("to_only_stride_%s" % tag, [0, 1, 1, 2, bad], [5], 2, False, 5))
        # a trajectory shorter than the lag: its frames are in no transition
        out.append(("no_transition_%s" % tag, [bad, 0, 1, 2, 3, 4, 0, 1], [2, 6], 3,
                    True, 5))
        # ... and a frame the stride steps over
        out.append(("stepped_over_%s" % tag, [0, bad, 1, 3, 2], [5], 2, False, 5))
    return out


# ---- counts, the default histogram form, in this process -------------------------------
@pytest.mark.parametrize("name", nm.case_names())
def test_counts_equal_the_reference(name):
    if name == "K46341" and not _huge_table_fits():
        pytest.skip("less than 12 GB of device memory free for the 8.6 GB table")
    case, want = _want(name)
    got = _abi_counts(case.flat, case.lengths, case.lag, case.sliding, case.K)
    _assert_coo(got, want, name)
    assert (got[1] == 0) == (name in nm.NO_TRANSITIONS)


@pytest.mark.parametrize("case", _bad_state_cases(), ids=lambda c: c[0])
def test_a_state_outside_the_table_is_an_error(case):
    name, flat, lengths, lag, sliding, K = case
    rc = _abi_counts(flat, lengths, lag, sliding, K)[0]
    assert rc == _lib.EK_EARG, name


def test_capacity_is_respected():
    case, want = _want("states_31")
    nnz = len(want[0])
    assert nnz > 100
    rc, _, rows, cols, vals = _abi_counts(case.flat, case.lengths, case.lag, case.sliding,
                                          case.K, capacity=nnz - 1, pad=200)
    assert rc == _lib.EK_EARG
    for a in (rows, cols, vals):
        assert np.all(a[nnz - 1:] == SENTINEL)
    got = _abi_counts(case.flat, case.lengths, case.lag, case.sliding, case.K,
                      capacity=nnz, pad=200)
    _assert_coo(got, want, "capacity = nnz")
    for a in got[2:]:
        assert np.all(a[nnz:] == SENTINEL)


# ---- the form that gathers in LDS: the same grid in one child process ----------------------
def _child(path, with_huge):
    out = {}
    for name in nm.case_names():
        if name == "K46341" and not with_huge:
            continue
        case = nm.make_case(name)
        rc, nnz, rows, cols, vals = _abi_counts(case.flat, case.lengths, case.lag,
                                                case.sliding, case.K)
        k = max(nnz, 0)
        out[name + "__rc"], out[name + "__nnz"] = rc, nnz
        out[name + "__rows"], out[name + "__cols"], out[name + "__vals"] = \
            rows[:k], cols[:k], vals[:k]
    for case in _bad_state_cases():
        out["bad__" + case[0]] = _abi_counts(*case[1:])[0]
    np.savez(path, **out)


def test_counts_gathered_in_lds_equal_the_reference(tmp_path):
    """msm_hist_lds_kernel over the whole grid, plus lds_probe_wraps, the case made
    for its table: ten cells hashing to slots 8190 and 8191"""
    env = dict(os.environ)
    env["EK_MSM_HIST_LDS"] = "1"
    path = str(tmp_path / "lds.npz")
    huge = _huge_table_fits()
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path, str(int(huge))],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    Z = np.load(path)
    failed = []
    for name in nm.case_names():
        if name == "K46341" and not huge:
            continue
        got = (int(Z[name + "__rc"]), int(Z[name + "__nnz"]), Z[name + "__rows"],
               Z[name + "__cols"], Z[name + "__vals"])
        try:
            _assert_coo(got, _want(name)[1], name)
        except AssertionError as e:
            failed.append("%s: %s" % (name, str(e)[:300]))
    for case in _bad_state_cases():
        if int(Z["bad__" + case[0]]) != _lib.EK_EARG:
            failed.append("bad/%s: rc %d" % (case[0], int(Z["bad__" + case[0]])))
    assert not failed, "\n".join(failed)


# ---- the labels resident in a context, its scratch growing and shrinking ----------------------
def _ctx_counts(st, lengths, lag, sliding, K):
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    cap = max(1, min(st.n, K * K))
    rows = np.full(cap, SENTINEL, dtype=np.int32)
    cols = np.full(cap, SENTINEL, dtype=np.int32)
    vals = np.full(cap, SENTINEL, dtype=np.int64)
    nnz = C.c_int64(SENTINEL)
    rc = st.lib.ek_msm_counts_ctx(st._h, _lib.i64p(lengths), len(lengths), lag,
                                  1 if sliding else 0, K, cap, _lib.i32p(rows),
                                  _lib.i32p(cols), _lib.i64p(vals), C.byref(nnz))
    return rc, nnz.value, rows, cols, vals


def test_counts_over_resident_labels_as_the_scratch_grows_and_shrinks():
    """one context, a sequence of counts whose table (K 50 -> 700 -> 3 -> 2000 -> 3),
    trajectory count (1 -> 5000 -> 2 -> 1) and lag (1 -> 4097 -> 1) go up and down, a
    failing call in between: every one equals the reference, nothing of a larger call
    (table, per-workgroup counts and offsets, trajectory starts) shows in a smaller"""
    from enspara_amd.device import FrameStore
    n = 30000
    rng = np.random.RandomState(77)
    many = rng.multinomial(n, np.ones(5000) / 5000)
    many[::13] += many[1::13][:len(many[::13])]        # some empty, the sum kept
    many[1::13] = 0
    assert many.sum() == n
    steps = [
        # (K, lengths, lag, sliding, share of -1)
        (50, [n], 1, True, 0.01),
        (700, many, 2, False, 0.05),
        (700, many, 1, True, 0.05),
        (3, [n - 1, 1], 4097, True, 0.3),
        (2000, [n // 2, n - n // 2], 1, True, 0.0),
        ("bad", [n], 1, True, 0.0),
        (3, [n], 1, True, 0.0),
        (50, [7, 0, n - 7], 40, False, 0.5),
    ]
    with FrameStore.from_array(np.zeros((n, 1, 3), dtype=np.float32)) as st:
        for i, (K, lengths, lag, sliding, gaps) in enumerate(steps):
            bad = K == "bad"
            K = 50 if bad else K
            labels = nm._walk(rng, n, K, band=3, gaps=gaps).astype(np.int32)
            if bad:
                labels[n // 2] = K
            st.upload_state(np.zeros(n, dtype=np.float32), labels)
            got = _ctx_counts(st, lengths, lag, sliding, K)
            if bad:
                assert got[0] == _lib.EK_EARG
                continue
            _assert_coo(got, nm.counts_ref(labels, lengths, lag, sliding, K),
                        "step %d" % i)
            assert got[1] > 0


# ---- row normalisation ---------------------------------------------------------------------------
ROW_LENGTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 5000]


def _values(kind, rng, n):
    if kind == "counts":
        return rng.poisson(3.0, size=n).astype(np.float64) + 1.0
    if kind == "prior":                 # counts plus the usual 1 / K
        return rng.poisson(0.7, size=n).astype(np.float64) + 1.0 / 5000
    if kind == "wide":                  # 2^-40 .. 2^40 inside every row
        return 2.0 ** rng.uniform(-40, 40, size=n)
    if kind == "stored_zeros":
        return rng.poisson(0.7, size=n).astype(np.float64)
    raise ValueError(kind)


def _rownorm_cases():
    """-> [(name, indptr int64, data float64, positive)]"""
    out = []
    for kind in ("counts", "prior", "wide", "stored_zeros"):
        rng = np.random.RandomState(nm.hash_name(kind))
        for tag, lens in (("", ROW_LENGTHS), ("_reversed", ROW_LENGTHS[::-1])):
            indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            out.append((kind + "_every_length" + tag, indptr, _values(kind, rng, indptr[-1]),
                        kind != "stored_zeros"))
    rng = np.random.RandomState(5)
    for n_rows in (1, 2, 3, 4, 5, 1001):
        lens = rng.choice([0, 1, 3, 17, 64, 65, 200], size=n_rows)
        lens[0] = 66
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        out.append(("rows_%d" % n_rows, indptr, _values("prior", rng, indptr[-1]), True))
    out.append(("empty_last_row", np.array([0, 5, 5, 12, 12], dtype=np.int64),
                _values("wide", rng, 12), True))
    out.append(("every_row_empty", np.zeros(7, dtype=np.int64), np.zeros(0), True))
    out.append(("zero_sum_rows", np.array([0, 3, 5, 6, 6, 70], dtype=np.int64),
                np.concatenate([[0.0, 0.0, 0.0, 2.0, 6.0, 0.0], np.zeros(64)]), False))
    out.append(("subnormal_sum", np.array([0, 3, 5, 70], dtype=np.int64),
                np.concatenate([[5e-324, 0.0, 1e-323, 2.0, 6.0], np.full(65, 5e-324)]),
                False))
    return out


def _abi_rownorm(indptr, data, with_rowsum):
    L = _lib.load()
    n_rows = len(indptr) - 1
    out = np.full(len(data) + 8, float(SENTINEL))
    rowsum = np.full(n_rows + 8, float(SENTINEL))
    rc = L.ek_msm_row_normalize(0, _lib.i64p(indptr), _lib.f64p(data), n_rows,
                                _lib.f64p(out), _lib.f64p(rowsum) if with_rowsum else None)
    assert rc == _lib.EK_OK, L.ek_last_error()
    assert np.all(out[len(data):] == SENTINEL) and np.all(rowsum[n_rows:] == SENTINEL)
    if not with_rowsum:
        assert np.all(rowsum == SENTINEL)
    return out[:len(data)], rowsum[:n_rows]


@pytest.mark.parametrize("with_rowsum", [False, True], ids=["rowsum_null", "rowsum_out"])
@pytest.mark.parametrize("case", _rownorm_cases(), ids=lambda c: c[0])
def test_row_normalize_equals_the_sequential_formula_bit_for_bit(case, with_rowsum):
    name, indptr, data, _ = case
    data = np.ascontiguousarray(data, dtype=np.float64)
    with np.errstate(all="ignore"):
        want, _ = nm.rownorm_ref(indptr, data)
    got, rowsum = _abi_rownorm(indptr, data, with_rowsum)
    np.testing.assert_array_equal(got, want)
    if with_rowsum:
        np.testing.assert_array_equal(rowsum, nm.rowsums_ref(indptr, data))
    if name == "subnormal_sum":
        assert np.isinf(got[0]) and np.isnan(got[1]) and np.all(np.isinf(got[5:]))
    if name == "zero_sum_rows":
        assert np.all(got[:3] == 0) and np.all(got[5:] == 0)


@pytest.mark.parametrize("case", [c for c in _rownorm_cases() if c[3]],
                         ids=lambda c: c[0])
def test_row_normalize_is_within_its_rounding_bound_of_the_truth(case):
    """positive data only: that is a condition of the bound (no cancellation in the
    row sum), the bit test above takes everything"""
    name, indptr, data, _ = case
    data = np.ascontiguousarray(data, dtype=np.float64)
    assert np.all(data > 0)
    _, truth = nm.rownorm_ref(indptr, data)
    got, _ = _abi_rownorm(indptr, data, False)
    lens = np.repeat(np.diff(indptr), np.diff(indptr))
    err = np.abs(got.astype(LD) - truth)
    bound = (lens + 2).astype(LD) * LD(U) * np.abs(truth)
    worst = float((err / bound).max()) if len(err) else 0.0
    print("%s: worst error / bound = %.3f" % (name, worst))
    assert np.all(err <= bound)


@pytest.mark.parametrize("K", [60, 1000])
def test_dense_normalize_with_a_fractional_prior(K):
    """builders.normalize(dense counts, prior_counts=1/K) against the reference's dense
    branch written out (builders.py:198-202): C * inv.reshape(K, 1) with C.sum(axis=1),
    numpy's pairwise row sum.  This project sums the CSR row in storage order, so the
    two are NOT bit-equal (on the CPU the two row sums already differ in 59 of 60 rows
    at K = 60, in all 1000 at K = 1000); both are within (K + 2) u of the long-double
    truth, which is what is asserted.  Largest distance measured between the device
    result and the reference formula, MI355X: 9 ulp at K = 60, 206 ulp at K = 1000."""
    from enspara_amd.msm import builders
    rng = np.random.RandomState(K)
    counts = rng.poisson(0.5, size=(K, K)).astype(np.float64)
    _, got, _ = builders.normalize(counts, prior_counts=1.0 / K, calculate_eq_probs=False)
    Cp = counts + 1.0 / K
    w = Cp.sum(axis=1)
    inv = np.zeros(K)
    inv[w > 0] = 1.0 / w[w > 0]
    formula = Cp * inv.reshape((K, 1))
    Cl = Cp.astype(LD)
    truth = Cl / Cl.sum(axis=1).reshape((K, 1))
    bound = LD(K + 2) * LD(U) * truth
    ulps = np.abs(got - formula) / np.spacing(formula)
    print("K = %d: device against the reference's dense formula: %d ulp at most, "
          "%d of %d entries differ" % (K, int(ulps.max()), int((ulps > 0).sum()), K * K))
    assert got.shape == (K, K) and isinstance(got, np.ndarray)
    assert np.all(np.abs(got.astype(LD) - truth) <= bound)
    assert np.all(np.abs(formula.astype(LD) - truth) <= bound)
    # and the device result is the sequential formula's, bit for bit
    indptr = np.arange(K + 1, dtype=np.int64) * K
    want, _ = nm.rownorm_ref(indptr, Cp.reshape(-1))
    np.testing.assert_array_equal(got.reshape(-1), want)


def test_long_double_is_wide():
    assert np.finfo(LD).eps <= 2.0 ** -63


if __name__ == "__main__":
    t0 = time.time()
    _child(sys.argv[1], sys.argv[2] == "1")
    print("child: %.1f s" % (time.time() - t0))
