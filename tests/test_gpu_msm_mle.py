"""The reversible maximum-likelihood builder on the device (builders.mle,
enspara_amd/csrc/ek_msm_mle.hip) against the plain numpy restatement of
tests/_numpy_prinz.py and against outputs of the real reference
(tests/golden/mle_golden.npz, written by tests/golden/make_mle_golden.py).

The kernel runs a sweep's pair updates level by level instead of one after the
other; the level order keeps every two updates that share a state in their
sequential order, so X and X_rs must be the sequential sweep's BIT FOR BIT -- that
is what the fixed-sweep tests ask, at the sizes where the kernel changes shape: the
a == 0 branch, compressed levels with dropped pairs, a level wider than a wave
(n = 130) and wider than the workgroup (n = 2100), row sums that need more LDS than a
launch gets by default (n = 3200), den == 0 on the diagonal, a zero
diagonal, counts that are no integers, and the row sums in global memory instead of
LDS.  No expected value comes from a device call.

logl decides the stop and is summed in the device's own (fixed) order:
|logl_dev - logl_ref| <= (P + 8) eps sum|term| for its P terms -- the worst case of
reordering a sum of P terms plus a few ulp per term for log and the division."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]
import _numpy_prinz as npz  # noqa: E402
from enspara_amd.exception import ConvergenceWarning  # noqa: E402
from enspara_amd.msm import MSM, builders  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
TABLE3 = np.array([[0, 2, 8], [4, 2, 4], [7, 3, 0]])    # the reference's own test table


def _self_count_only():
    C = npz.dense_counts(7, seed=11)
    C[2, :] = 0
    C[2, 2] = 9             # den = C_rs[2] - C[2,2] == 0
    return C


def _zero_diagonal():
    C = npz.dense_counts(7, seed=12)
    C[np.arange(7), np.arange(7)] = 0
    return C


# name -> (counts, restatement form, sweeps to run)
CASES = {
    "n2_a0": (lambda: np.array([[0., 3.], [5., 0.]]), "sequential", (1, 5)),
    "n3_table": (lambda: TABLE3.astype(np.float64), "sequential", (1, 5)),
    "n7_dense": (lambda: npz.dense_counts(7, seed=7), "sequential", (1, 5)),
    "n33_sparse": (lambda: npz.sparse_counts(33, 0.15, seed=2), "sequential", (1, 5)),
    "n130_dense": (lambda: npz.dense_counts(130, seed=13), "levelled", (1, 5)),
    "n2100_dense": (lambda: npz.dense_counts(2100, seed=21), "levelled", (2,)),
    # (16 n bytes of row sums > 48 KiB: the LDS form beyond the default dynamic limit)
    "n3200_sparse": (lambda: npz.sparse_counts(3200, 0.0005, seed=32), "levelled", (2,)),
    "den0": (_self_count_only, "sequential", (1, 5)),
    "zero_diag": (_zero_diagonal, "sequential", (1, 5)),
    "prior_frac": (lambda: builders._apply_prior_counts(
        npz.sparse_counts(12, 0.4, seed=5), 0.37), "sequential", (1, 5)),
}
FIXED = [(name, k) for name, (_, _, ks) in CASES.items() for k in ks]


@functools.lru_cache(maxsize=None)
def _counts(name):
    C = CASES[name][0]()
    C.setflags(write=False)
    return C


@functools.lru_cache(maxsize=None)
def _want(name, sweeps, tol=-1.0):
    """numpy only"""
    return getattr(npz, CASES[name][1])(_counts(name), sweeps, tol=tol)


def _device(C, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        return builders._prinz_mle_full(C, **kw)


def _check_fixed(name, sweeps, **kw):
    want = _want(name, sweeps)
    T, pi, X, X_rs, n_iter, logl = _device(_counts(name), tol=-1.0, max_iter=sweeps, **kw)
    assert n_iter == sweeps == want["n_iter"]
    assert np.array_equal(X, want["X"])
    assert np.array_equal(X_rs, want["X_rs"])
    bound = (want["P"][-1] + 8) * EPS * want["abs"][-1]
    print("%s sweeps %d: |logl_dev - logl_ref| = %.3g, bound %.3g"
          % (name, sweeps, abs(logl - want["logl"][-1]), bound))
    assert abs(logl - want["logl"][-1]) <= bound
    Tw, piw = npz.finish(want["X"], want["X_rs"])
    assert np.array_equal(T, Tw) and np.array_equal(pi, piw)


@pytest.mark.parametrize("name,sweeps", FIXED, ids=["%s-%d" % c for c in FIXED])
def test_fixed_sweeps_are_the_sequential_sweeps_bit_for_bit(name, sweeps):
    _check_fixed(name, sweeps)


@pytest.mark.parametrize("name,sweeps", [("n33_sparse", 5), ("n130_dense", 5),
                                         ("den0", 1)])
def test_row_sums_in_global_memory(name, sweeps):
    _check_fixed(name, sweeps, _force_global=True)


@pytest.mark.parametrize("name", ["n7_dense", "n33_sparse"])
def test_logl_of_every_sweep(name):
    want = _want(name, 5)
    for k in range(1, 6):
        logl = _device(_counts(name), tol=-1.0, max_iter=k)[5]
        assert abs(logl - want["logl"][k - 1]) <= \
            (want["P"][k - 1] + 8) * EPS * want["abs"][k - 1]


@pytest.mark.parametrize("name,form", [("n7_dense", "sequential"),
                                       ("n33_sparse", "levelled"),
                                       ("n3_table", "sequential")])
def test_default_stop(name, form):
    C = _counts(name)
    own = getattr(npz, form)(C, 10**5, tol=1e-10)
    T, pi, X, X_rs, n_iter, logl = builders._prinz_mle_full(C)
    print("%s: device stops after %d sweeps, the restatement after %d"
          % (name, n_iter, own["n_iter"]))
    assert abs(n_iter - own["n_iter"]) <= 2
    same = getattr(npz, form)(C, n_iter)
    assert np.array_equal(X, same["X"])
    assert np.array_equal(X_rs, same["X_rs"])


def test_two_runs_give_the_same_bits():
    C = _counts("n33_sparse")
    a = builders._prinz_mle_full(C)
    b = builders._prinz_mle_full(C)
    assert a[4] == b[4] and a[5] == b[5]
    for u, v in zip(a[:4], b[:4]):
        assert np.array_equal(u, v)


# ---- the public surface -------------------------------------------------------------
@pytest.mark.parametrize("arr_type", [np.array, scipy.sparse.csr_matrix,
                                      scipy.sparse.coo_matrix, scipy.sparse.lil_matrix])
@pytest.mark.parametrize("eq", [True, False])
def test_mle_types(arr_type, eq):
    """reference test_msm_funcs.py:225-258"""
    in_cts = arr_type(TABLE3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out_cts, out_probs, pops = builders.mle(in_cts, calculate_eq_probs=eq)
    assert type(in_cts) is type(out_probs) and type(in_cts) is type(out_cts)
    assert (pops is not None) == eq
    if scipy.sparse.issparse(out_probs):
        out_probs, out_cts = out_probs.toarray(), out_cts.toarray()
    assert np.array_equal(out_cts, TABLE3)
    assert np.array_equal(np.round(out_probs, decimals=1),
                          np.array([[0.0, 0.2, 0.8], [0.4, 0.2, 0.4], [0.7, 0.3, 0.0]]))


def test_mle_not_in_place():
    """reference test_msm_funcs.py:261-269"""
    in_cts = TABLE3.copy()
    out_cts, _, _ = builders.mle(in_cts, prior_counts=10)
    assert np.array_equal(in_cts, TABLE3)
    assert np.array_equal(out_cts, TABLE3 + 10)
    sp = scipy.sparse.csr_matrix(TABLE3)
    builders.mle(sp)
    assert np.array_equal(sp.toarray(), TABLE3)


def test_warnings():
    with pytest.warns(RuntimeWarning, match="cannot suppress"):
        _, _, pops = builders.mle(TABLE3, calculate_eq_probs=False)
    assert pops is None
    with pytest.warns(ConvergenceWarning, match="did not converge after 2"):
        builders._prinz_mle(TABLE3, max_iter=2)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        builders.mle(TABLE3)


def test_msm_fit_with_mle():
    rng = np.random.RandomState(3)
    assigns = np.empty((4, 300), dtype=np.int64)
    for t in range(4):
        s = rng.randint(6)
        for i in range(300):
            assigns[t, i] = s
            s = (s + rng.choice([-1, 0, 0, 1, 2])) % 6
    m = MSM(lag_time=2, method="mle", trim=True).fit(assigns)
    assert m.n_states_ == 6
    T = np.asarray(m.tprobs_.todense()) if scipy.sparse.issparse(m.tprobs_) \
        else np.asarray(m.tprobs_)
    assert np.all(np.abs(T.sum(axis=1) - 1.0) <= 4 * EPS)
    assert abs(m.eq_probs_.sum() - 1.0) <= 4 * EPS
    # detailed balance, within what the reference itself still moves after its stop
    g = _golden()
    atol = max(float(g["atol_" + c]) for c in g["cases"])
    F = m.eq_probs_[:, None] * T
    assert np.all(np.abs(F - F.T) <= atol)
    # the fit is the restatement's, run for as many sweeps
    C = m.tcounts_.toarray() if scipy.sparse.issparse(m.tcounts_) \
        else np.asarray(m.tcounts_)
    n_iter = builders._prinz_mle_full(C)[4]
    want = npz.sequential(C, n_iter)
    Tw, piw = npz.finish(want["X"], want["X_rs"])
    assert np.array_equal(T, Tw) and np.array_equal(m.eq_probs_, piw)


# ---- the real reference -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(HERE, "golden", "mle_golden.npz"))


@pytest.mark.parametrize("case", ["n3_dense", "n3_sparse", "n12_dense", "n12_sparse",
                                  "n40_dense", "n40_sparse"])
def test_against_the_reference(case):
    g = _golden()
    assert sorted(g["cases"]) == ["n12_dense", "n12_sparse", "n3_dense", "n3_sparse",
                                  "n40_dense", "n40_sparse"]
    C = g["C_" + case]
    atol = float(g["atol_" + case])
    assert atol < 1e-9
    if case.endswith("sparse"):
        C = scipy.sparse.csr_matrix(C)
    Cout, T, pi = builders.mle(C)
    assert type(T) is type(C)
    if scipy.sparse.issparse(T):
        T = T.toarray()
    print("%s: max |T - T_ref| = %.3g, max |pi - pi_ref| = %.3g, atol %.3g"
          % (case, np.abs(T - g["T_" + case]).max(), np.abs(pi - g["pi_" + case]).max(),
             atol))
    assert np.all(np.abs(T - g["T_" + case]) <= atol)
    assert np.all(np.abs(pi - g["pi_" + case]) <= atol)
