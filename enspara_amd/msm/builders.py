"""Counts -> transition probabilities (reference enspara/msm/builders.py:
normalize :123-155, transpose :83-120, _row_normalize :171-204, mle :24-80 with
the iteration _prinz_mle_py :215-318)."""
import ctypes
import os
import warnings

import numpy as np
import scipy.sparse

from .. import _lib
from ..exception import ConvergenceWarning, DataInvalid


def _apply_prior_counts(C, prior_counts):
    """reference builders.py:158-168"""
    if prior_counts is not None:
        try:
            C = C + prior_counts
        except NotImplementedError:
            C = np.array(C.todense()) + prior_counts
    return C


def _row_normalize(C, device=0):
    """Row-normalise on the device; zero rows stay zero
    (reference builders.py:171-204).  Sparse in -> same sparse type out."""
    sparse_in = scipy.sparse.issparse(C)
    csr = scipy.sparse.csr_matrix(C).astype(np.float64)
    n = csr.shape[0]
    indptr = np.ascontiguousarray(csr.indptr, dtype=np.int64)
    data = np.ascontiguousarray(csr.data, dtype=np.float64)
    out = np.empty_like(data)
    L = _lib.load()
    _lib.check(L.ek_msm_row_normalize(int(device), _lib.i64p(indptr),
                                      _lib.f64p(data), n, _lib.f64p(out),
                                      None))
    T = scipy.sparse.csr_matrix((out, csr.indices, csr.indptr),
                                shape=csr.shape)
    if sparse_in:
        return type(C)(T)
    return np.asarray(T.todense())


def normalize(C, prior_counts=None, calculate_eq_probs=True, device=0):
    """reference builders.py:123-155"""
    from .transition_matrices import eq_probs
    C = _apply_prior_counts(C, prior_counts)
    probs = _row_normalize(C, device=device)
    equilibrium = None
    if calculate_eq_probs:
        equilibrium = eq_probs(probs, device=device)
    return C, probs, equilibrium


def transpose(C, prior_counts=None, calculate_eq_probs=True, device=0):
    """reference builders.py:83-120"""
    C = _apply_prior_counts(C, prior_counts)
    C_sym = C + C.T
    probs = _row_normalize(C_sym, device=device)
    if type(C) is not type(probs):
        probs = type(C)(probs)
        C_sym = type(C)(C_sym)
    equilibrium = None
    if calculate_eq_probs:
        equilibrium = np.array(C_sym.sum(axis=1) / C_sym.sum()).flatten()
    return C_sym / 2, probs, equilibrium


def _mle_schedule(C):
    """The order in which the device runs a sweep of Prinz's iteration over
    the dense count matrix ``C`` (reference builders.py:268-299).

    The reference updates the pairs (i, j), i < j, in lexicographic order.  An
    update touches X[i,j], X[j,i], X_rs[i] and X_rs[j] only, so a schedule
    that keeps the relative order of any two updates sharing a state computes
    the same bits.  Pairs with C[i,j] + C[j,i] == 0 stay exactly 0.0 and leave
    both row sums as they are (c = -0, sqrt(b*b) = |b|, v = 0): they are not
    scheduled.  The others get ``level = 1 + max(last[i], last[j])``, taken in
    lexicographic order, ``last[s]`` being the level of the latest earlier pair
    with state s (-1 if none): no two pairs of a level share a state, and every
    earlier pair that shares a state with a pair has a smaller level.  On a
    full pattern level(i, j) = i + j - 1.

    Returns ``(level_ptr, pair_i, pair_j, c_ij, c_ji, x_pairs)``, the pairs
    level-major (lexicographic inside a level), level l being
    ``[level_ptr[l], level_ptr[l + 1])``; ``x_pairs`` = C[i,j] + C[j,i].
    """
    C = np.asarray(C, dtype=np.float64)
    n = C.shape[0]
    S = C + C.T
    I, J = np.nonzero(np.triu(S > 0, 1))        # row-major = lexicographic
    # within row i: level_k = max(level_{k-1}, last[j_k]) + 1, level_{-1} = last[i]
    # <=> level_k - k = max(last[i] + 1, max_{t <= k}(last[j_t] + 1 - t))
    last = np.full(n, -1, dtype=np.int64)
    level = np.empty(len(I), dtype=np.int64)
    row_ptr = np.searchsorted(I, np.arange(n + 1))
    for i in range(n):
        lo, hi = row_ptr[i], row_ptr[i + 1]
        if lo == hi:
            continue
        js = J[lo:hi]
        k = np.arange(hi - lo)
        m = np.maximum.accumulate(last[js] + 1 - k)
        np.maximum(m, last[i] + 1, out=m)
        m += k
        level[lo:hi] = m
        last[js] = m
        last[i] = m[-1]
    n_levels = int(level.max()) + 1 if len(level) else 0
    order = np.argsort(level, kind="stable")
    level_ptr = np.zeros(n_levels + 1, dtype=np.int64)
    np.cumsum(np.bincount(level, minlength=n_levels), out=level_ptr[1:])
    I, J = I[order], J[order]
    return (level_ptr, I.astype(np.int32), J.astype(np.int32),
            np.ascontiguousarray(C[I, J]), np.ascontiguousarray(C[J, I]),
            np.ascontiguousarray(S[I, J]))


def _prinz_mle_full(C, tol=1e-10, max_iter=10**5, device=0, _force_global=False):
    """Prinz's iteration on the device -> ``(T, pi, X, X_rs, n_iter, logl)``:
    what ``_prinz_mle`` returns plus the iterate, its row sums, the number of
    sweeps that ran and the last sweep's ``logl``.  ``_force_global`` keeps the
    row sums in global memory whatever ``n`` (the form large ``n`` takes)."""
    C = np.array(C, dtype=np.float64)
    if C.ndim != 2 or C.shape[0] != C.shape[1] or C.shape[0] < 1:
        raise DataInvalid("a count matrix is square, not %s" % (C.shape,))
    if not np.all(np.isfinite(C)) or np.any(C < 0):
        raise DataInvalid("counts are finite and not negative")
    if max_iter < 1:
        raise DataInvalid("max_iter must be at least 1, not %s" % (max_iter,))
    n = C.shape[0]
    X = C + C.T
    X_rs = np.ascontiguousarray(X.sum(axis=1))
    C_rs = np.ascontiguousarray(C.sum(axis=1))
    # the reference's asserts (builders.py:250-251)
    for name, rs in (("C", C_rs), ("C + C.T", X_rs)):
        bad = np.flatnonzero(~(rs > 0))
        if len(bad):
            raise DataInvalid("row %d of %s sums to %r: mle needs every state "
                              "to have counts" % (bad[0], name, rs[bad[0]]))
    level_ptr, pi_, pj_, c_ij, c_ji, x_pairs = _mle_schedule(C)
    c_diag = np.ascontiguousarray(np.diagonal(C))
    x_diag = np.ascontiguousarray(np.diagonal(X))
    n_iter = ctypes.c_int64(0)
    logl = ctypes.c_double(0.0)
    L = _lib.load()
    saved = os.environ.get("EK_MSM_MLE_GLOBAL")
    if _force_global:
        os.environ["EK_MSM_MLE_GLOBAL"] = "1"
    try:
        _lib.check(L.ek_msm_mle_prinz(
            int(device), n, len(pi_), len(level_ptr) - 1, _lib.i64p(level_ptr),
            _lib.i32p(pi_), _lib.i32p(pj_), _lib.f64p(c_ij), _lib.f64p(c_ji),
            _lib.f64p(c_diag), _lib.f64p(C_rs), _lib.f64p(x_pairs),
            _lib.f64p(x_diag), _lib.f64p(X_rs), float(tol), int(max_iter),
            ctypes.byref(n_iter), ctypes.byref(logl)))
    finally:
        if _force_global:
            if saved is None:
                del os.environ["EK_MSM_MLE_GLOBAL"]
            else:
                os.environ["EK_MSM_MLE_GLOBAL"] = saved
    if n_iter.value >= max_iter:                            # builders.py:307-310
        warnings.warn("Prinz MLE did not converge after %d iterations."
                      % n_iter.value, category=ConvergenceWarning)
    X = np.zeros((n, n))
    X[pi_, pj_] = x_pairs
    X[pj_, pi_] = x_pairs
    X[np.arange(n), np.arange(n)] = x_diag
    # the reference's last two lines (:312-313), in numpy as there
    T = X / X.sum(axis=-1).reshape(n, 1)
    pi = X_rs / X_rs.sum()
    return T, pi, X, X_rs, n_iter.value, logl.value


def _prinz_mle(C, tol=1e-10, max_iter=10**5, device=0):
    """Reversible maximum-likelihood transition matrix of the dense counts
    ``C`` by Prinz's iteration (reference builders.py:215-318; Prinz et al.,
    J. Chem. Phys. 134, 174105 (2011)) -> ``(T, pi)``.

    All sweeps run in one launch on the device, in a level order that gives the
    reference's lexicographic sweep bit for bit (``_mle_schedule``).  Sweeps go
    on while ``|logl - oldlogl| > tol``, at most ``max_iter`` of them; reaching
    ``max_iter`` emits a ``ConvergenceWarning`` (the reference's call has its
    arguments swapped and raises instead).  The reference's closing asserts
    ``T.sum(axis=1) == 1`` and ``pi.sum() == 1`` (:315-316) are NOT made: they
    compare rounded sums for equality and fail on ordinary inputs."""
    return _prinz_mle_full(C, tol=tol, max_iter=max_iter, device=device)[:2]


def mle(C, prior_counts=None, calculate_eq_probs=True, device=0):
    """reference builders.py:24-80: counts -> (counts with pseudocounts,
    reversible maximum-likelihood transition probabilities, equilibrium
    populations).  Sparse input is densified for the iteration and ``C`` and
    ``T`` come back in its type.  The populations are a by-product of the
    iteration: ``calculate_eq_probs=False`` warns and returns ``None`` for
    them."""
    C = _apply_prior_counts(C, prior_counts)
    sparsetype = np.array
    if scipy.sparse.issparse(C):
        sparsetype = type(C)
        C = np.asarray(C.todense())
    equilibrium = None
    if not calculate_eq_probs:
        warnings.warn('MLE method cannot suppress calculation of '
                      'equilibrium probabilities, since they are calculated '
                      'together.', category=RuntimeWarning)
        T, _ = _prinz_mle(C, device=device)
    else:
        T, equilibrium = _prinz_mle(C, device=device)
    return sparsetype(C), sparsetype(T), equilibrium
