"""Plain-numpy restatement of enspara_amd.tpt (committors, mfpts, reactive_fluxes,
net_fluxes, reactive_populations) on an unblocked LU with first-index partial
pivoting, the test matrices, the error measures of the acceptance criteria and
a high-precision solver.  No device, no scipy solver: a second implementation
the goldens are checked against before the device is."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _numpy_bace as nb  # noqa: E402

U = 2.0 ** -53
LD = np.longdouble


# ---- the solver ---------------------------------------------------------------------
def lu_solve(A, B, return_gaps=False):
    """Gaussian elimination with partial pivoting (largest |a|, first row on
    ties) on [A | B], unblocked, then back substitution -> (X, pivots, info):
    pivots[k] = the row exchanged with row k, info = -1 or the first column with
    a zero or NaN pivot (that column is left as it is and the run goes on).

    return_gaps: -> (X, pivots, info, gaps) with gaps[k] = (m1 - m2) / m1, m1 >= m2
    the two largest |a| among step k's candidates: how far the choice of the pivot
    is from a tie (0 on a tie or a column of zeros; inf for a single candidate).
    Another summation order may choose another row only where this is rounding."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    B = np.array(B, dtype=np.float64)
    vector = B.ndim == 1
    M = np.concatenate([A, B.reshape(n, -1)], axis=1)
    piv = np.zeros(n, dtype=np.int32)
    gaps = np.full(n, np.inf)
    info = -1
    for k in range(n):
        p, gap = _pivot(M[k:, k], return_gaps)
        p += k
        piv[k], gaps[k] = p, gap
        if p != k:
            M[[k, p]] = M[[p, k]]
        pv = M[k, k]
        if pv == 0 or pv != pv:
            if info < 0:
                info = k
            continue
        l = M[k + 1:, k] / pv
        M[k + 1:, k] = l
        M[k + 1:, k + 1:] -= l[:, None] * M[k, k + 1:][None, :]
    X = M[:, n:]
    with np.errstate(all="ignore"):
        for k in range(n - 1, -1, -1):
            X[k] = X[k] / M[k, k]
            X[:k] -= M[:k, k][:, None] * X[k][None, :]
    X = np.ascontiguousarray(X)
    X = X[:, 0] if vector else X
    return (X, piv, info, gaps) if return_gaps else (X, piv, info)


def _pivot(col, want_gap=True):
    """(offset of the pivot in the candidates col, the relative gap to the runner-up)"""
    col = np.abs(col)
    col = np.where(np.isnan(col), np.inf, col)
    gap = np.inf
    if want_gap and len(col) > 1:
        m2, m1 = np.partition(col, len(col) - 2)[-2:]
        gap = (m1 - m2) / m1 if 0 < m1 < np.inf else 0.0
    return int(np.argmax(col)), gap


def leading_pivots(A, w):
    """(pivots, info, gaps) of lu_solve's first w steps, from A's first w columns
    alone (what is right of them changes no choice among them)"""
    M = np.array(np.asarray(A)[:, :w], dtype=np.float64)
    piv = np.zeros(w, dtype=np.int32)
    gaps = np.full(w, np.inf)
    info = -1
    for k in range(w):
        p, gaps[k] = _pivot(M[k:, k])
        p += k
        piv[k] = p
        if p != k:
            M[[k, p]] = M[[p, k]]
        pv = M[k, k]
        if pv == 0 or pv != pv:
            if info < 0:
                info = k
            continue
        l = M[k + 1:, k] / pv
        M[k + 1:, k] = l
        M[k + 1:, k + 1:] -= l[:, None] * M[k, k + 1:][None, :]
    return piv, info, gaps


def solve(A, B):
    X, _, info = lu_solve(A, B)
    if info >= 0:
        raise np.linalg.LinAlgError("zero pivot in column %d" % info)
    return X


# ---- the five functions ----------------------------------------------------------------
def _states(s):
    return np.array(s, dtype=int).reshape(-1)


def i_m_q(T, absorbing):
    A = np.eye(T.shape[0]) - T
    A[:, absorbing] = 0.0
    A[absorbing, :] = 0.0
    A[absorbing, absorbing] = 1.0
    return A


def committor_system(T, sources, sinks):
    """(I - Q, r): the one right-hand side of enspara_amd's committors"""
    T = np.asarray(T, dtype=np.float64)
    sources, sinks = _states(sources), _states(sinks)
    r = np.zeros(T.shape[0])
    for s in sinks:
        r = r + T[:, s]
    r[sinks] = 1.0
    r[sources] = 0.0
    return i_m_q(T, np.append(sources, sinks)), r


def mfpt_sink_system(T, sinks):
    T = np.asarray(T, dtype=np.float64)
    sinks = _states(sinks)
    c = np.ones(T.shape[0])
    c[sinks] = 0.0
    return i_m_q(T, sinks), c


def mfpt_all_system(T, pops):
    T = np.asarray(T, dtype=np.float64)
    n = T.shape[0]
    return (np.eye(n) - T) + np.asarray(pops, dtype=np.float64)[None, :], np.eye(n)


def committors(T, sources, sinks, solver=solve):
    A, r = committor_system(T, sources, sinks)
    q = solver(A, r)
    q[_states(sinks)] = 1.0
    q[_states(sources)] = 0.0
    return q


def mfpts(T, sinks=None, populations=None, lagtime=1., solver=solve):
    if sinks is None:
        A, eye = mfpt_all_system(T, populations)
        Z = solver(A, eye)
        return (lagtime * (np.diag(Z)[None, :] - Z)) / np.asarray(populations)[None, :]
    A, c = mfpt_sink_system(T, sinks)
    return lagtime * solver(A, c)


def fluxes_from(T, pops, q):
    """the reference's order: (T * (pi (1 - q))[:, None]) * q, zero diagonal; any
    float type"""
    f = (T * (pops * (1 - q))[:, None]) * q[None, :]
    f[np.arange(len(q)), np.arange(len(q))] = 0
    return f


def net_from(f):
    d = f - f.T
    d[d < 0] = 0
    return d


def reactive_fluxes(T, sources, sinks, populations, solver=solve):
    T = np.asarray(T, dtype=np.float64)
    return fluxes_from(T, np.asarray(populations, dtype=np.float64),
                       committors(T, sources, sinks, solver=solver))


def net_fluxes(T, sources, sinks, populations, solver=solve):
    return net_from(reactive_fluxes(T, sources, sinks, populations, solver=solver))


def reactive_populations(T, sources, sinks, populations, solver=solve):
    q = committors(T, sources, sinks, solver=solver)
    d = np.asarray(populations, dtype=np.float64) * q * (1 - q)
    return d / np.sum(d)


# ---- test matrices -----------------------------------------------------------------------
def chain_counts(n, seed, cross=0.01, steps=None):
    """block_chain_counts symmetrised, one count more on the diagonal: the counts
    of a reversible metastable chain (integers: the goldens store these)"""
    n_blocks = max(2, min(6, n // 8))
    C = nb.block_chain_counts(n, n_blocks, steps or 60 * n + 2000, seed, cross=cross)
    return C + C.T + np.eye(n, dtype=np.int64)


def weighted_chain(n, seed=0):
    """(T, pops) of a reversible metastable chain without the sampled walk (too
    slow in Python above a few hundred states): symmetric weights, heavy inside
    10 blocks, light across"""
    rng = np.random.RandomState(seed)
    block = np.arange(n) * 10 // n
    W = rng.rand(n, n) * np.where(block[:, None] == block[None, :], 1.0, 1e-3)
    W = W + W.T + np.diag(0.3 * n * rng.rand(n))
    return W / W.sum(axis=1)[:, None], W.sum(axis=1) / W.sum()


# the sizes of tests/test_gpu_lu_large.py: the first keeps rows in a thread's second
# register slot, the second in all four slots and in memory behind them
LU_N_SLOTS, LU_N_TAIL = 1100, 4200


def _distinct(groups, n):
    idx = np.array(groups, dtype=np.int64).reshape(-1)
    assert len(set(idx.tolist())) == idx.size and idx.min() >= 0 and idx.max() < n, \
        "indices are distinct and in [0, %d)" % n
    assert all(list(g) == sorted(g) for g in groups), "every group ascends"


def swapped_dominant(n, pairs, seed=0):
    """(A, pivots): D = rand(n, n) + n I with rows k and r exchanged for every
    (k, r) of pairs, k < r, the pairs disjoint.  The diagonal dominates every
    column throughout the elimination (entries right of it change by about 1 / n
    per step), so step k finds D's row k, which lies in row r: pivots[k] = r
    and pivots[j] = j for every other j, r included"""
    _distinct(pairs, n)
    A = np.random.RandomState(seed).rand(n, n) + n * np.eye(n)
    piv = np.arange(n, dtype=np.int32)
    for k, r in pairs:
        A[[k, r]] = A[[r, k]]
        piv[k] = r
    return A, piv


def tie_system(n, triples):
    """(A, pivots) for triples (k, r1, r2, s), k < r1 < r2, s = +1 or -1, all
    indices distinct.  From the identity: A[k, k] = 0, A[k, r1] = 1, A[r1, r1] = 0,
    A[r1, k] = s, A[r2, k] = -s.  Column k then holds exactly two candidates, s in
    row r1 and -s in row r2, equal in |a|: the rule (largest |a|, lowest row) gives
    pivots[k] = r1, and pivots[j] = j everywhere else (after the exchange row r1
    is e_r1, and row r2 only gains the multiplier 1 in column k).  The elimination
    is exact in integers, and so is the solution for an integer B: x[r1] = b[k],
    x[k] = s b[r1], x[r2] = b[r2] + b[r1]"""
    _distinct([t[:3] for t in triples], n)
    A = np.eye(n)
    piv = np.arange(n, dtype=np.int32)
    for k, r1, r2, s in triples:
        assert s in (1, -1)
        A[k, k] = 0.0
        A[k, r1] = 1.0
        A[r1, r1] = 0.0
        A[r1, k] = s
        A[r2, k] = -s
        piv[k] = r1
    return A, piv


def small_integer_rhs(n, nrhs=2):
    return np.arange(nrhs * n, dtype=np.float64).reshape(n, nrhs) % 7 - 3


def tprob_from_counts(C):
    C = np.asarray(C, dtype=np.float64)
    return C / C.sum(axis=1)[:, None]


def pops_from_counts(C):
    """the stationary distribution of the row-normalised symmetric counts"""
    C = np.asarray(C, dtype=np.float64)
    return C.sum(axis=1) / C.sum()


# ---- error measures -------------------------------------------------------------------------
def backward_error(A, X, B):
    """eta = ||B - A X||_inf / (||A||_inf ||X||_inf + ||B||_inf), the residual in
    long double; matrix infinity norms"""
    A, X, B = (np.asarray(a, dtype=np.float64) for a in (A, X, B))
    n = A.shape[0]
    X2, B2 = X.reshape(n, -1), B.reshape(n, -1)
    R = B2.astype(LD) - A.astype(LD) @ X2.astype(LD)

    def ninf(M):
        return float(np.abs(M).sum(axis=1).max())
    return ninf(R) / (ninf(A) * ninf(X2) + ninf(B2))


def check_backward(tag, A, B, X):
    """the backward criterion: eta(X) <= 8 max(eta_ref, u), eta_ref that of
    numpy.linalg.solve on the same system; prints both and returns the ratio"""
    eta = backward_error(A, X, B)
    eta_ref = backward_error(A, np.linalg.solve(A, B), B)
    ratio = eta / max(eta_ref, U)
    print("%-22s eta_dev %.2f u  eta_ref %.2f u  eta_dev / max(eta_ref, u) = %.2f (<= 8)"
          % (tag, eta / U, eta_ref / U, ratio))
    assert eta <= 8 * max(eta_ref, U)
    return ratio


def forward_bound(err_ref, x_hp):
    """32 max(err_ref, u max|x_hp|)"""
    return 32.0 * max(float(err_ref), U * float(np.max(np.abs(x_hp))))


# ---- high precision ----------------------------------------------------------------------------
def _exact_ints(a):
    """float64 array -> (object array of Python ints m, e) with a == m 2^e exactly"""
    a = np.asarray(a, dtype=np.float64)
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64).astype(object)
    e = e.astype(np.int64) - 53
    nz = a != 0
    emin = int(e[nz].min()) if np.any(nz) else 0
    sh = np.where(nz, e - emin, 0).astype(object)
    return mi * (2 ** sh), emin


def _split(x):
    """long double -> (hi, lo) float64 with x == hi + lo exactly (64-bit mantissa)"""
    hi = x.astype(np.float64)
    lo = (x - hi.astype(LD)).astype(np.float64)
    assert np.all(hi.astype(LD) + lo.astype(LD) == x)
    return hi, lo


def exact_residual(A, X, B):
    """B - A X with X long double: computed exactly in integers, each entry rounded
    once to float64 (the correction needs its leading digits only)"""
    n = A.shape[0]
    Ai, ea = _exact_ints(A)
    hi, lo = _split(X.reshape(n, -1))
    Hi, eh = _exact_ints(hi)
    Li, el = _exact_ints(lo)
    Bi, eb = _exact_ints(np.asarray(B, dtype=np.float64).reshape(n, -1))
    e0 = min(ea + eh, ea + el, eb)
    R = (Bi * 2 ** (eb - e0) - Ai.dot(Hi) * 2 ** (ea + eh - e0)
         - Ai.dot(Li) * 2 ** (ea + el - e0))
    out = np.zeros(R.shape)
    for idx, v in np.ndenumerate(R):
        v = int(v)
        s = max(abs(v).bit_length() - 64, 0)
        out[idx] = math.ldexp(float(v >> s), s + e0)
    return out


def solve_hp(A, B, max_steps=8):
    """Iterative refinement of numpy's solution, the iterate in long double and the
    residuals exact -> (X as long double, steps).  Accepted when two successive
    iterates agree to 4 long-double ulps of max|X|; raises if they never do."""
    A = np.asarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    n = A.shape[0]
    X = np.linalg.solve(A, B.reshape(n, -1)).astype(LD)
    eps = float(np.finfo(LD).eps)
    for step in range(1, max_steps + 1):
        D = np.linalg.solve(A, exact_residual(A, X, B))
        X = X + D.astype(LD)
        if float(np.max(np.abs(D))) <= 4 * eps * float(np.max(np.abs(X))):
            return X.reshape(B.shape), step
    raise RuntimeError("refinement did not converge in %d steps" % max_steps)


def hp_solver(steps_out=None):
    def s(A, B):
        X, k = solve_hp(A, B)
        if steps_out is not None:
            steps_out.append(k)
        return X
    return s
