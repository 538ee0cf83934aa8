"""A restatement of weighted joint probabilities and weighted mutual information
(reference enspara/info_theory/mutual_info.py:78-178) whose sums are math.fsum --
correctly rounded, whatever the order -- the expected values of tests/test_gpu_wmi.py.

    P[i, j, u, v] = fsum over t of w_t [f_ti == u] [f_tj == v]
    P_x[i, u]     = fsum over t of w_t [f_ti == u]          (= P[i, i, u, u])
    term          = P * log(P / (P_x[i, u] * P_x[j, v]))    where P_x P_x != 0 and P != 0
    mi[i, j]      = fsum of the terms

and, for the bounds of the tests, L[i, j] = max |log(P / P_x P_x)| and A[i, j] =
fsum |term|.
"""
import math

import numpy as np

U = 2.0 ** -52


def joint_probabilities(features, weights, S):
    """-> P [F, F, S, S] float64, every cell the correctly rounded sum"""
    features = np.asarray(features).astype(np.int64)
    w = np.asarray(weights, dtype=np.float64)
    T, F = features.shape
    P = np.zeros((F, F, S, S))
    for i in range(F):
        for j in range(i, F):
            key = features[:, i] * S + features[:, j]
            order = np.argsort(key, kind="stable")
            ks = key[order]
            ws = w[order].tolist()
            cells = np.unique(ks)
            lo = np.searchsorted(ks, cells, side="left")
            hi = np.searchsorted(ks, cells, side="right")
            for c, a, b in zip(cells.tolist(), lo.tolist(), hi.tolist()):
                P[i, j, c // S, c % S] = math.fsum(ws[a:b])
            P[j, i] = P[i, j].T
    return P


def normalise(weights):
    """the reference's: divided by the L1 norm unless the sum is 1"""
    w = np.array(weights, dtype=np.float64)
    return w if w.sum() == 1 else w / np.linalg.norm(w, ord=1)


def mutual_information(P):
    """-> (mi, L, A), each [F, F]: not normalised, not clipped"""
    F, S = P.shape[0], P.shape[2]
    mi, L, A = np.zeros((F, F)), np.zeros((F, F)), np.zeros((F, F))
    Px = np.array([[P[i, i, u, u] for u in range(S)] for i in range(F)])
    for i in range(F):
        for j in range(F):
            terms = []
            for u in range(S):
                for v in range(S):
                    pm, p = Px[i, u] * Px[j, v], P[i, j, u, v]
                    if pm == 0 or p == 0:
                        continue
                    lg = math.log(p / pm)
                    L[i, j] = max(L[i, j], abs(lg))
                    terms.append(p * lg)
            mi[i, j] = math.fsum(terms)
            A[i, j] = math.fsum(abs(t) for t in terms)
    return mi, L, A


def finish(mi, n_states, normalize=True):
    """channel-capacity normalisation (log of the smaller number of states) and clip"""
    mi = np.array(mi)
    if normalize:
        n = np.full(len(mi), n_states) if np.ndim(n_states) == 0 else np.asarray(n_states)
        mi = mi / np.log(np.minimum(n[:, None], n[None, :]))
    return np.clip(mi, 0, np.inf)


def p_bound(T, P):
    """|P_dev - P| <= T 2^-52 P: T - 1 additions of non-negative terms, each rounding by
    at most 2^-53 of a partial sum that is at most the whole"""
    return T * U * P


def mi_bound(T, S, L, A):
    """|mi_dev - mi| <= 2^-52 (T (L + 3) + (S^2 + 4) A).  First part: P, P_x and P_y each
    within T 2^-52 relative, carried to first order through P log(P / P_x P_y) and
    summed with sum P = 1 (|log| <= L, and the three relative errors inside the log);
    second part: a log within one ulp and S^2 additions, as _numpy_mi.mi_bound."""
    return U * (T * (L + 3) + (S * S + 4) * A)


def codes(rng, T, F, S):
    """feature i leans towards state i % S; feature F - 1 a noisy copy of feature 0"""
    X = rng.randint(0, S, size=(T, F))
    X = np.where(rng.rand(T, F) < 0.4, (np.arange(F) % S)[None, :], X)
    if F > 1:
        X[:, F - 1] = np.where(rng.rand(T) < 0.1, rng.randint(0, S, size=T), X[:, 0])
    return X
