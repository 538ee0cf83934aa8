"""Affinity propagation (Frey and Dueck, Science 315, 2007) of a precomputed
similarity matrix, in numpy: what the reference's exposons take from
``sklearn.cluster.AffinityPropagation(affinity='precomputed', random_state=0)``.

It gives scikit-learn's labels because it makes scikit-learn's choices: the
noise that breaks ties between equal similarities is ``RandomState(0)
.standard_normal((n, n))`` scaled by ``eps * S + 100 * tiny``; responsibilities
are updated before availabilities, both damped; a point is an exemplar while
``A[k, k] + R[k, k] > 0``; the run stops once the exemplars have not changed
for ``convergence_iter`` iterations; the exemplar of each cluster is then
replaced by the member most similar to the others, and labels number the
exemplars in ascending order.  A matrix whose off-diagonal entries are all
equal is not iterated on: one cluster, or one per point if the preference is
larger.
"""
import warnings

import numpy as np

__all__ = ["affinity_propagation", "ConvergenceWarning"]


class ConvergenceWarning(UserWarning):
    """Affinity propagation stopped at ``max_iter``."""


def _all_equal(S):
    off = S[~np.eye(len(S), dtype=bool)]
    return np.all(off == off[0])


def affinity_propagation(S, damping, preference=0, max_iter=10000, convergence_iter=15,
                         return_n_iter=False):
    """Cluster by the similarities ``S`` ([n, n], left as it is).

    Returns the labels [n] (``-1`` everywhere, with a ``ConvergenceWarning``,
    if no exemplar was found; with the same warning and whatever exemplars
    the last iteration had if ``max_iter`` was reached), and with
    ``return_n_iter`` also the number of iterations run.
    """
    S = np.array(S, dtype=np.float64)
    if S.ndim != 2 or S.shape[0] != S.shape[1] or S.shape[0] < 1:
        raise ValueError("S must be a square matrix, got shape %s" % (S.shape,))
    if not 0.5 <= damping < 1:
        raise ValueError("damping must be in [0.5, 1), got %r" % (damping,))
    n = S.shape[0]
    preference = float(preference)

    if n == 1 or _all_equal(S):
        warnings.warn("All samples have mutually equal similarities. "
                      "Returning arbitrary cluster center(s).")
        labels = np.arange(n) if preference > S.flat[n - 1] else np.zeros(n, dtype=np.intp)
        return (labels, 0) if return_n_iter else labels

    diag = slice(None, None, n + 1)
    S.flat[diag] = preference
    A, R, tmp = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    S += ((np.finfo(S.dtype).eps * S + np.finfo(S.dtype).tiny * 100)
          * np.random.RandomState(0).standard_normal(size=(n, n)))
    e = np.zeros((n, convergence_iter))
    ind = np.arange(n)

    never_converged = True
    it = -1
    for it in range(max_iter):
        # responsibilities: tmp = A + S, its row maximum and runner-up
        np.add(A, S, tmp)
        I = np.argmax(tmp, axis=1)
        Y = tmp[ind, I]
        tmp[ind, I] = -np.inf
        Y2 = np.max(tmp, axis=1)
        np.subtract(S, Y[:, None], tmp)
        tmp[ind, I] = S[ind, I] - Y2
        tmp *= 1 - damping
        R *= damping
        R += tmp
        # availabilities: tmp = the positive responsibilities, the diagonal as it is
        np.maximum(R, 0, tmp)
        tmp.flat[diag] = R.flat[diag]
        tmp -= np.sum(tmp, axis=0)
        dA = np.diag(tmp).copy()
        tmp.clip(0, np.inf, tmp)
        tmp.flat[diag] = dA
        tmp *= 1 - damping
        A *= damping
        A -= tmp
        # the exemplars, and whether they have stood still
        E = (np.diag(A) + np.diag(R)) > 0
        e[:, it % convergence_iter] = E
        K = np.sum(E, axis=0)
        if it >= convergence_iter:
            se = np.sum(e, axis=1)
            unconverged = np.sum((se == convergence_iter) + (se == 0)) != n
            if not unconverged and K > 0:
                never_converged = False
                break

    I = np.flatnonzero(E) if max_iter > 0 else np.zeros(0, dtype=np.intp)
    K = I.size
    if K > 0:
        if never_converged:
            warnings.warn("Affinity propagation did not converge, this model "
                          "may return degenerate cluster centers and labels.",
                          ConvergenceWarning)
        c = np.argmax(S[:, I], axis=1)
        c[I] = np.arange(K)
        # the member of each cluster that is most similar to the others
        for k in range(K):
            ii = np.flatnonzero(c == k)
            j = np.argmax(np.sum(S[ii[:, np.newaxis], ii], axis=0))
            I[k] = ii[j]
        c = np.argmax(S[:, I], axis=1)
        c[I] = np.arange(K)
        labels = I[c]
        labels = np.searchsorted(np.unique(labels), labels)
    else:
        warnings.warn("Affinity propagation did not converge and this model "
                      "will not have any cluster centers.", ConvergenceWarning)
        labels = np.full(n, -1, dtype=np.intp)
    return (labels, it + 1) if return_n_iter else labels
