"""Committors and mean first passage times (reference enspara/tpt/core.py;
Grinstead and Snell, Introduction to Probability, AMS 2006) on the device.

Where this differs from the reference, on purpose:

* ``committors`` solves once.  The reference solves ``(I - Q) b = T[:, s]`` for
  every sink ``s`` and sums the solutions; the solve is linear, so the sum of
  the right-hand sides gives the same ``q`` with one right-hand side.
* Sparse ``tprob`` is accepted everywhere and densified for the work (the
  reference's ``mfpts`` fails on sparse input at ``len(tprob)``).
* ``DataInvalid`` is raised for input that is not square or not finite, for
  empty ``sources`` / ``sinks``, for indices out of range, for a state that is
  both source and sink, and for a system the factorisation finds singular
  (a zero or NaN pivot; the message names the column) -- where the reference
  lets LAPACK or SuperLU warn or raise.
* The solver is the device's own LU (csrc/ek_lu.hip): backward stable like
  LAPACK's, but blocked differently and with sums in another order, so values
  agree with the reference's to the conditioning of the system, not bit for bit.
  Two runs of the same call give the same bits.
"""
import numpy as np
import scipy.sparse

from .. import _lib
from ..exception import DataInvalid

__all__ = ["committors", "mfpts"]

# the solver's panel width (EK_LU_NB of csrc/ek_lu.h): systems are padded to
# whole panels on the device
LU_PANEL = 64
# where the solver's kernels change form (csrc/ek_lu.hip; nothing here computes
# with them: the tests place their shapes around them).  A sub-panel's thread t
# keeps rows c0 + t + LU_PANEL_WG * i, i < LU_SUB_RPT, in registers and leaves the
# rows from c0 + LU_PANEL_WG * LU_SUB_RPT on in memory; the back substitution runs
# a workgroup per LU_COL_WG right-hand sides.
LU_PANEL_WG = 1024      # LU_PANEL_WG
LU_SUB_RPT = 4          # LU_SUB_RPT
LU_COL_WG = 256         # LU_COL_WG


def _dense_tprob(tprob):
    """``tprob`` as a checked, C-contiguous float64 array."""
    if scipy.sparse.issparse(tprob):
        tprob = tprob.toarray()
    T = np.ascontiguousarray(np.asarray(tprob), dtype=np.float64)
    if T.ndim != 2 or T.shape[0] != T.shape[1] or T.shape[0] < 1:
        raise DataInvalid("a transition matrix is square, not %s" % (T.shape,))
    if not np.all(np.isfinite(T)):
        raise DataInvalid("the transition matrix has entries that are not finite")
    return T


def _states(states, n, what):
    """``states`` (a scalar or a sequence) as a checked int32 array."""
    try:
        s = np.array(states, dtype=int).reshape(-1)
    except (TypeError, ValueError):
        raise DataInvalid("%s are state indices, not %r" % (what, states))
    if s.size == 0:
        raise DataInvalid("%s are empty" % what)
    if s.min() < 0 or s.max() >= n:
        raise DataInvalid("%s %s are not all in [0, %d)" % (what, s.tolist(), n))
    return np.ascontiguousarray(s, dtype=np.int32)


def _source_sink_states(sources, sinks, n):
    sources = _states(sources, n, "sources")
    sinks = _states(sinks, n, "sinks")
    both = np.intersect1d(sources, sinks)
    if both.size:
        raise DataInvalid("states %s are both source and sink" % both.tolist())
    return sources, sinks


def _populations(T, populations, device):
    if populations is None:
        from ..msm import eq_probs
        populations = eq_probs(T, device=device)
    pops = np.ascontiguousarray(np.asarray(populations), dtype=np.float64).reshape(-1)
    if pops.shape[0] != T.shape[0]:
        raise DataInvalid("%d populations for %d states" % (pops.shape[0], T.shape[0]))
    if not np.all(np.isfinite(pops)):
        raise DataInvalid("the populations have entries that are not finite")
    return pops


def _check_info(info, what):
    if info >= 0:
        raise DataInvalid(
            "%s: the system is singular to working precision (zero or NaN pivot in "
            "column %d); is there a closed set of states that holds no absorbing "
            "state, or a disconnected one?" % (what, info))


def _solve(A, B, return_pivots=False, device=0):
    """``X`` with ``A X = B`` by the device's LU (ek_lu_solve) -> ``X``, or
    ``(X, pivots, info)`` with ``return_pivots``: ``pivots[k]`` the row exchanged
    with row k at step k, ``info`` -1 or the first column with a zero or NaN
    pivot (without ``return_pivots`` that raises ``DataInvalid``).  ``B`` is
    ``[n]`` or ``[n, nrhs]``, ``nrhs <= n``.  Private: tests exercise the solver
    through it on matrices no TPT system produces."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    if A.ndim != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise DataInvalid("A is square, not %s" % (A.shape,))
    n = A.shape[0]
    vector = B.ndim == 1
    B2 = np.ascontiguousarray(B.reshape(-1, 1) if vector else B)
    if B2.ndim != 2 or B2.shape[0] != n or not 1 <= B2.shape[1] <= n:
        raise DataInvalid("B is [n] or [n, nrhs <= n], not %s" % (B.shape,))
    if not (np.all(np.isfinite(A)) and np.all(np.isfinite(B2))):
        raise DataInvalid("A and B have entries that are not finite")
    X = np.zeros_like(B2)
    piv = np.zeros(n, dtype=np.int32)
    info = np.zeros(1, dtype=np.int32)
    L = _lib.load()
    _lib.check(L.ek_lu_solve(int(device), n, _lib.f64p(A), B2.shape[1], _lib.f64p(B2),
                             _lib.f64p(X), _lib.i32p(piv), _lib.i32p(info)))
    if vector:
        X = X[:, 0]
    if return_pivots:
        return X, piv, int(info[0])
    _check_info(int(info[0]), "_solve")
    return X


def committors(tprob, sources, sinks, device=0):
    """Get the forward committors of the reaction sources -> sinks: for every
    state the probability that it reaches a sink before it reaches a source
    (reference core.py:40-102).

    Parameters
    ----------
    tprob : array-like or scipy sparse matrix, shape=(n_states, n_states)
        Transition probability matrix (sparse input is densified).
    sources, sinks : int or array-like of int
        The source (reactant) and the sink (product) states.
    device : int
        The HIP device.

    Returns
    -------
    committors : np.ndarray, shape=(n_states,), float64
        ``committors[sinks] == 1`` and ``committors[sources] == 0`` exactly.

    Sources and sinks are made absorbing and ``(I - Q) q = r`` is solved on the
    device with ``r = sum over the sinks of T[:, s]``, ``r[sinks] = 1``,
    ``r[sources] = 0``: ONE solve, where the reference solves one right-hand
    side per sink and sums the solutions -- the same ``q``, since the solve is
    linear.  See the module's docstring for the other deviations."""
    T = _dense_tprob(tprob)
    n = T.shape[0]
    sources, sinks = _source_sink_states(sources, sinks, n)
    q = np.zeros(n)
    info = np.zeros(1, dtype=np.int32)
    L = _lib.load()
    _lib.check(L.ek_tpt_committors(int(device), n, _lib.f64p(T), _lib.i32p(sources),
                                   len(sources), _lib.i32p(sinks), len(sinks),
                                   _lib.f64p(q), _lib.i32p(info)))
    _check_info(int(info[0]), "committors")
    return q


def mfpts(tprob, sinks=None, populations=None, lagtime=1., device=0):
    """Mean first passage times, to a set of sinks or from all states to all
    (reference core.py:105-155).

    Parameters
    ----------
    tprob : array-like or scipy sparse matrix, shape=(n_states, n_states)
        Transition probability matrix (sparse input is densified).
    sinks : int or array-like of int, optional
        The product states.  None: all to all.
    populations : array-like, shape=(n_states,), optional
        Equilibrium populations, used (and, if None, computed with
        ``enspara_amd.msm.eq_probs``) for all-to-all only.
    lagtime : float
        Scales the result; 1: units of lag times.
    device : int
        The HIP device.

    Returns
    -------
    mfpts : np.ndarray, float64
        With sinks, shape (n_states,): ``lagtime * (I - Q)^-1 c`` with ``c`` 1
        off the sinks and 0 on them.  Without, shape (n_states, n_states):
        ``mfpts[i, j] = lagtime * (Z[j, j] - Z[i, j]) / populations[j]`` with
        the fundamental matrix ``Z = (I - T + W)^-1``, every row of ``W`` the
        populations; the inverse is a solve against the identity on the device
        (about 3 n^2 float64 of device memory).

    See the module's docstring for the deviations from the reference."""
    T = _dense_tprob(tprob)
    n = T.shape[0]
    lagtime = float(lagtime)
    info = np.zeros(1, dtype=np.int32)
    L = _lib.load()
    if sinks is None:
        pops = _populations(T, populations, device)
        out = np.zeros((n, n))
        _lib.check(L.ek_tpt_mfpts_all(int(device), n, _lib.f64p(T), _lib.f64p(pops),
                                      lagtime, _lib.f64p(out), _lib.i32p(info)))
    else:
        sinks = _states(sinks, n, "sinks")
        out = np.zeros(n)
        _lib.check(L.ek_tpt_mfpts_sinks(int(device), n, _lib.f64p(T), _lib.i32p(sinks),
                                        len(sinks), lagtime, _lib.f64p(out),
                                        _lib.i32p(info)))
    _check_info(int(info[0]), "mfpts")
    return out
