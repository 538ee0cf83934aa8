"""Relative entropy of Markov state models, Jensen-Shannon divergence and Shannon
entropy (reference enspara/info_theory/entropy.py) on the device, and the state
histogram of discrete features that the reference's ``compute-shannon-entropy``
app reads off the diagonal of ``joint_counts(X, X)``.

The sums over a row -- ``P * log(P / Q)``, the two sums of the Jensen-Shannon
form, ``-p * log(p)`` -- are taken by csrc/ek_entropy.hip in float64, in an
order the row's width fixes: the same bits on every run, but not numpy's
pairwise order, so a result differs from the reference's by rounding (about
``(columns + 4) * 2^-52`` of the sum of the terms' magnitudes).
Conversion to ``base`` and the population-weighted sum over the states are numpy
on the ``[n]`` vector, as in the reference.

Where this differs from the reference, on purpose:

* ``kl_divergence`` raises ``DataInvalid`` on shapes that differ (the reference
  has a bare ``raise``), on input that is not 1-D or 2-D, empty, or sparse (the
  reference densifies).
* ``relative_entropy_per_state`` with neither ``Q`` nor ``assignments`` raises
  ``DataInvalid`` (the reference prints a message and fails on ``None``).
* ``shannon_entropy``: an element ``p <= 0`` contributes exactly 0.  The
  reference's ``np.log(p, where=p > 0)`` leaves those slots of its output
  uninitialised, which is 0 in effect for ``p = 0``; here it is pinned to 0.
* With ``assignments=`` and the default builder, ``Q`` is built on the device
  from the sparse counts and never visits the host; the result has the bits of
  ``kl_divergence(P, Q_from_assignments(...))``.
"""
import ctypes
import warnings

import numpy as np
import scipy.sparse

from .. import _lib, exception
from ..msm import builders
from ..msm.transition_matrices import _rows_of, assigns_to_counts, eq_probs
from .mutual_info import _check, _codes, _n_states, _u8p, MAX_FEATURES, MAX_FRAMES

__all__ = ["Q_from_assignments", "relative_entropy_per_state", "relative_entropy_msm",
           "energy_to_probability", "shannon_entropy", "shannon_entropy_rows",
           "kl_divergence", "js_divergence", "state_counts", "StateCounts",
           "last_timing"]


def _default_prior(assignments):
    """The pseudocount used when none is given: the reciprocal of the number
    of frame-to-next-frame steps in all trajectories together (inf for none)."""
    _, lengths = _rows_of(assignments)
    n_steps = np.sum(lengths - 1)
    with np.errstate(divide="ignore"):
        return 1 / n_steps


def _dense_matrix(M, what):
    """``M`` as an ndarray; ``DataInvalid`` for scipy sparse input."""
    if scipy.sparse.issparse(M):
        raise exception.DataInvalid(
            "%s is sparse; densify it first (no sparse support)." % what)
    return np.asarray(M)


def Q_from_assignments(
        assignments, n_states=None, lag_time=1, builder=builders.normalize,
        prior_counts=None, device=0):
    """Transition probabilities estimated from state assignments, for use as
    the ``Q`` of the relative entropies below.

    The transitions at ``lag_time`` are counted on the device, made a dense
    ``[n_states, n_states]`` matrix, every cell raised by ``prior_counts`` and
    the sum handed to ``builder``.

    Parameters
    ----------
    assignments : array [n_trajectories, n_frames], list of arrays or RaggedArray
    n_states : int, optional
        Size of the matrix; the largest label plus one if left out.
    lag_time : int
    builder : one of ``msm.builders``
        Invoked as ``builder(counts, calculate_eq_probs=False)``; whatever it
        warns about is suppressed.
    prior_counts : float, optional
        Pseudocount per cell.  Left out: one over the number of lag-1 steps of
        all trajectories together.

    Returns
    -------
    np.ndarray, shape=(n_states, n_states): the builder's probabilities.
    """
    pseudo = _default_prior(assignments) if prior_counts is None else prior_counts
    sparse_counts = assigns_to_counts(
        assignments, max_n_states=n_states, lag_time=lag_time, device=device)
    dense = np.array(sparse_counts.todense()) + pseudo
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        built = builder(dense, calculate_eq_probs=False)
    return built[1]


def _rows(M, what):
    """``M`` as (C-contiguous float64 [rows, cols], was it 1-D)"""
    M = np.asarray(_dense_matrix(M, what), dtype=np.float64)   # (no copy of float64)
    if M.ndim == 0:
        M = M.reshape(1)
    if M.ndim > 2 or M.size == 0:
        raise exception.DataInvalid(
            "%s is a distribution or rows of distributions, not an array of shape %s."
            % (what, M.shape,))
    return np.ascontiguousarray(M.reshape(-1, M.shape[-1])), M.ndim == 1


def _raise_negative(flags, P, Q):
    for bit, name, M in ((1, "P", P), (2, "Q", Q)):
        if flags & bit:
            raise exception.DataInvalid(
                "%s has a negative probability among its entries:\n%s" % (name, M))


def _kl_rows(P, Q, js, device):
    """-> the row sums in nats ([rows], or two of them), was the input 1-D"""
    P, flat = _rows(P, "P")
    Q, _ = _rows(Q, "Q")
    if P.shape != Q.shape:
        raise exception.DataInvalid(
            "P and Q must have the same shape; got %s and %s." % (P.shape, Q.shape))
    out = np.zeros((2 if js else 1, P.shape[0]))
    flags = ctypes.c_uint32(0)
    L = _lib.load()
    if js:
        _check(L.ek_ent_js_rows(int(device), P.shape[0], P.shape[1], _lib.f64p(P),
                                _lib.f64p(Q), _lib.f64p(out[0]), _lib.f64p(out[1]),
                                ctypes.byref(flags)))
    else:
        _check(L.ek_ent_kl_rows(int(device), P.shape[0], P.shape[1], _lib.f64p(P),
                                _lib.f64p(Q), _lib.f64p(out[0]), ctypes.byref(flags)))
    _raise_negative(flags.value, P, Q)
    return out, flat


def kl_divergence(P, Q, base=2, device=0):
    """Kullback-Leibler divergence ``sum_j P_j log(P_j / Q_j)`` of ``P`` from
    ``Q``, row by row for matrices, summed on the device.

    Parameters
    ----------
    P, Q : array, shape=(n_rows, n_values) or (n_values,), equal shapes
        Distributions (rows of them); not negative anywhere.
    base : float
        Unit of the result: 2 for bits (the default), e for nats.

    Returns
    -------
    np.ndarray, shape=(n_rows,); a float64 scalar for 1-D input
        A term with ``P = 0`` is 0; one with ``P > 0`` and ``Q = 0`` is +inf,
        and so is its row.

    Raises ``DataInvalid`` for a negative entry of either argument, for shapes
    that differ, and for sparse, empty or more than 2-D input.
    """
    out, flat = _kl_rows(P, Q, False, device)
    nats = out[0]
    nats /= np.log(base)
    return nats[0] if flat else nats


def js_divergence(p, q, device=0):
    """Jensen-Shannon divergence in bits: the mean of the KL divergences of
    ``p`` and of ``q`` from their midpoint ``m = (p + q) / 2``.  The device
    makes one pass over ``p`` and ``q`` and never stores ``m``."""
    out, flat = _kl_rows(p, q, True, device)
    out /= np.log(2)
    js = 0.5 * out[0] + 0.5 * out[1]
    return js[0] if flat else js


def shannon_entropy_rows(p, normalize=True, device=0):
    """The Shannon entropy ``-sum p log p`` of every row of ``p`` ([rows,
    values]), in nats; with ``normalize`` each row is first divided by its sum.
    Elements ``<= 0`` contribute 0."""
    p = _dense_matrix(p, "p")
    if p.ndim != 2:
        raise exception.DataInvalid("p is [rows, values], not %s" % (p.shape,))
    p, _ = _rows(p, "p")
    out = np.zeros(p.shape[0])
    _check(_lib.load().ek_ent_shannon_rows(int(device), p.shape[0], p.shape[1],
                                           _lib.f64p(p), 1 if normalize else 0,
                                           _lib.f64p(out)))
    return out


def shannon_entropy(p, normalize=True, device=0):
    """Entropy ``-sum p log p`` in nats of ONE distribution: all cells of ``p``
    together, whatever its shape (``shannon_entropy_rows`` treats rows apart).

    Parameters
    ----------
    p : array of any shape
        Weights of the outcomes.
    normalize : bool
        Divide by the total first, so that the weights need not sum to one.
        The argument itself is not modified.

    Returns
    -------
    float.  Cells with ``p <= 0`` add exactly 0.  (The reference evaluates
    ``np.log(p, where=p > 0)``, which leaves the masked slots of its result
    uninitialised; for ``p = 0`` the product is 0 in effect.  Here 0 is
    guaranteed.)
    """
    p = np.asarray(_dense_matrix(p, "p"), dtype=np.float64)
    if p.size == 0:
        raise exception.DataInvalid("p is empty")
    return float(shannon_entropy_rows(p.reshape(1, -1), normalize, device)[0])


def energy_to_probability(u, kT=2.479):
    """Boltzmann probabilities ``exp(-u / kT) / Z`` of the energies ``u``
    (``kT`` in their unit; the default is kJ/mol near 298 K).  Host numpy; the
    mean energy is subtracted before exponentiating, which cancels in the
    ratio and keeps the exponents small."""
    u = np.asarray(u, dtype=np.float64)
    weights = np.exp((u.mean() - u) / kT)
    return weights / weights.sum()


def _kl_from_counts(P, assignments, n_states, lag_time, prior_counts, device):
    """``kl_divergence(P, Q_from_assignments(...), base=e)`` for
    builders.normalize with Q built on the device from the sparse counts."""
    P, _ = _rows(P, "P")
    if prior_counts is None:
        prior_counts = _default_prior(assignments)
    prior = float(prior_counts)
    if not prior >= 0:
        raise exception.DataInvalid("prior_counts must not be negative, got %r" % prior)
    # (assigns_to_counts returns every cell at most once, duplicates summed: what
    # ek_ent_kl_counts requires of its caller)
    counts = assigns_to_counts(
        assignments, max_n_states=n_states, lag_time=lag_time, device=device)
    if P.shape != counts.shape:
        raise exception.DataInvalid(
            "P and Q must have the same shape; got %s and %s." % (P.shape, counts.shape))
    ci = np.ascontiguousarray(counts.row, dtype=np.int32)
    cj = np.ascontiguousarray(counts.col, dtype=np.int32)
    cv = np.ascontiguousarray(counts.data, dtype=np.int64)
    out = np.zeros(P.shape[0])
    flags = ctypes.c_uint32(0)
    _check(_lib.load().ek_ent_kl_counts(
        int(device), P.shape[0], _lib.f64p(P), len(cv), _lib.i32p(ci), _lib.i32p(cj),
        _lib.i64p(cv), prior, _lib.f64p(out), ctypes.byref(flags)))
    _raise_negative(flags.value, P, "(built on the device)")
    return out


_RESIDENT_KWARGS = {"builder", "lag_time", "prior_counts"}


def relative_entropy_per_state(
        P, Q=None, assignments=None, weights=1, state_subset=None,
        base=2.0, device=0, **kwargs):
    """Per state ``i`` of a Markov state model, how far the row ``Q[i]`` of a
    second model is from the row ``P[i]`` of this one: ``kl_divergence`` of
    the two transition matrices' rows, scaled by ``weights``.

    The second model is given either as ``Q`` or as ``assignments`` to
    estimate it from; then ``kwargs`` (``lag_time``, ``builder``,
    ``prior_counts``) are ``Q_from_assignments``'s.  With its default builder
    the estimate is made on the device from the sparse counts and is never
    downloaded; the values have the bits of the two-step computation.

    Parameters
    ----------
    P : array, shape=(n_states, n_states)
        Transition probabilities of the model taken as the truth.
    Q : array, shape=(n_states, n_states), optional
        Transition probabilities of the model compared with it.
    assignments : array [n_trajectories, n_frames], list or RaggedArray, optional
    weights : float or array, shape=(n_subset,)
        Factor on every returned value.
    state_subset : index array, optional
        Return these states only.
    base : float
        2 for bits (the default), e for nats.

    Raises ``DataInvalid`` if neither ``Q`` nor ``assignments`` is given, and
    as ``kl_divergence`` does.
    """
    if Q is None and assignments is None:
        raise exception.DataInvalid(
            "Nothing to compare P with: pass Q, or assignments to estimate Q from.")
    P = _dense_matrix(P, "P")
    if P.ndim != 2:
        raise exception.DataInvalid("P is a transition matrix, not of shape %s" % (P.shape,))
    pick = Ellipsis if state_subset is None else state_subset
    resident = Q is None and set(kwargs) <= _RESIDENT_KWARGS and \
        kwargs.get("builder", builders.normalize) is builders.normalize
    if resident:
        per_state = _kl_from_counts(P, assignments, P.shape[0], kwargs.get("lag_time", 1),
                                    kwargs.get("prior_counts"), device)
        per_state /= np.log(base)
    else:
        if Q is None:
            Q = Q_from_assignments(assignments, n_states=P.shape[0], device=device, **kwargs)
        per_state = kl_divergence(P, Q, base=base, device=device)
    return per_state[pick] * weights


def relative_entropy_msm(
        P, Q=None, assignments=None, populations=None, state_subset=None,
        base=2.0, device=0, **kwargs):
    """One number for how far a second Markov state model is from this one:
    the per-state values of ``relative_entropy_per_state`` averaged with this
    model's equilibrium populations, ``sum_i pi_i KL(P[i] || Q[i])``.

    Arguments as for ``relative_entropy_per_state``, and

    populations : array, shape=(n_subset,), optional
        The weights ``pi`` of the states (of ``state_subset``, if given).
        Left out: the stationary distribution ``eq_probs(P)``, restricted to
        the subset and scaled to sum to one.

    The weighted sum is numpy's on the ``[n_subset]`` vector.
    """
    pick = Ellipsis if state_subset is None else state_subset
    if populations is None:
        if Q is None and assignments is None:
            raise exception.DataInvalid(
                "Nothing to compare P with: pass Q, or assignments to estimate Q from.")
        pi = eq_probs(_dense_matrix(P, "P"), device=device)[pick]
        populations = pi / pi.sum()
    weighted = relative_entropy_per_state(
        P, Q=Q, assignments=assignments, weights=populations, state_subset=state_subset,
        base=base, device=device, **kwargs)
    return np.sum(weighted)


def last_timing():
    """Milliseconds between device events of the last KL, JS or Shannon call:
    upload, building Q (the ``assignments=`` path, else 0), row kernel."""
    ms = np.zeros(3)
    _check(_lib.load().ek_ent_last_timing(_lib.f64p(ms)))
    return ms


# ---- state counts -----------------------------------------------------------------
class StateCounts(object):
    """Counts ``[n_features, n_states]`` that live on the device
    (ek_ent_state_counts of include/enspara_hip.h): ``add`` counts one
    trajectory into them, ``counts`` downloads them.  Usable as a context
    manager; ``close`` frees the device memory."""

    def __init__(self, n_features, n_states, device=0):
        self.shape = (int(n_features), _n_states(n_states, "n_states"))
        if not 1 <= self.shape[0] <= MAX_FEATURES:
            raise exception.DataInvalid(
                "%d features: the device counts 1 to %d features"
                % (self.shape[0], MAX_FEATURES))
        self._h = ctypes.c_void_p()
        self._L = _lib.load()
        _check(self._L.ek_ent_state_counts_open(int(device), self.shape[0], self.shape[1],
                                                ctypes.byref(self._h)))

    def add(self, X):
        """Count the frames of ``X`` ([frames, n_features] integers in [0, n_states))."""
        X = np.asarray(X)
        X = _codes(X.reshape(-1, 1) if X.ndim == 1 else X, self.shape[1], "X")
        if X.shape[1] != self.shape[0]:
            raise exception.DataInvalid(
                "%d features do not fit counts of shape %s" % (X.shape[1], self.shape,))
        if len(X) >= MAX_FRAMES:
            raise exception.DataInvalid(
                "No support for trajectories of %d frames or more." % MAX_FRAMES)
        _check(self._L.ek_ent_state_counts_add(self._h, _u8p(X), len(X)))
        return self

    def counts(self):
        out = np.zeros(self.shape, dtype=np.uint64)
        _check(self._L.ek_ent_state_counts_read(
            self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
        return out.astype(np.int64)

    def last_timing(self):
        """Milliseconds between device events: the last ``add``'s upload, its kernel."""
        ms = np.zeros(2)
        _check(self._L.ek_ent_state_counts_last_timing(self._h, _lib.f64p(ms)))
        return ms

    def close(self):
        if self._h:
            self._L.ek_ent_state_counts_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def state_counts(feature_trajs, n_states, device=0):
    """How often every feature was seen in each of its states.

    Parameters
    ----------
    feature_trajs : list of arrays, 3-D array or RaggedArray of [frames, features]
        State codes, one entry per trajectory (a single 2-D array is one
        trajectory).  Each is uploaded once and counted where it lands.
    n_states : int or array, shape=(n_features,)
        Number of states of each feature; an integer applies to all.

    Returns
    -------
    counts : np.ndarray, shape=(n_features, max(n_states)), int64
        ``counts[j, u]`` = the number of frames with feature ``j`` in state
        ``u``: the diagonal ``joint_counts(X, X)[j, j].sum(-1)`` of the
        reference's app, without the ``n_features^2`` pairs.  ``DataInvalid``
        if a code is no state of its feature.
    """
    if isinstance(feature_trajs, np.ndarray) and feature_trajs.ndim == 2:
        feature_trajs = [feature_trajs]
    n_vec = np.asarray(n_states)
    if n_vec.size == 0 or not np.issubdtype(n_vec.dtype, np.integer):
        raise exception.DataInvalid("n_states holds integers, got %r" % (n_states,))
    n_max = int(n_vec.max())
    sc = None
    try:
        for i, X in enumerate(feature_trajs):
            X = np.asarray(X)
            if X.ndim == 1:
                X = X.reshape(-1, 1)
            if sc is None:
                if n_vec.ndim and len(n_vec) != X.shape[-1]:
                    raise exception.DataInvalid(
                        "n_states has %d entries but the trajectories, of shape %s, "
                        "do not have that many features."
                        % (len(n_vec), X.shape,))
                sc = StateCounts(X.shape[-1], n_max, device=device)
            elif X.ndim != 2 or X.shape[1] != sc.shape[0]:
                raise exception.DataInvalid(
                    "Trajectory %d has shape %s where %d features were expected."
                    % (i, X.shape, sc.shape[0]))
            sc.add(X)
        if sc is None:
            raise exception.DataInvalid("No trajectories were given.")
        counts = sc.counts()
    finally:
        if sc is not None:
            sc.close()
    if n_vec.ndim:
        beyond = np.arange(n_max)[None, :] >= n_vec[:, None]
        if np.any(counts[beyond]):
            j = int(np.flatnonzero((counts * beyond).sum(axis=1))[0])
            raise exception.DataInvalid(
                "State indices of feature %d must lie in [0, %d)." % (j, n_vec[j]))
    return counts
