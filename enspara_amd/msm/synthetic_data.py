"""Kinetic Monte Carlo on a transition matrix and the time evolution of an
ensemble (reference enspara/msm/synthetic_data.py) on the device.

A step of a chain is numpy's ``Generator.choice(n_states, 1, p=T[state])`` fed
one double: the first entry of ``cumsum(row) / cumsum(row)[-1]`` that exceeds
it.  The doubles come from Philox4x32-10 keyed by the seed and counted by
(chain, step), so what a chain visits depends on ``(seed, chain index, step)``
alone: not on how many chains a call holds, which kernel form runs them or how
the steps are cut into launches (csrc/ek_kmc.hip).  The
reference seeds ``default_rng()`` from the OS on every call and cannot be
reproduced; here an integer ``random_state`` reproduces a run, and ``None``
draws a seed from the OS that stays readable as ``last_seed``.

The device holds the rows of ``T`` compressed to their nonzero entries
(``indptr``, ``cols`` and the normalised CDF, built once per ``Sampler`` on the
host with numpy so that its bits are ``np.cumsum(nonzeros) / last``); dense and
scipy-sparse ``T`` take the same path and give the same states.

Where this differs from the reference, on purpose:

* a row of ``T`` with no nonzero entry is accepted (states of a trimmed model
  that nothing enters); a chain that has to step from one raises
  ``DataInvalid`` naming the state;
* a ``T`` that is not square, has negative or NaN entries, or a row whose sum
  is off 1 by more than ``sqrt(eps)`` raises ``DataInvalid`` before any device
  call (the reference fails inside ``rng.choice``);
* ``synthetic_ensemble`` sums ``p T`` in a fixed order on the device, so its
  result differs from the reference's BLAS / scipy product by rounding, within
  the bound of DESIGN.md 4k.
"""
import ctypes
import os

import numpy as np
import scipy.sparse

from .. import _lib, exception

__all__ = ["synthetic_trajectory", "synthetic_trajectories", "synthetic_ensemble",
           "sample_next", "Sampler", "last_seed", "last_timing"]

#: the seed of the last call that drew chains (an int; None before the first)
last_seed = None

_ATOL = float(np.sqrt(np.finfo(np.float64).eps))    # numpy's tolerance on sum(p) == 1
_FORMS = {"auto": 0, "lane": 1, "wave": 2}


def _check(rc):
    _lib.check(rc)


def _seed(random_state):
    """-> the 64-bit seed: ``random_state`` itself, or 8 bytes from the OS"""
    global last_seed
    if random_state is None:
        seed = int.from_bytes(os.urandom(8), "little")
    elif isinstance(random_state, (int, np.integer)) and not isinstance(random_state, bool) \
            and 0 <= int(random_state) < 2 ** 64:
        seed = int(random_state)
    else:
        raise exception.DataInvalid(
            "random_state is None or an integer in [0, 2^64), got %r" % (random_state,))
    last_seed = seed
    return seed


def _square(T):
    if getattr(T, "ndim", None) is None:
        T = np.asarray(T)
    if T.ndim != 2 or T.shape[0] != T.shape[1] or T.shape[0] < 1:
        raise exception.DataInvalid(
            "T is a square transition matrix, not of shape %s" % (T.shape,))
    if T.shape[0] >= 2 ** 31 - 1:
        raise exception.DataInvalid("No support for %d states." % T.shape[0])
    return T


def _check_entries(data, what):
    data = np.asarray(data)
    if data.size and not np.all(data >= 0):        # (NaN fails the comparison too)
        raise exception.DataInvalid("%s has negative or NaN entries." % what)


def _check_sums(sums, what):
    """``sums``: the sums of the rows that have a nonzero entry"""
    off = np.abs(sums - 1.0) > _ATOL
    if np.any(off) or not np.all(np.isfinite(sums)):
        i = int(np.flatnonzero(off | ~np.isfinite(sums))[0])
        raise exception.DataInvalid(
            "%s do not sum to 1 (the first that does not sums to %r)." % (what, sums[i]))


def compress_rows(T):
    """``T`` (dense or scipy sparse, validated) -> ``(indptr int64 [n + 1], cols
    int32 [nnz], cdf float64 [nnz])``: per row the columns of its nonzero
    entries, ascending, and ``np.cumsum(nonzeros) / last``."""
    T = _square(T)
    n = T.shape[0]
    if scipy.sparse.issparse(T):
        csr = scipy.sparse.csr_matrix(T, dtype=np.float64, copy=True)
        csr.sum_duplicates()
        csr.sort_indices()
        _check_entries(csr.data, "T")
        csr.eliminate_zeros()
        indptr = csr.indptr.astype(np.int64)
        cols = csr.indices.astype(np.int32)
        cdf = np.empty(len(cols), dtype=np.float64)
        sums = np.ones(n)
        for i in range(n):
            lo, hi = indptr[i], indptr[i + 1]
            if hi > lo:
                c = np.cumsum(csr.data[lo:hi])
                sums[i] = c[-1]
                c /= c[-1]
                cdf[lo:hi] = c
        _check_sums(sums, "The rows of T")
    else:
        T = np.ascontiguousarray(T, dtype=np.float64)
        _check_entries(T, "T")
        mask = T != 0
        indptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int64)
        cols = np.nonzero(mask)[1].astype(np.int32)
        full = np.cumsum(T, axis=1)     # (adding 0.0 changes no bit: the nonzeros' cumsum)
        last = full[:, -1]
        _check_sums(np.where(last > 0, last, 1.0), "The rows of T")
        with np.errstate(invalid="ignore", divide="ignore"):
            full /= last[:, None]
        cdf = full[mask]
    return indptr, cols, np.ascontiguousarray(cdf)


def _states(states, n, what):
    a = np.asarray(states)
    if a.size == 0 or not (np.issubdtype(a.dtype, np.integer)):
        raise exception.DataInvalid("%s holds integers, got %r" % (what, states))
    if a.min() < 0 or a.max() >= n:
        raise exception.DataInvalid(
            "%s must lie in [0, %d); got values from %d to %d." % (what, n, a.min(), a.max()))
    return np.ascontiguousarray(a.reshape(-1), dtype=np.int32)


def _raise_bad_row(bad):
    if bad >= 0:
        raise exception.DataInvalid(
            "A chain stood on state %d, whose row of T has no nonzero entry, and had "
            "to step." % bad)


class Sampler(object):
    """The compressed rows of one transition matrix, resident on the device
    (``ek_kmc`` of include/enspara_hip.h) once the first device call is made.
    Usable as a context manager; ``close`` frees the device memory.

    Attributes ``indptr``, ``cols``, ``cdf`` are the host copies of what the
    device searches; ``last_seed`` the seed of the last call that drew chains.
    """

    def __init__(self, T, device=0):
        self.indptr, self.cols, self.cdf = compress_rows(T)
        self.n_states = len(self.indptr) - 1
        self.device = int(device)
        self.last_seed = None
        self._h = None
        self._L = None

    def _handle(self):
        if self._h is None:
            self._L = _lib.load()
            h = ctypes.c_void_p()
            _check(self._L.ek_kmc_create(self.device, self.n_states, _lib.i64p(self.indptr),
                                         _lib.i32p(self.cols), _lib.f64p(self.cdf),
                                         ctypes.byref(h)))
            self._h = h
        return self._h

    def next(self, states, u):
        """One step from each of ``states`` with the given doubles ``u`` in
        [0, 1): the column of the first CDF entry of the state's row that is
        ``> u``.  -> int32 array of ``states``' shape."""
        shape = np.shape(states)
        s = _states(states, self.n_states, "states")
        u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).reshape(-1))
        if u.shape != s.shape:
            raise exception.DataInvalid(
                "%d doubles for %d states" % (len(u), len(s)))
        if not np.all((u >= 0) & (u < 1)):
            raise exception.DataInvalid("u must lie in [0, 1).")
        out = np.empty(len(s), dtype=np.int32)
        bad = ctypes.c_int64(-1)
        h = self._handle()
        _check(self._L.ek_kmc_next(h, len(s), _lib.i32p(s), _lib.f64p(u), _lib.i32p(out),
                                   ctypes.byref(bad)))
        _raise_bad_row(bad.value)
        return out.reshape(shape)

    def trajectories(self, start_states, n_steps, random_state=None, first_chain=0,
                     dtype=np.int32, form="auto", step_cap=None):
        """``[n_chains, n_steps]`` states; see ``synthetic_trajectories``.

        form : 'auto', 'lane' (a lane per chain) or 'wave' (a wave per chain);
            the states do not depend on it.
        step_cap : int, optional
            Steps per kernel launch (the library's default if left out); the
            states do not depend on it.
        """
        start = _states(start_states, self.n_states, "start states")
        n_steps = _n_steps(n_steps)
        if form not in _FORMS:
            raise exception.DataInvalid("form is one of %s" % sorted(_FORMS))
        first_chain, cap = int(first_chain), int(step_cap or 0)
        if first_chain < 0 or first_chain + len(start) > 2 ** 60 or cap < 0:
            raise exception.DataInvalid("first_chain in [0, 2^60), step_cap > 0")
        seed = _seed(random_state)
        self.last_seed = seed
        out = np.empty((len(start), n_steps), dtype=np.int32)
        bad = ctypes.c_int64(-1)
        h = self._handle()
        _check(self._L.ek_kmc_trajectories(h, seed, first_chain, len(start), _lib.i32p(start),
                                           n_steps, _FORMS[form], cap, _lib.i32p(out),
                                           ctypes.byref(bad)))
        _raise_bad_row(bad.value)
        return out if np.dtype(dtype) == np.int32 else out.astype(dtype)

    def close(self):
        if self._h is not None:
            self._L.ek_kmc_destroy(self._h)
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


def _n_steps(n_steps):
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 1:
        raise exception.DataInvalid("n_steps is an integer >= 1, got %r" % (n_steps,))
    return int(n_steps)


def _sampler(T, device):
    """(sampler, do I own it)"""
    if isinstance(T, Sampler):
        return T, False
    return Sampler(T, device=device), True


def synthetic_trajectories(T, start_states, n_steps, random_state=None, first_chain=0,
                           dtype=np.int32, device=0, form="auto", step_cap=None):
    """Independent chains of kinetic Monte Carlo on ``T``.

    Parameters
    ----------
    T : array or scipy sparse matrix, shape=(n_states, n_states), or a Sampler
        Row-normalised transition probabilities.
    start_states : array, shape=(n_chains,)
        State every chain starts from.
    n_steps : int
        Length of every chain, its starting state included.
    random_state : int, optional
        The seed; ``None`` draws one from the OS (readable as ``last_seed``).
    first_chain : int
        Index of the first chain: chains ``[0, N)`` of one call equal chains
        ``[0, k)`` and ``[k, N)`` of two calls with ``first_chain=0`` and ``k``.

    Returns
    -------
    np.ndarray, shape=(n_chains, n_steps), of ``dtype``.  The device buffer is
    bounded; long runs are cut into chunks and launches inside the library.
    """
    sampler, own = _sampler(T, device)
    try:
        return sampler.trajectories(start_states, n_steps, random_state=random_state,
                                    first_chain=first_chain, dtype=dtype, form=form,
                                    step_cap=step_cap)
    finally:
        if own:
            sampler.close()


def synthetic_trajectory(T, start_state, n_steps, random_state=None, device=0):
    """Simulate a single trajectory using kinetic Monte Carlo.

    Parameters
    ----------
    T : array or scipy sparse matrix, shape=(n_states, n_states), or a Sampler
        A row-normalized transition probability matrix.
    start_state : int
        State to start the trajectory from.
    n_steps : int
        Number of steps in the trajectory. This includes the starting state,
        so n_steps=2 would result in a trajectory consisting of the starting
        state and one additional state.
    random_state : int, optional
        The seed (chain 0 of it); ``None`` draws one from the OS.

    Returns
    -------
    traj : array, shape=(n_steps, ), int64
        A 1-D array containing a sequence of state indices.
    """
    if np.ndim(start_state) != 0:
        raise exception.DataInvalid("start_state is one state, got %r" % (start_state,))
    return synthetic_trajectories(T, [start_state], n_steps, random_state=random_state,
                                  dtype=np.int64, device=device)[0]


def sample_next(T, states, u, device=0):
    """One step from each of ``states`` with the caller's own doubles ``u``
    (in [0, 1)): what ``np.random.default_rng().choice(n, 1, p=T[state])``
    returns when its generator hands out ``u``."""
    sampler, own = _sampler(T, device)
    try:
        return sampler.next(states, u)
    finally:
        if own:
            sampler.close()


def synthetic_ensemble(T, init_pops, n_steps, observable_per_state=None, device=0):
    """Simulate the time evolution of an ensemble: ``p <- p T`` repeated
    ``n_steps - 1`` times on the device, every ``p`` (or only ``p .
    observable``) kept there, one download.

    Parameters
    ----------
    T : array or scipy sparse matrix, shape=(n_states, n_states)
        A row-normalized transition probability matrix.  Sparse input is
        propagated in its column-compressed form.
    init_pops : array, shape=(n_states, )
        The initial probabilities of every state (not negative).
    n_steps : int
        Number of steps to advance the ensemble, the starting populations
        included.
    observable_per_state : array, shape=(n_states, ), optional
        Some observable for each state.

    Returns
    -------
    p : array, shape=(n_states,)
        The last populations.
    observations : array, shape=(n_steps, n_states) or (n_steps,)
        The populations as a function of time or, with an observable, its
        population-weighted average as a function of time.
    """
    T = _square(T)
    n = T.shape[0]
    n_steps = _n_steps(n_steps)
    p0 = np.ascontiguousarray(init_pops, dtype=np.float64)
    if p0.shape != (n,):
        raise exception.DataInvalid(
            "init_pops of shape %s do not fit %d states." % (p0.shape, n))
    _check_entries(p0, "init_pops")
    obs = None
    if observable_per_state is not None:
        obs = np.ascontiguousarray(observable_per_state, dtype=np.float64)
        if obs.shape != (n,):
            raise exception.DataInvalid(
                "observable_per_state of shape %s does not fit %d states." % (obs.shape, n))
    null = lambda t: ctypes.cast(None, ctypes.POINTER(t))      # noqa: E731
    if scipy.sparse.issparse(T):
        csc = scipy.sparse.csc_matrix(T, dtype=np.float64, copy=True)
        csc.sum_duplicates()
        csc.sort_indices()
        _check_entries(csc.data, "T")
        sums = np.asarray(csc.sum(axis=1)).reshape(-1)
        _check_sums(np.where(sums > 0, sums, 1.0), "The rows of T")
        colptr = csc.indptr.astype(np.int64)
        rows = csc.indices.astype(np.int32)
        vals = np.ascontiguousarray(csc.data, dtype=np.float64)
        mat = (null(ctypes.c_double), _lib.i64p(colptr), _lib.i32p(rows), _lib.f64p(vals))
    else:
        Td = np.ascontiguousarray(T, dtype=np.float64)
        _check_entries(Td, "T")
        sums = Td.sum(axis=1)
        _check_sums(np.where(sums > 0, sums, 1.0), "The rows of T")
        mat = (_lib.f64p(Td), null(ctypes.c_int64), null(ctypes.c_int32), null(ctypes.c_double))
    p = np.empty(n)
    out = np.empty(n_steps if obs is not None else (n_steps, n))
    _check(_lib.load().ek_kmc_ensemble(
        int(device), n, mat[0], mat[1], mat[2], mat[3], _lib.f64p(p0), n_steps,
        _lib.f64p(obs) if obs is not None else null(ctypes.c_double), _lib.f64p(p),
        _lib.f64p(out)))
    return p, out


def last_timing():
    """Milliseconds between device events of the last call: upload, kernels, download."""
    ms = np.zeros(3)
    _check(_lib.load().ek_kmc_last_timing(_lib.f64p(ms)))
    return ms
