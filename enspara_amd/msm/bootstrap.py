"""Bootstrap resampling of MSMs (reference enspara/msm/bootstrap.py: bootstrap :10-48,
MSMs :51-60), with the transition counts of ALL resamples taken in one pass over the
frames on the device (csrc/ek_msm_boot.hip; the contract is DESIGN.md 4p).

A trial draws resampling units -- trajectories, or with ``chunk_by`` consecutive blocks
of them -- with replacement.  Its count matrix is ``sum_u m[trial, u] * C_u``, ``m`` being
how often the trial drew unit ``u``, so every trial's counts live on the sparsity
pattern of the full data's counts: one walk over the frames fills an integer table
``[cells of the pattern, trials]`` that stays on the device, and one more launch
row-normalises every trial (``'normalize'``, ``'transpose'``).  Integer adds are exact
in any order: the table is bit-reproducible.
"""
import collections
import ctypes as C

import numpy as np
import scipy.sparse

from .. import _lib
from ..exception import DataInvalid, InsufficientResourceError
from . import builders
from .msm import MSM
from .transition_matrices import (_INT32_MAX, _int32_arg, _rows_of, assigns_to_counts,
                                  eq_probs)
from .trimming import TrimMapping, trim_disconnected

_timing = np.zeros(3, dtype=np.float64)


def _check(rc):
    if rc == _lib.EK_ENOMEM:
        msg = _lib.load().ek_last_error().decode("utf-8", "replace")
        raise InsufficientResourceError(msg)
    _lib.check(rc)


def _generator(random_state):
    """None: numpy's global generator (np.random.seed(s) before the call reproduces the
    reference's draws); an int seeds a RandomState; a RandomState is used as it is."""
    if random_state is None:
        return np.random
    if isinstance(random_state, np.random.RandomState):
        return random_state
    if isinstance(random_state, (int, np.integer)) and not isinstance(random_state, bool):
        return np.random.RandomState(int(random_state))
    raise DataInvalid("random_state is None, an int or a numpy RandomState, not %r"
                      % (random_state,))


def resample_indices(n_units, n_trials, random_state=None):
    """The draws of ``n_trials`` bootstrap trials over ``n_units`` units: int64
    ``[n_trials, n_units]``, one ``choice(np.arange(n_units), n_units)`` per trial in
    trial order, exactly as the reference draws them (bootstrap.py:35-37)."""
    for name, v in (("n_units", n_units), ("n_trials", n_trials)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise DataInvalid("%s = %r is not a positive integer" % (name, v))
    rng = _generator(random_state)
    draws = [rng.choice(np.arange(n_units), n_units) for _ in np.arange(n_trials)]
    return np.array(draws, dtype=np.int64).reshape(int(n_trials), int(n_units))


def _integer_rows(data):
    """``data`` of bootstrap(): a 2-D integer array, or a list of 1-D integer arrays"""
    if isinstance(data, np.ndarray) and data.dtype != object:
        arrays = [data]
        if data.ndim != 2:
            raise DataInvalid("data is a 2-D integer array or a list of 1-D integer "
                              "arrays, not an array of shape %s" % (data.shape,))
    else:
        arrays = [np.asarray(r) for r in data]
    for a in arrays:
        if not np.issubdtype(a.dtype, np.integer):
            raise DataInvalid(
                "Given array (type '%s') is not an integral type (e.g. int32). "
                "Bootstrapping requires discretized state trajectories." % a.dtype)
    return len(data)


def bootstrap(func, data, n_trials, n_procs=1, random_state=None, **kwargs):
    """Do a bootstrap sampling of ``func`` on ``data`` (reference bootstrap.py:10-48).

    Parameters
    ----------
    func : callable
        Called as ``func(resampled data, **kwargs)`` once per trial.
    data : 2-D integer array, or list of 1-D integer arrays
        The rows are what is drawn, with replacement, as many as there are.
    n_trials : int
        Number of bootstrapping trials to run.
    n_procs : int
        Accepted and ignored: the trials run one after the other (the reference forks
        a pool; ``func`` here drives one device).
    random_state : None, int or numpy RandomState
        See ``resample_indices``.

    Returns
    -------
    list : ``[func(data[idx], **kwargs) for idx in draws]``
    """
    n_units = _integer_rows(data)
    indices = resample_indices(n_units, n_trials, random_state)
    if isinstance(data, np.ndarray):
        return [func(data[idx], **kwargs) for idx in indices]
    return [func([data[i] for i in idx], **kwargs) for idx in indices]


class _Units(object):
    """the resampling units as assigns_to_counts takes a ragged array"""

    def __init__(self, flat, lengths):
        self._data = flat
        self.lengths = lengths

    def pick(self, idx):
        starts = np.concatenate([[0], np.cumsum(self.lengths)])
        return [self._data[starts[i]:starts[i + 1]] for i in idx]


def _units_of(assigns, chunk_by):
    """-> (flat states, int64 lengths of the resampling units)"""
    flat, lengths = _rows_of(assigns)
    if chunk_by is None:
        return flat, lengths
    if isinstance(chunk_by, bool) or not isinstance(chunk_by, (int, np.integer)) or chunk_by < 1:
        raise DataInvalid("chunk_by = %r is not a positive integer" % (chunk_by,))
    k = int(chunk_by)
    out = []
    for n in lengths.tolist():
        out.extend([k] * (n // k))
        if n % k:
            out.append(n % k)
    return flat, np.array(out, dtype=np.int64)


def _indices_arg(indices, n_units):
    idx = np.asarray(indices)
    if idx.ndim != 2 or idx.shape[0] < 1 or idx.shape[1] < 1 or \
            not np.issubdtype(idx.dtype, np.integer):
        raise DataInvalid("indices is an integer array [n_trials, n_draws] with at least "
                          "one trial and one draw, not %s of shape %s" % (idx.dtype, idx.shape))
    if idx.min() < 0 or idx.max() >= n_units:
        raise DataInvalid("indices draw units %d .. %d; there are %d units"
                          % (idx.min(), idx.max(), n_units))
    return np.ascontiguousarray(idx, dtype=np.int64)


def _pattern_lookup(rows, cols, n, want_rows, want_cols):
    """index of every (want_rows, want_cols) in the pattern sorted by (row, col); -1: none"""
    key = rows.astype(np.int64) * n + cols
    want = want_rows.astype(np.int64) * n + want_cols
    pos = np.searchsorted(key, want)
    pos_c = np.minimum(pos, max(len(key) - 1, 0))
    hit = (pos < len(key)) & (key[pos_c] == want) if len(key) else np.zeros(len(want), bool)
    return np.where(hit, pos_c, -1).astype(np.int64)


BootstrapBuild = collections.namedtuple(
    "BootstrapBuild", ["rows", "cols", "idx_ij", "idx_ji", "probs", "rowsums"])


class BootstrapCounts(object):
    """The transition counts of every trial, resident on the device: what
    ``bootstrap_counts`` returns.  A context manager; ``close()`` releases the table.

    Attributes
    ----------
    indices : int64 [n_trials, n_draws], the draws
    rows, cols : int32 [nnz], the shared sparsity pattern, sorted by (row, col)
    full : coo_matrix, the counts of the full data
    n_states, n_trials, n_units
    """

    def __init__(self, assigns, lag_time, n_trials=None, indices=None, max_n_states=None,
                 sliding_window=True, chunk_by=None, random_state=None, device=0,
                 _chunk=256):
        self._h = None
        flat, lengths = _units_of(assigns, chunk_by)
        self.n_units = len(lengths)
        if self.n_units < 1:
            raise DataInvalid("there is nothing to resample: no units")
        if indices is None:
            if n_trials is None:
                raise DataInvalid("give n_trials (the draws are made here) or indices")
            indices = resample_indices(self.n_units, n_trials, random_state)
        else:
            indices = _indices_arg(indices, self.n_units)
            if n_trials is not None and int(n_trials) != indices.shape[0]:
                raise DataInvalid("n_trials = %s, indices holds %d trials"
                                  % (n_trials, indices.shape[0]))
        self.indices = indices
        self.n_trials = int(indices.shape[0])
        longest = int(lengths.max())
        if indices.shape[1] * longest > _INT32_MAX:
            raise DataInvalid("%d draws of units of up to %d frames: a cell of the int32 "
                              "table could reach 2^31" % (indices.shape[1], longest))
        if isinstance(_chunk, bool) or not isinstance(_chunk, (int, np.integer)) or _chunk < 1:
            raise DataInvalid("_chunk = %r is not a positive integer" % (_chunk,))
        self._units = _Units(flat, lengths)
        self.device = _int32_arg("device", device)
        # the full data's counts: the pattern every trial lives on (this also checks the
        # lag, the labels and max_n_states as assigns_to_counts does)
        self.full = assigns_to_counts(self._units, lag_time, max_n_states=max_n_states,
                                      sliding_window=sliding_window, device=self.device)
        self.n_states = int(self.full.shape[0])
        self.rows = np.ascontiguousarray(self.full.row, dtype=np.int32)
        self.cols = np.ascontiguousarray(self.full.col, dtype=np.int32)
        self.nnz = int(len(self.rows))
        if self.nnz == 0:
            return                  # no transition anywhere: every trial's table is empty
        R = (self.n_trials + 63) // 64 * 64
        mult = np.bincount(
            (indices * R + np.arange(self.n_trials)[:, None]).ravel(),
            minlength=self.n_units * R).astype(np.int32).reshape(self.n_units, R)
        indptr = np.zeros(self.n_states + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.rows, minlength=self.n_states), out=indptr[1:])
        a32 = np.ascontiguousarray(flat, dtype=np.int32)
        lengths = np.ascontiguousarray(lengths, dtype=np.int64)
        h = C.c_void_p()
        L = _lib.load()
        _check(L.ek_msm_boot_open(
            self.device, _lib.i32p(a32), _lib.i64p(lengths), self.n_units,
            _int32_arg("lag_time", lag_time), 1 if sliding_window else 0, self.n_states,
            self.nnz, _lib.i64p(indptr), _lib.i32p(self.cols), self.n_trials,
            _lib.i32p(mult), _int32_arg("_chunk", _chunk), C.byref(h)))
        self._h = h
        _timing[:] = 0.0
        self._read_timing()

    def _read_timing(self):
        _check(_lib.load().ek_msm_boot_last_timing(self._h, _lib.f64p(_timing)))

    def close(self):
        if getattr(self, "_h", None):
            _lib.load().ek_msm_boot_close(self._h)
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

    def units(self, r):
        """the units trial ``r`` drew, as a list of arrays, in the order drawn"""
        return self._units.pick(self.indices[r])

    def values(self, r0=0, r1=None):
        """int64 ``[r1 - r0, nnz]``: the counts of trials ``r0 .. r1 - 1`` on the pattern"""
        r1 = self.n_trials if r1 is None else r1
        if not 0 <= r0 <= r1 <= self.n_trials:
            raise DataInvalid("trials [%s, %s) of %d" % (r0, r1, self.n_trials))
        out = np.zeros((r1 - r0, self.nnz), dtype=np.int64)
        if self.nnz and r1 > r0:
            if not self._h:
                raise DataInvalid("the table is closed")
            _check(_lib.load().ek_msm_boot_fetch(self._h, int(r0), int(r1), _lib.i64p(out)))
        return out

    def _coo(self, v, n=None):
        keep = v != 0
        n = self.n_states if n is None else n
        return scipy.sparse.coo_matrix(
            (v[keep].astype(int), (self.rows[keep], self.cols[keep])), shape=(n, n))

    def matrix(self, r):
        """the counts of trial ``r`` as ``assigns_to_counts`` returns them: a coo_matrix
        sorted by (row, col), cells the trial never saw dropped"""
        return self._coo(self.values(r, r + 1)[0])

    def build(self, method):
        """Row-normalise every trial in one launch.  ``method``: ``'normalize'`` (the
        counts as they are) or ``'transpose'`` (``C + C.T``).  Returns a
        ``BootstrapBuild``: the pattern ``rows`` / ``cols`` of the result (the shared one,
        or its union with its transpose), ``idx_ij`` / ``idx_ji`` = where cell (i, j) and
        cell (j, i) sit in ``self.rows`` / ``self.cols`` (-1: nowhere), ``probs`` float64
        ``[n_trials, cells]`` and ``rowsums`` float64 ``[n_trials, n_states]``, the exact
        row sums of what was normalised."""
        if method not in ("normalize", "transpose"):
            raise DataInvalid("build() batches 'normalize' and 'transpose', not %r" % (method,))
        n = self.n_states
        if method == "normalize":
            rows, cols = self.rows, self.cols
            idx_ij = np.arange(self.nnz, dtype=np.int64)
            idx_ji = np.full(self.nnz, -1, dtype=np.int64)
        else:
            key = np.union1d(self.rows.astype(np.int64) * n + self.cols,
                             self.cols.astype(np.int64) * n + self.rows)
            rows, cols = (key // n).astype(np.int32), (key % n).astype(np.int32)
            idx_ij = _pattern_lookup(self.rows, self.cols, n, rows, cols)
            idx_ji = _pattern_lookup(self.rows, self.cols, n, cols, rows)
        probs = np.zeros((self.n_trials, len(rows)), dtype=np.float64)
        rowsums = np.zeros((self.n_trials, n), dtype=np.float64)
        if len(rows):
            if not self._h:
                raise DataInvalid("the table is closed")
            indptr = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
            _check(_lib.load().ek_msm_boot_build(
                self._h, len(rows), _lib.i64p(indptr), _lib.i64p(idx_ij), _lib.i64p(idx_ji),
                _lib.f64p(probs), _lib.f64p(rowsums)))
            self._read_timing()
        return BootstrapBuild(rows, cols, idx_ij, idx_ji, probs, rowsums)


def bootstrap_counts(assigns, lag_time, n_trials=None, indices=None, max_n_states=None,
                     sliding_window=True, chunk_by=None, random_state=None, device=0,
                     _chunk=256):
    """Count the transitions of every bootstrap trial in one pass over the frames.

    Parameters
    ----------
    assigns : 2-D integer array, ragged list of 1-D arrays, or ``ra``-like object
        The trajectories, as ``assigns_to_counts`` takes them from the host; ``-1``
        frames are dropped per unit before pairing.
    lag_time : int
    n_trials : int, default=None
        Draw this many trials here (``resample_indices``); or give ``indices``.
    indices : integer array [n_trials, n_draws], default=None
        The units each trial draws; any number of draws per trial (>= 1).
    max_n_states : int, default=None
        By default one more than the largest label of the data.
    sliding_window : bool, default=True
    chunk_by : int, default=None
        The resampling units are consecutive blocks of ``chunk_by`` frames of each
        trajectory (the last block of a trajectory may be shorter and is kept);
        transitions never cross a block's end, exactly as when the list of blocks is
        passed as trajectories.  (The reference's ``_chunk_assignments`` is a stub that
        returns None: its ``chunk_by`` raises AttributeError.)
    random_state : None, int or numpy RandomState
    device : int

    Returns
    -------
    BootstrapCounts : holds the table ``[cells, trials]`` (int32, ``cells x trials
        rounded up to 64 x 4`` bytes of device memory) until closed.

    Raises
    ------
    DataInvalid : indices out of range, neither ``n_trials`` nor ``indices``, or
        ``n_draws x (longest unit)`` could reach 2^31 (a cell of the table could
        overflow).
    """
    return BootstrapCounts(assigns, lag_time, n_trials=n_trials, indices=indices,
                           max_n_states=max_n_states, sliding_window=sliding_window,
                           chunk_by=chunk_by, random_state=random_state, device=device,
                           _chunk=_chunk)


_FAST = {"normalize": "normalize", "transpose": "transpose",
         builders.normalize: "normalize", builders.transpose: "transpose"}


def _fast_method(method):
    try:
        return _FAST.get(method)
    except TypeError:               # an unhashable callable
        return None


def MSMs(assignments, lag_time, method, n_trials=None, max_n_states=None, n_procs=1,
         chunk_by=None, trim=False, indices=None, random_state=None, device=0):
    """Bootstrapped MSMs (reference bootstrap.py:51-60): a list of fitted ``MSM``, trial
    ``r`` equal to ``MSM.from_assignments([units[i] for i in indices[r]], lag_time=...,
    method=..., max_n_states=..., trim=...)``.

    With ``method`` ``'normalize'`` / ``'transpose'`` (or the builders of that name) and
    ``trim=False`` the counts of all trials come from one ``bootstrap_counts`` and their
    probabilities from one batched build: no kernel runs per trial for either
    (``'normalize'`` then calls ``eq_probs`` per trial for the populations;
    ``'transpose'`` takes them from the batched row sums).  Any other method, and
    ``trim=True``, loop over the trials' count matrices with the existing builders.
    ``chunk_by``: see ``bootstrap_counts``.  ``n_procs`` is accepted and ignored."""
    with BootstrapCounts(assignments, lag_time, n_trials=n_trials, indices=indices,
                         max_n_states=max_n_states, chunk_by=chunk_by,
                         random_state=random_state, device=device) as bc:
        # (max_n_states=None: a per-trial call sizes its matrix by the units it drew)
        if max_n_states is None:
            tops = np.array([int(u[u != -1].max()) + 1 if (u != -1).any() else 0
                             for u in bc._units.pick(range(bc.n_units))], dtype=np.int64)
            sizes = tops[bc.indices].max(axis=1)
        else:
            sizes = np.full(bc.n_trials, bc.n_states, dtype=np.int64)
        models = [MSM(lag_time=lag_time, method=method, trim=trim,
                      max_n_states=max_n_states, device=device) for _ in range(bc.n_trials)]
        fast = None if trim else _fast_method(method)
        if fast is None:
            for r, m in enumerate(models):
                counts = bc._coo(bc.values(r, r + 1)[0], int(sizes[r]))
                if trim:
                    m.mapping_, counts = trim_disconnected(counts)
                else:
                    m.mapping_ = TrimMapping(zip(range(counts.shape[0]),
                                                 range(counts.shape[0])))
                m.tcounts_, m.tprobs_, m.eq_probs_ = m.method(counts)
            return models
        b = bc.build(fast)
        batch = max(1, min(bc.n_trials, (1 << 24) // max(bc.nnz, 1)))
        for r0 in range(0, bc.n_trials, batch):
            vals = bc.values(r0, min(bc.n_trials, r0 + batch))
            for r in range(r0, r0 + len(vals)):
                t, m, n = vals[r - r0], models[r], int(sizes[r])
                m.mapping_ = TrimMapping(zip(range(n), range(n)))
                if fast == "normalize":
                    v = t
                else:
                    v = np.where(b.idx_ij >= 0, t[b.idx_ij], 0) + \
                        np.where(b.idx_ji >= 0, t[b.idx_ji], 0)
                keep = v != 0
                ij = (b.rows[keep], b.cols[keep])
                probs = scipy.sparse.coo_matrix((b.probs[r][keep], ij), shape=(n, n))
                counts = scipy.sparse.coo_matrix((v[keep].astype(int), ij), shape=(n, n))
                if fast == "normalize":
                    m.tcounts_, m.tprobs_ = counts, probs
                    m.eq_probs_ = eq_probs(probs, device=device)
                else:
                    # builders.transpose's own expressions on the batched row sums
                    rs = b.rowsums[r][:n].astype(np.int64)
                    m.tcounts_, m.tprobs_ = counts / 2, probs
                    m.eq_probs_ = np.array(rs / rs.sum()).flatten()
        return models


def last_timing():
    """Kernel milliseconds between device events of the last table and build: the
    squeeze and the cells, the scatter, the batched build (ek_msm_boot_last_timing)."""
    return _timing.copy()
