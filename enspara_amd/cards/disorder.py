"""Transition statistics and order / disorder states (reference
enspara/cards/disorder.py) on the device (csrc/ek_cards.hip).

The reference loops in Python over trajectories x features x transitions.  Here
a trajectory's state codes are uploaded once and stay on the device; per
trajectory and feature the device returns four integers ``(n, first, last, s2)``
-- the number of transitions, the first and last transition frame and the sum
of ``w (w + 1) / 2`` over the waiting times ``w = [first, differences ...]`` --
from which ``traj_ord_disord_times`` follows bit for bit (``times_from_stats``).
The likelihood-ratio decision of ``create_disorder_traj`` depends only on the
feature and on the integer span between two transitions, and is monotone in the
span, so per feature the disordered spans form one interval ``[lo, hi]``
(``disorder_interval``, found on the host with numpy's own ``exp`` in the
reference's expression); the device then assigns the states with integer
compares.

Where this differs from the reference, on purpose:

* State codes are checked to lie in ``[0, n)``, trajectories to have the same
  width and fewer than 2^26 frames (``MAX_FRAMES``: ``s2`` stays an exact
  integer below 2^53), at least one frame each: else ``DataInvalid``.
* ``transitions`` of a 2-D or ragged array has one row per input row, also
  where the last rows have no transition (the reference's ``bincount`` drops
  them).
* ``transition_stats`` computes the ragged transition times on the host from
  the arrays it was given (the device holds only the four integers).
"""
import numbers

import numpy as np

from .. import _lib, exception, ra

__all__ = ["transitions", "traj_ord_disord_times", "create_disorder_traj",
           "assign_order_disorder", "transition_stats", "aggregate_mean_times",
           "disorder_interval", "times_from_stats", "CardsStates", "MAX_FRAMES"]

# frames of one chunk of the device's scans (CARDS_CHUNK of csrc/ek_cards.hip; a multiple
# of the rotamer scan's, enspara_amd.geometry.rotamer.SCAN_CHUNK)
SCAN_CHUNK = 2048
# frames of one trajectory
MAX_FRAMES = 2 ** 26
MAX_STATES = 255


def _check(rc):
    if rc == _lib.EK_ENOMEM:
        msg = _lib.load().ek_last_error().decode("utf-8", "replace")
        raise exception.InsufficientResourceError(msg)
    _lib.check(rc)


# ---- host functions of the reference -----------------------------------------------------
def transitions(assignments):
    """The frames at which a state transition occurs: ``t`` where frames ``t``
    and ``t + 1`` differ.  1-D input gives an array, 2-D input or a
    ``RaggedArray`` (one trajectory per row) a ``RaggedArray`` of one row each."""
    if isinstance(assignments, ra.RaggedArray):
        rows = [np.asarray(r) for r in assignments]
    else:
        assignments = np.asarray(assignments)
        if assignments.ndim == 1:
            return np.where(assignments[1:] != assignments[:-1])[0]
        rows = list(assignments)
    tt = [np.where(r[1:] != r[:-1])[0] for r in rows]
    flat = np.concatenate(tt) if tt else np.zeros(0, dtype=np.int64)
    return ra.RaggedArray(flat, lengths=[len(t) for t in tt])


def traj_ord_disord_times(transition_times):
    """Order and disorder times of one trajectory from the times of its
    transitions -> (ord_time, n_ord, disord_time, n_disord), as the reference:
    the disorder time is the mean time between events, the order time the mean
    waiting time until an event from any starting point."""
    tt = np.asarray(transition_times)
    n = tt.shape[0]
    ord_time = n_ord = disord_time = n_disord = 0.0
    if n == 1:
        n_ord = tt[0]
        ord_time = tt[0] * (tt[0] + 1.0) / 2
    elif n > 1:
        gaps = np.diff(tt)
        disord_time = gaps.mean()
        waits = np.array([tt[0].tolist()] + gaps.tolist())
        ord_time = (waits * (waits + 1.0) / 2).sum() / waits.sum()
        n_disord = tt[-1] - tt[0]
        n_ord = tt[-1]
    return ord_time, n_ord, disord_time, n_disord


def create_disorder_traj(transition_times, traj_len, ord_time, disord_time):
    """The order (0) / disorder (1) states of one feature of one trajectory: the
    frames between two neighbouring transitions are disordered where the
    likelihood ratio ``ord / dis * exp(-span * (1 / dis - 1 / ord))`` is at
    least 3.  float64 ``[traj_len]``, as the reference."""
    tt = np.asarray(transition_times)
    traj = np.zeros(traj_len)
    with np.errstate(all="ignore"):
        for i in range(tt.shape[0] - 1):
            span = tt[i + 1] - tt[i]
            ratio = ord_time / disord_time * np.exp(
                -span * (1. / disord_time - 1. / ord_time))
            if ratio >= 3.0:
                traj[tt[i]:tt[i + 1]] = 1.
    return traj


def aggregate_mean_times(times, n_times, weight):
    """The mean of the trajectories' times ``[n_trajectories, n_features]``,
    weighted by ``weight / sum(weight)`` (usually the trajectory lengths).
    ``n_times`` is accepted and, as in the reference, not used."""
    times = np.asarray(times, dtype=np.float64)
    weight = np.asarray(weight)
    mean_times = np.zeros(times.shape[1])
    nl_weight = weight / np.sum(weight)
    with np.errstate(all='ignore'):
        for i in range(times.shape[1]):
            mean_times[i] = ((times[:, i] * nl_weight).sum())
    return mean_times


# ---- the device's integers -> the reference's numbers ------------------------------------
def times_from_stats(stats):
    """``stats`` [..., 4] int64 = (n, first, last, s2) -> (ord_time, n_ord,
    disord_time, n_disord) float64 arrays: ``traj_ord_disord_times`` of the
    transition times behind them, bit for bit."""
    stats = np.asarray(stats, dtype=np.int64)
    n, first, last, s2 = (stats[..., k] for k in range(4))
    one, many = n == 1, n > 1
    w = first.astype(np.float64)
    ord_time = np.where(one, w * (w + 1.0) / 2, 0.0)
    with np.errstate(all="ignore"):
        ord_time = np.where(many, s2.astype(np.float64) / last.astype(np.float64), ord_time)
        dis = np.where(many, (last - first).astype(np.float64) / (n - 1), 0.0)
    n_ord = np.where(one, first, np.where(many, last, 0)).astype(np.float64)
    n_dis = np.where(many, last - first, 0).astype(np.float64)
    return ord_time, n_ord, dis, n_dis


def _likelihood(ord_time, disord_time, span):
    return ord_time / disord_time * np.exp(-span * (1. / disord_time - 1. / ord_time))


def disorder_interval(ord_time, disord_time, max_span=MAX_FRAMES):
    """Per feature the spans ``s`` in ``[1, max_span]`` that
    ``create_disorder_traj`` calls disordered, as one interval ``lo <= s <=
    hi`` (int64 arrays; empty: ``lo = 1, hi = 0``).  The likelihood ratio is
    monotone in ``s``: with ``ord > dis`` it falls, the interval is ``s <= hi``;
    with ``ord < dis`` it grows, ``s >= lo``; with ``ord == dis`` it is 1 and
    the interval empty.  The threshold is found by bisection on the reference's
    own expression."""
    o = np.atleast_1d(np.asarray(ord_time, dtype=np.float64))
    d = np.atleast_1d(np.asarray(disord_time, dtype=np.float64))
    big = np.int64(max_span)
    with np.errstate(all="ignore"):
        falling = ~((1. / d - 1. / o) < 0)

        def yes(s):
            return _likelihood(o, d, s) >= 3.0

        at_1, at_max = yes(np.ones(len(o), dtype=np.int64)), yes(np.full(len(o), big))
        # a: the predicate is known to hold at a (falling) / fail at a (growing); b the
        # other way round; the threshold lies between them
        a = np.ones(len(o), dtype=np.int64)
        b = np.full(len(o), big, dtype=np.int64)
        while np.any(b - a > 1):
            mid = a + (b - a) // 2
            y = yes(mid)
            left = np.where(falling, y, ~y)     # the threshold is right of mid
            a = np.where(left, mid, a)
            b = np.where(left, b, mid)
    lo = np.ones(len(o), dtype=np.int64)
    hi = np.zeros(len(o), dtype=np.int64)
    # falling: holds on [1, a] if it holds at 1 (everywhere if it holds at max_span)
    f_ok = falling & at_1
    hi = np.where(f_ok, np.where(at_max, big, a), hi)
    # growing: holds on [b, max_span] if it holds at max_span (everywhere if at 1)
    g_ok = ~falling & at_max
    lo = np.where(g_ok, np.where(at_1, 1, b), lo)
    hi = np.where(g_ok, big, hi)
    return lo, hi


# ---- the device handle ----------------------------------------------------------------------
def _n_states(n_feature_states, width):
    n = np.asarray(n_feature_states)
    if n.ndim == 0:
        n = np.full(width, n)
    if n.shape != (width,) or not np.issubdtype(n.dtype, np.integer):
        raise exception.DataInvalid(
            "The number-of-states vector (shape %s, %s) does not fit state assignments of "
            "width %d." % (n.shape, n.dtype, width))
    if n.min() < 1 or n.max() > MAX_STATES:
        raise exception.DataInvalid(
            "Features have 1 to %d states, got %d .. %d" % (MAX_STATES, n.min(), n.max()))
    # (int64: numpy's log of an int16, the type of the reference's state numbers, is a float32)
    return n.astype(np.int64)


def check_feature_trajs(feature_trajs, n_feature_states=None):
    """The trajectories as C-contiguous uint8 ``[frames, F]`` arrays and the
    vector of state numbers, or ``DataInvalid``: before any device call."""
    trajs = [np.asarray(t) for t in feature_trajs]
    if not trajs:
        raise exception.DataInvalid("No trajectories were given.")
    for i, t in enumerate(trajs):
        if t.ndim != 2 or t.shape[1] < 1:
            raise exception.DataInvalid(
                "Trajectory %d is [frames, features], not %s" % (i, t.shape,))
        if not issubclass(t.dtype.type, numbers.Integral):
            raise exception.DataInvalid(
                "Trajectory %d holds state indices, not %s" % (i, t.dtype))
    widths = [t.shape[1] for t in trajs]
    if len(set(widths)) > 1:
        raise exception.DataInvalid(
            "The number of features differs between trajectories. "
            "Numbers of features were: %s." % widths)
    if n_feature_states is None:
        n_feature_states = np.full(widths[0], max(int(t.max()) for t in trajs if t.size) + 1
                                   if any(t.size for t in trajs) else 1)
    n = _n_states(n_feature_states, widths[0])
    for i, t in enumerate(trajs):
        if len(t) < 1 or len(t) >= MAX_FRAMES:
            raise exception.DataInvalid(
                "Trajectory %d has %d frames: 1 to 2^26 - 1 are supported." % (i, len(t)))
        if t.min() < 0 or np.any(t >= n[None, :]):
            raise exception.DataInvalid(
                "State indices of trajectory %d must lie in [0, n) of their feature; "
                "found %d .. %d." % (i, t.min(), t.max()))
    if sum(len(t) for t in trajs) >= 2 ** 32:
        raise exception.DataInvalid("No support for 2^32 frames or more in all.")
    return [np.ascontiguousarray(t, dtype=np.uint8) for t in trajs], n


class CardsStates(object):
    """The state codes of a set of trajectories resident on the device (ek_cards of
    include/enspara_hip.h): ``add`` uploads one trajectory and computes its
    transition statistics, ``disorder`` assigns the disorder states from the
    per-feature intervals, ``matrices`` counts S-S, D-D, S-D and D-S and returns
    their mutual information.  Usable as a context manager."""

    def __init__(self, n_features, n_states, device=0):
        import ctypes as C
        self.n_features, self.n_states = int(n_features), int(n_states)
        if self.n_features < 1 or not 1 <= self.n_states <= MAX_STATES:
            raise exception.DataInvalid(
                "%d features of %d states: at least one feature, 1 to %d states"
                % (self.n_features, self.n_states, MAX_STATES))
        self.lengths = []
        self._h = C.c_void_p()
        self._L = _lib.load()
        _check(self._L.ek_cards_open(int(device), self.n_features, self.n_states,
                                     C.byref(self._h)))

    def add(self, X):
        """Upload ``X`` (uint8 ``[frames, F]``, validated by the caller)."""
        X = np.ascontiguousarray(X, dtype=np.uint8)
        if X.ndim != 2 or X.shape[1] != self.n_features or not 1 <= len(X) < MAX_FRAMES:
            raise exception.DataInvalid(
                "A trajectory of shape %s does not fit %d features and 1 to 2^26 - 1 frames"
                % (X.shape, self.n_features))
        _check(self._L.ek_cards_add(self._h, _lib.u8p(X), len(X)))
        self.lengths.append(len(X))
        return self

    def stats(self):
        """int64 ``[trajectories, F, 4]`` = (n, first, last, s2)."""
        out = np.zeros((len(self.lengths), self.n_features, 4), dtype=np.int64)
        if len(self.lengths):
            _check(self._L.ek_cards_stats(self._h, _lib.i64p(out)))
        return out

    def mean_times(self):
        """-> (mean ordered times, mean disordered times) ``[F]``, the
        reference's ``aggregate_mean_times`` of the per-trajectory times."""
        ord_t, n_ord, dis_t, n_dis = times_from_stats(self.stats())
        lengths = np.array(self.lengths)
        return (aggregate_mean_times(ord_t, n_ord, lengths),
                aggregate_mean_times(dis_t, n_dis, lengths))

    def disorder(self, lo, hi):
        lo = np.ascontiguousarray(lo, dtype=np.int64)
        hi = np.ascontiguousarray(hi, dtype=np.int64)
        if lo.shape != (self.n_features,) or hi.shape != (self.n_features,):
            raise exception.DataInvalid("one interval per feature")
        _check(self._L.ek_cards_disorder(self._h, _lib.i64p(lo), _lib.i64p(hi)))
        return self

    def disorder_codes(self, traj):
        out = np.zeros((self.lengths[traj], self.n_features), dtype=np.uint8)
        _check(self._L.ek_cards_disorder_codes(self._h, int(traj), _lib.u8p(out)))
        return out

    def matrices(self):
        """float64 ``[4, F, F]``: the mutual information (not normalised) of S-S,
        D-D, S-D, D-S."""
        out = np.zeros((4, self.n_features, self.n_features), dtype=np.float64)
        _check(self._L.ek_cards_matrices(self._h, _lib.f64p(out)))
        return out

    def counts(self, which):
        """The joint counts behind matrix ``which`` (after ``matrices``)."""
        F, n = self.n_features, self.n_states
        shape = [(F, F, n, n), (F, F, 2, 2), (F, F, n, 2), (F, F, 2, n)][which]
        out = np.zeros(shape, dtype=np.uint32)
        _check(self._L.ek_cards_counts(self._h, int(which), _lib.u32p(out)))
        return out

    def last_timing(self):
        """Milliseconds between device events: the last ``add``'s upload and pack,
        its statistics kernels; the last ``disorder``; of the last ``matrices``
        the S-S, D-D and S-D count passes, the transpose and the four
        information kernels."""
        ms = np.zeros(8)
        _check(self._L.ek_cards_last_timing(self._h, _lib.f64p(ms)))
        return ms

    def close(self):
        if self._h:
            self._L.ek_cards_close(self._h)
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


def _resident(rotamer_trajs, n_feature_states, device):
    trajs, n = check_feature_trajs(rotamer_trajs, n_feature_states)
    d = CardsStates(trajs[0].shape[1], int(n.max()), device=device)
    try:
        for t in trajs:
            d.add(t)
    except Exception:
        d.close()
        raise
    return d, trajs, n


def transition_stats(rotamer_trajs, device=0):
    """-> (transition_times, mean_ordered_times, mean_disordered_times):
    per trajectory and feature the frames at which a transition occurs (a list
    of lists of arrays), and per feature the mean ordered and disordered time
    over the trajectories, weighted by their lengths."""
    d, trajs, _ = _resident(rotamer_trajs, None, device)
    with d:
        mean_ord, mean_dis = d.mean_times()
    times = [[np.where(t[1:, j] != t[:-1, j])[0] for j in range(t.shape[1])] for t in trajs]
    return times, mean_ord, mean_dis


def assign_order_disorder(rotamer_trajs, device=0):
    """Assign each frame an ordered (0) or disordered (1) state.

    Returns
    -------
    disordered_trajs : list of int16 arrays ``[frames, n_features]``
    disorder_n_states : int16 array ``[n_features]`` of 2s
    """
    d, trajs, _ = _resident(rotamer_trajs, None, device)
    with d:
        d.disorder(*disorder_interval(*d.mean_times()))
        out = [d.disorder_codes(i).astype(np.int16) for i in range(len(trajs))]
    return out, 2 * np.ones(trajs[0].shape[1], dtype='int16')
