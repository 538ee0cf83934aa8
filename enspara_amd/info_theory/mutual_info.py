"""Mutual information between discrete features (reference
enspara/info_theory/mutual_info.py and libinfo.pyx) on the device.

The joint counts ``jc[i, j, u, v] = sum_t [X[t, i] == u] [Y[t, j] == v]`` are
the product of two one-hot matrices; csrc/ek_mi.hip takes it on the int8 matrix
cores without ever storing a one-hot array, and computes the mutual information
of every feature pair from the counts where they lie.  ``mi_matrix`` uploads
each trajectory once, keeps the counts on the device and downloads the
``[Fx, Fy]`` matrix once.  The ``mi_to_*`` conversions, the channel-capacity
normalisation and ``deconvolute_network`` are ``[F, F]`` work in numpy, as in
the reference.

Where this differs from the reference, on purpose:

* State codes are checked: every code of ``X`` lies in ``[0, n_x)`` (``Y``:
  ``n_y``), else ``DataInvalid`` -- the reference asserts on codes that are too
  large and writes out of bounds on negative ones.
* A feature has at most 255 states (``MAX_STATES``; the device holds codes as
  bytes and 255 pads the frame axis); more is ``DataInvalid``.
* The observations of one count array stay below 2^32 (the counts are uint32,
  as in the reference); more is ``DataInvalid`` where the reference wraps.
* A side has at most 65535 * 64 features (``MAX_FEATURES``) and one upload
  fewer than 2^31 - 64 frames; more is ``DataInvalid``.
* Counts that do not fit the device's free memory raise
  ``InsufficientResourceError``.
* ``mutual_information`` follows the reference operation for operation, in
  float64, terms added ``u`` outer, ``v`` inner; only ``log`` may differ from
  numpy's, in its last bit.  A pair without observations gives 0.  Nothing is
  mirrored: like the reference's, the matrix of ``X`` against itself is
  symmetric only to rounding (``P_x * P_y`` and ``P_y * P_x`` are the same, but
  the terms of ``[i, j]`` and ``[j, i]`` are added in different orders), so
  entries may differ from their transpose in the last bits.
* ``channel_capacity_normalization`` divides ``mi[i, j]`` by
  ``log(min(n_x[i], n_y[j]))``, as its documentation says.  The reference
  builds that table with ``meshgrid(n_x, n_y)``, which is its transpose: the
  same wherever ``n_x`` and ``n_y`` are equal or plain integers, an error for a
  matrix that is not square, and the other feature's capacity for a square one
  with unequal state vectors.
* ``weighted_mi`` (csrc/ek_wmi.hip) raises ``DataInvalid`` where the reference
  asserts (negative weights, weights that sum to zero, arrays of the wrong
  rank), for weights that are not finite, for a code outside ``[0, n)`` of its
  own feature and for more than ``MAX_STATES`` states.  Its joint probabilities
  are float64 sums over the frames on the matrix cores, in a fixed order (the
  same bits every run) that is not numpy's: within ``frames * 2^-52`` relative
  of the exact sum.  The marginals are the same sums (``P[i, i, u, u]``).
  The default numbers of states are int64 where the reference's are int16,
  which makes numpy take the channel capacity's logarithm in float32.
"""
import logging
import numbers
import warnings

import numpy as np

from .. import _lib, exception

logger = logging.getLogger(__name__)

__all__ = ["mi_matrix", "mi_matrix_serial", "joint_counts", "mutual_information",
           "mi_to_nmi_apc", "deconvolute_network", "mi_to_nmi", "mi_to_apc",
           "channel_capacity_normalization", "check_features_states", "JointCounts",
           "weighted_joint_probabilities", "weighted_mi", "weighted_mi_last_timing"]

# frames one workgroup of the count kernel takes (MI_CHUNK of csrc/ek_mi.hip)
MI_CHUNK = 16384
# frames of one chunk of the weighted product, up to 64 chunks (WMI_CHUNK of
# csrc/ek_wmi.hip; longer input is cut into 64 longer chunks)
WMI_CHUNK = 2048
# states per feature (MI_MAX_STATES of csrc/ek_mi.hip)
MAX_STATES = 255
# features of one side (MI_MAX_FEATURES of csrc/ek_mi.hip: the pack kernel's grid)
MAX_FEATURES = 65535 * 64
# frames of one upload, and observations of one count array
MAX_FRAMES = 2 ** 31 - 64
MAX_OBSERVATIONS = 2 ** 32


def _check(rc):
    if rc == _lib.EK_ENOMEM:
        msg = _lib.load().ek_last_error().decode("utf-8", "replace")
        raise exception.InsufficientResourceError(msg)
    _lib.check(rc)


def _n_states(n, what):
    if not isinstance(n, numbers.Integral) or isinstance(n, bool):
        raise exception.DataInvalid("%s is an integer, not %r" % (what, n))
    n = int(n)
    if n < 1:
        raise exception.DataInvalid("%s must be at least 1, got %d" % (what, n))
    if n > MAX_STATES:
        raise exception.DataInvalid(
            "%s = %d: the device counts at most %d states per feature"
            % (what, n, MAX_STATES))
    return n


def _codes(X, n, what):
    """``X`` ([frames, features] integers in [0, n)) as C-contiguous uint8."""
    if X.ndim != 2:
        raise exception.DataInvalid(
            "%s is [frames] or [frames, features], not %s" % (what, X.shape,))
    if not issubclass(X.dtype.type, numbers.Integral):
        raise exception.DataInvalid(
            "%s holds state indices, not %s" % (what, X.dtype))
    if X.shape[1] < 1:
        raise exception.DataInvalid("%s has no features" % what)
    if X.size and (X.min() < 0 or X.max() >= n):
        raise exception.DataInvalid(
            "State indices of %s must lie in [0, %d); found %d .. %d."
            % (what, n, X.min(), X.max()))
    return np.ascontiguousarray(X, dtype=np.uint8)


def _u8p(a):
    import ctypes as C
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _u32p(a):
    import ctypes as C
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


class JointCounts(object):
    """Joint counts ``[Fx, Fy, n_x, n_y]`` that live on the device (ek_mi of
    include/enspara_hip.h): ``add`` counts one trajectory into them,
    ``counts`` downloads them, ``mutual_information`` works on them in place.
    Usable as a context manager; ``close`` frees the device memory."""

    def __init__(self, n_features_x, n_features_y, n_x, n_y, device=0):
        import ctypes as C
        self.shape = (int(n_features_x), int(n_features_y),
                      _n_states(n_x, "n_x"), _n_states(n_y, "n_y"))
        if not 1 <= min(self.shape[:2]) <= max(self.shape[:2]) <= MAX_FEATURES:
            raise exception.DataInvalid(
                "%d x %d features: the device counts 1 to %d features a side"
                % (self.shape[0], self.shape[1], MAX_FEATURES))
        self.n_observations = 0
        self._h = C.c_void_p()
        self._L = _lib.load()
        _check(self._L.ek_mi_open(int(device), self.shape[0], self.shape[1],
                                  self.shape[2], self.shape[3], C.byref(self._h)))

    def add(self, X, Y=None):
        """Count the frames of ``X`` ([frames, Fx]) against ``Y`` ([frames,
        Fy]; None: ``X`` against itself)."""
        X = _codes(np.asarray(X), self.shape[2], "X")
        shape = (X.shape[1], X.shape[1] if Y is None else np.asarray(Y).shape[-1])
        if Y is not None:
            Y = _codes(np.asarray(Y), self.shape[3], "Y")
            if len(Y) != len(X):
                raise exception.DataInvalid(
                    "Feature arrays X and Y must match in length (%d and %d frames)."
                    % (len(X), len(Y)))
        if shape != self.shape[:2] or (Y is None and self.shape[2] != self.shape[3]):
            raise exception.DataInvalid(
                "%s x %s features do not fit joint counts of shape %s"
                % (shape[0], shape[1], self.shape,))
        if len(X) >= MAX_FRAMES:
            raise exception.DataInvalid(
                "No support for trajectories of %d frames or more." % MAX_FRAMES)
        if self.n_observations + len(X) >= MAX_OBSERVATIONS:
            raise exception.DataInvalid(
                "No support for more than 2^32 - 1 observations per joint counts "
                "array (%d + %d)." % (self.n_observations, len(X)))
        _check(self._L.ek_mi_add(self._h, _u8p(X), None if Y is None else _u8p(Y),
                                 len(X)))
        self.n_observations += len(X)
        return self

    def load(self, jc):
        """Replace the counts by ``jc`` (integers, this shape)."""
        jc = np.asarray(jc)
        if jc.shape != self.shape:
            raise exception.DataInvalid(
                "counts of shape %s do not fit %s" % (jc.shape, self.shape))
        if not issubclass(jc.dtype.type, numbers.Integral):
            raise exception.DataInvalid("Joint counts are integers, not %s." % jc.dtype)
        if jc.size and jc.min() < 0:
            raise exception.DataInvalid("Joint counts must not be negative.")
        if jc.size and int(jc.sum(axis=(2, 3), dtype=np.uint64).max()) >= MAX_OBSERVATIONS:
            raise exception.DataInvalid(
                "No support for more than 2^32 - 1 observations per feature pair.")
        largest = int(jc.sum(axis=(2, 3), dtype=np.uint64).max()) if jc.size else 0
        jc = np.ascontiguousarray(jc, dtype=np.uint32)
        _check(self._L.ek_mi_load_counts(self._h, _u32p(jc), largest))
        # (what a later add() has to stay below 2^32 with: the fullest pair)
        self.n_observations = largest
        return self

    def counts(self):
        out = np.zeros(self.shape, dtype=np.uint32)
        _check(self._L.ek_mi_counts(self._h, _u32p(out)))
        return out

    def mutual_information(self):
        out = np.zeros(self.shape[:2], dtype=np.float64)
        _check(self._L.ek_mi_information(self._h, _lib.f64p(out)))
        return out

    def last_timing(self):
        """Milliseconds between device events: the last ``add``'s upload and
        pack, its count kernel, the last ``mutual_information``'s kernel."""
        ms = np.zeros(3)
        _check(self._L.ek_mi_last_timing(self._h, _lib.f64p(ms)))
        return ms

    def close(self):
        if self._h:
            self._L.ek_mi_close(self._h)
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


def _as_columns(a):
    a = np.asarray(a)
    return a.reshape(-1, 1) if a.ndim == 1 else a


def _prepare_xy(X, Y, n_x, n_y):
    """joint_counts' arguments as it documents them -> (X, Y, n_x, n_y): 1-D
    input is one feature, a missing number of states is ``max + 1``, and the
    reference's two warnings (``n_y`` without ``Y``; integer types that
    differ) are raised with its words.  ``Y`` stays None for X against
    itself, with ``n_y = n_x``."""
    X = _as_columns(X)
    alone = Y is None
    Y = None if alone else _as_columns(Y)
    if alone and n_y is not None:
        warnings.warn("n_y unused if Y is None.")
    if not alone and X.dtype != Y.dtype:
        warnings.warn("Feature trajs (types %s and %s) being uptyped to match."
                      % (X.dtype, Y.dtype), exception.PerformanceWarning)

    def states(a, n, what):
        if n is not None:
            return int(n) if isinstance(n, np.integer) else n
        if a.size == 0:
            raise exception.DataInvalid(
                "%s is empty and its number of states is not given" % what)
        return int(a.max()) + 1

    n_x = states(X, n_x, "X")
    n_y = n_x if alone else states(Y, n_y, "Y")
    return X, Y, n_x, n_y


def joint_counts(X, Y=None, n_x=None, n_y=None, device=0):
    """Compute the array of joint counts matrices between X and Y (or itself.)

    Parameters
    ----------
    X : np.ndarray, shape=(n_observations, n_features) or (n_observations,)
        Assignments to discrete states; integers of any width.
    Y : np.ndarray, shape=(n_observations, n_features), default=None
        As X; None: joint counts between X and itself.
    n_x, n_y : int, default=None
        Number of possible states in X / Y; ``max + 1`` if unspecified.
    device : int
        The HIP device.

    Returns
    -------
    jc : np.ndarray, shape=(n_features_x, n_features_y, n_x, n_y), uint32
        Cell [i, j, u, v] holds the number of times feature i of X was in
        state u while feature j of Y was in state v.  Exact.
    """
    X, Y, n_x, n_y = _prepare_xy(X, Y, n_x, n_y)
    fy = X.shape[-1] if Y is None else Y.shape[-1]
    with JointCounts(X.shape[-1], fy, n_x, n_y, device=device) as jc:
        return jc.add(X, Y).counts()


def mutual_information(jc, device=0):
    """Compute the mutual information of a matrix of joint counts matrices.

    Parameters
    ----------
    jc : ndarray of integers, shape=(n_feat_x, n_feat_y, n_x, n_y), or JointCounts
        Cell (i, j, u, v) is the number of times feature i was seen in state
        u and feature j in state v.  A ``JointCounts`` is used where it lies.
    device : int
        The HIP device (for counts given as an array).

    Returns
    -------
    mutual_information : np.ndarray, shape=(n_feat_x, n_feat_y), float64

    See the module's docstring for the order of operations and the symmetry.
    """
    if isinstance(jc, JointCounts):
        return jc.mutual_information()
    jc = _validate_joint_counts_matrix(np.asarray(jc))
    if 0 in jc.shape:
        raise exception.DataInvalid("Joint counts of shape %s are empty." % (jc.shape,))
    with JointCounts(*jc.shape, device=device) as d:
        return d.load(jc).mutual_information()


def mi_matrix(Xs, Ys, n_x, n_y, normalize=True, device=0):
    """Compute the all-to-all matrix of mutual information across
    trajectories of assigned states.

    Parameters
    ----------
    Xs, Ys : list of arrays, 3-D array or RaggedArray of [frames, features]
        Assigned/binned features, one entry per trajectory.
    n_x, n_y : int or array, shape=(n_features,)
        Number of possible states of each feature of Xs / Ys; an integer
        applies to all features.
    normalize : bool, default=True
        Normalize by channel capacity.
    device : int
        The HIP device.

    Returns
    -------
    mi : np.ndarray, shape=(n_features_x, n_features_y), float64

    Every trajectory is uploaded once and counted into counts that stay on
    the device; the matrix is downloaded once.
    """
    jc = None
    try:
        for i, (X, Y) in enumerate(zip(Xs, Ys)):
            logger.debug("counting trajectory %d on the device", i)
            X, Y, nx, ny = _prepare_xy(X, Y, int(np.max(n_x)), int(np.max(n_y)))
            shape = (X.shape[-1], Y.shape[-1], nx, ny)
            if jc is None:
                jc = JointCounts(*shape, device=device)
            elif jc.shape != shape:
                raise exception.DataInvalid(
                    ("Trajectory %s gave a joint "
                     "counts matrix of shape %s where %s was expected. "
                     "Are you sure all your trajectories have the same "
                     "number of features?") % (i, shape, jc.shape))
            jc.add(X, Y)
        if jc is None:
            raise exception.DataInvalid("No trajectories were given.")
        mi = jc.mutual_information()
    finally:
        if jc is not None:
            jc.close()

    if normalize:
        mi = channel_capacity_normalization(mi, n_x, n_y)

    return mi


def mi_matrix_serial(states_a_list, states_b_list, n_a_states, n_b_states,
                     normalize=True, device=0):
    """The mutual information matrix one feature pair at a time: a
    cross-check of ``mi_matrix`` composed from ``joint_counts`` and
    ``mutual_information`` on single columns.  Like the reference's
    (:182-209) it visits the pairs ``i <= j`` only and mirrors them, so it
    fits square problems whose two sides hold the same features."""
    n_features = np.asarray(states_a_list[0]).shape[1]
    mi = np.zeros((n_features, n_features))
    for i, j in zip(*np.triu_indices(n_features)):
        pair = np.zeros((1, 1, int(n_a_states[i]), int(n_b_states[j])), dtype=np.uint64)
        for a, b in zip(states_a_list, states_b_list):
            pair += joint_counts(np.asarray(a)[:, i], np.asarray(b)[:, j],
                                 int(n_a_states[i]), int(n_b_states[j]), device=device)
        mi[i, j] = mi[j, i] = mutual_information(pair, device=device)[0, 0]
    if normalize:
        mi = channel_capacity_normalization(mi, n_a_states, n_b_states)
    return mi


# ---- weighted frames ----------------------------------------------------------------
def _weighted_args(features, weights):
    """-> (features [T, F] integers, weights [T] float64, checked as the
    reference asserts)"""
    features, weights = np.asarray(features), np.array(weights, dtype=np.float64)
    if features.ndim != 2:
        raise exception.DataInvalid(
            "features is [observations, features], not %s" % (features.shape,))
    if weights.ndim != 1:
        raise exception.DataInvalid("weights is [observations], not %s" % (weights.shape,))
    if features.dtype == np.bool_:
        features = features.astype(np.uint8)
    if weights.shape[0] != features.shape[0]:
        raise exception.DataInvalid(
            "The number of features (%s in array with shape %s) didn't match "
            "the number of weights (%s)" %
            (features.shape[0], features.shape, weights.shape[0]))
    if features.shape[0] < 1 or features.shape[1] < 1:
        raise exception.DataInvalid("features of shape %s are empty." % (features.shape,))
    if not np.all(np.isfinite(weights)) or np.any(weights < 0):
        raise exception.DataInvalid("Weights must be finite and not negative.")
    if not weights.sum() > 0:
        raise exception.DataInvalid("Weights must not sum to zero.")
    return features, weights


def _weighted_run(features, weights, n_states, want_P, want_mi, device):
    S = _n_states(n_states, "the number of states")
    codes = _codes(features, S, "features")
    T, F = codes.shape
    if T >= MAX_FRAMES or F > MAX_FEATURES:
        raise exception.DataInvalid(
            "No support for %d frames x %d features (fewer than %d frames, at most %d "
            "features)." % (T, F, MAX_FRAMES, MAX_FEATURES))
    weights = np.ascontiguousarray(weights, dtype=np.float64)
    P = np.zeros((F, F, S, S)) if want_P else None
    mi = np.zeros((F, F)) if want_mi else None
    _check(_lib.load().ek_wmi_run(int(device), _u8p(codes), _lib.f64p(weights), T, F, S,
                                  None if P is None else _lib.f64p(P),
                                  None if mi is None else _lib.f64p(mi)))
    return P, mi


def weighted_joint_probabilities(features, weights, n_states, device=0):
    """Joint probabilities of weighted observations.

    Parameters
    ----------
    features : np.ndarray, shape=(n_observations, n_features), bool or integers
        State of every feature in every observation, in ``[0, n_states)``.
    weights : np.ndarray, shape=(n_observations,)
        Weight of each observation; used as given (not normalised).
    n_states : int
        Number of states of every feature.

    Returns
    -------
    P : np.ndarray, shape=(n_features, n_features, n_states, n_states), float64
        ``P[i, j, u, v]`` = the sum of the weights of the observations with
        feature i in state u and feature j in state v (``joint_counts``'
        layout).
    """
    features, weights = _weighted_args(features, weights)
    return _weighted_run(features, weights, n_states, True, False, device)[0]


def weighted_mi(features, weights, n_feature_states=None, normalize=True, device=0):
    """Compute a mutual information matrix using weighted observations.

    The marginal and joint probability distributions P(x), P(y) and P(x, y)
    of every pair of features are sums of the observations' weights.

    Parameters
    ----------
    features : np.ndarray, shape=(n_observations, n_features), bool or integers
        Observations of multiple variables (features) between which to
        compute the pairwise mutual information.
    weights : np.ndarray, shape=(n_observations,)
        Probability distribution across observations; divided by its sum
        (L1 norm) if that is not 1.
    n_feature_states : np.ndarray, shape=(n_features,), default=None
        The number of states each feature can take on (used for
        normalization).  If None, ``features.max() + 1`` for every feature.
    normalize : bool, default=True
        Normalize by channel capacity.

    Returns
    -------
    mi : np.ndarray, shape=(n_features, n_features), float64
        Cell i, j is the mutual information between features i and j, not
        below 0.
    """
    features, weights = _weighted_args(features, weights)
    if weights.sum() != 1:
        weights = weights / np.linalg.norm(weights, ord=1)
    if n_feature_states is None:
        n_feature_states = np.full(features.shape[1], int(features.max()) + 1, dtype=np.int64)
    else:
        n_feature_states = np.array(n_feature_states)
    if n_feature_states.ndim != 1 or n_feature_states.shape[0] != features.shape[1]:
        raise exception.DataInvalid(
            "The length of feature states number vector (%s) must equal the"
            "number of features given (%s)" % (
                n_feature_states.shape[0] if n_feature_states.ndim else "scalar",
                features.shape[1]))
    if not np.issubdtype(n_feature_states.dtype, np.integer):
        raise exception.DataInvalid(
            "Numbers of states are integers, not %s." % n_feature_states.dtype)
    if features.min() < 0 or np.any(features.max(axis=0) >= n_feature_states):
        raise exception.DataInvalid(
            "State indices of every feature must lie in [0, n) of its number of states n.")
    mi = _weighted_run(features, weights, int(n_feature_states.max()), False, True, device)[1]
    if normalize:
        mi = channel_capacity_normalization(mi, n_feature_states, n_feature_states)
    np.clip(mi, a_min=0, a_max=np.inf, out=mi)
    return mi


def weighted_mi_last_timing():
    """Milliseconds between device events of the last weighted run: upload and
    pack, product kernel, reduction, information kernel (ek_wmi_last_timing)."""
    ms = np.zeros(4)
    _check(_lib.load().ek_wmi_last_timing(_lib.f64p(ms)))
    return ms


# ---- [F, F] work on the host ------------------------------------------------------
def mi_to_apc(mi_arr):
    """Average product correlation of a mutual information matrix (Dunn et
    al, Bioinformatics 24, 2008): ``APC[i, j] = sum_r MI[i, r] MI[r, j] / F^2``,
    the background every pair shares through the rest of the features."""
    _validate_mutual_information_matrix(mi_arr)
    n = mi_arr.shape[0]
    return (mi_arr @ mi_arr) / (n * n)


def mi_to_nmi(mutual_information, H_marginal=None):
    """Mutual information over the joint entropy of each pair,
    ``NMI[i, j] = MI[i, j] / (H[i] + H[j] - MI[i, j])``.

    ``H_marginal`` holds the features' own entropies; by default they are
    read off the diagonal (the mutual information of a feature with itself).
    The diagonal of the result is 1, pairs of zero joint entropy give 0, and
    the argument is left as it was."""
    _validate_mutual_information_matrix(mutual_information)
    H = np.diag(mutual_information) if H_marginal is None else np.asarray(H_marginal)
    if np.any(H == 0):
        warnings.warn('H_marginal contains zero entries. This may lead to '
                      'negative information.')
    if len(H) != len(mutual_information):
        raise exception.DataInvalid(
            "H_marginal must be the same length as the mutual "
            "information matrix. Got %s and %s." % (len(H), len(mutual_information)))
    n_zero, n_nan = np.count_nonzero(H == 0), np.count_nonzero(np.isnan(H))
    if n_zero == len(H) or n_nan:
        raise exception.DataInvalid(
            'The mutual information matrix must have non-zero entries '
            'and cannot contain any nan values. Found %s zero entries '
            'and %s nan entries.' % (n_zero, n_nan))

    filled = np.array(mutual_information, dtype=np.float64)
    np.fill_diagonal(filled, H)
    H_joint = (H[:, None] + H[None, :]) - filled
    with np.errstate(divide="ignore", invalid="ignore"):
        nmi = filled / H_joint
    nmi[np.isnan(nmi)] = 0          # 0 / 0: no joint entropy, no information
    np.fill_diagonal(nmi, 1)
    return nmi


def mi_to_nmi_apc(mutual_information, H_marginal=None):
    """NMI-APC (Lopez et al, Nat. Struct. Mol. Biol. 24, 2017): the mutual
    information less its average product correlation, over the joint entropy,
    ``(MI - APC) / H_joint``.  The joint entropy is recovered from
    ``mi_to_nmi`` as ``MI / NMI``; where that is undefined the result is 0.

    ``H_marginal`` as for ``mi_to_nmi``."""
    _validate_mutual_information_matrix(mutual_information)
    excess = mutual_information - mi_to_apc(mutual_information)
    nmi = mi_to_nmi(mutual_information, H_marginal)
    with np.errstate(all="ignore"):
        H_joint = np.reciprocal(nmi) * mutual_information
        out = excess / H_joint
    out[np.isnan(out)] = 0
    return out


def deconvolute_network(G_obs):
    """Network deconvolution (Feizi et al, Nat. Biotechnol. 31, 2013).  An
    observed network that sums direct effects and all their chains,
    ``G_obs = G_dir + G_dir^2 + ... = G_dir (I - G_dir)^-1``, has the
    eigenvectors of ``G_dir`` and the eigenvalues ``l / (1 - l)``; mapping each
    observed eigenvalue back by ``l_obs / (1 + l_obs)`` gives ``G_dir``."""
    lam, V = np.linalg.eig(G_obs)
    return (V * (lam / (1 + lam))[None, :]) @ np.linalg.inv(V)


def channel_capacity_normalization(mi, n_x, n_y):
    """Scale ``mi[i, j]`` ([Fx, Fy]) by the capacity of the narrower of the
    two features, ``log(min(n_x[i], n_y[j]))``: what a feature of that many
    states can carry at most.  ``n_x`` / ``n_y``: one integer for all
    features of a side, or one per feature.  Returns a new array.  (See the
    module's docstring for how the reference differs.)"""
    n_x = _validate_feature_states_array(n_x, mi.shape[0])
    n_y = _validate_feature_states_array(n_y, mi.shape[1])
    return mi / np.log(np.minimum(n_x[:, None], n_y[None, :]))


def check_features_states(states, n_states):
    """``DataInvalid`` unless every trajectory of ``states`` has one column
    per entry of ``n_states``."""
    widths = [len(traj[0]) for traj in states]
    if widths[0] != len(n_states):
        raise exception.DataInvalid(
            ("The number-of-states vector's length ({s}) didn't match the "
             "width of state assignments array with shape {a}.")
            .format(s=len(n_states), a=widths[0]))
    if len(set(widths)) > 1:
        raise exception.DataInvalid(
            ("The number of features differs between trajectories. "
             "Numbers of features were: {l}.").format(l=widths))


def _validate_joint_counts_matrix(jc):
    """``jc`` if it has the four axes [Fx, Fy, n_x, n_y]."""
    if jc.ndim == 2:
        raise exception.DataInvalid(
            "Expected a 4D array of joint counts matrices, but got a 2D "
            " array. If your dataset is a single joint counts matrix, "
            "try `jc[None, None, ...]` to expand its dimensions.")
    if jc.ndim != 4:
        raise exception.DataInvalid(
            "Expected a 4D array of joint counts matrices, but an array "
            "with shape %s." % (jc.shape,))
    return jc


def _validate_mutual_information_matrix(mi):
    """The conversions take a square matrix equal to its transpose bit for
    bit (symmetrise the device's result first: module docstring)."""
    if mi.ndim != 2:
        raise exception.DataInvalid('MI arrays must be 2D. Got %s.' % mi.ndim)
    if mi.shape[0] != mi.shape[1]:
        raise exception.DataInvalid(
            "Mutual information matrices must be square; got shape %s." % (mi.shape,))
    n_diff = np.count_nonzero(mi != mi.T)
    if n_diff:
        raise exception.DataInvalid(
            "Mutual information matrices must be symmetric; found "
            "differences at %s positions." % n_diff)


def _validate_feature_states_array(n, mi_dim):
    """Numbers of states as an integer vector of length ``mi_dim``, every
    entry at least 2 (one state carries nothing: log 1 = 0)."""
    n = np.full(mi_dim, n) if np.ndim(n) == 0 else np.asarray(n)
    if len(n) != mi_dim:
        raise exception.DataInvalid(
            "Feature states array must match mi array dim 0 "
            "(got %s and %s)" % (len(n), mi_dim))
    if not np.issubdtype(n.dtype, np.integer):
        raise exception.DataInvalid(
            "Feature states array must be integral (got %s)." % n.dtype)
    if np.any(n < 2):
        raise exception.DataInvalid(
            'Cannot normalize channel capacity for n_states < 1, got: %s' % n)
    return n
