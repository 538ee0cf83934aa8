"""numpy restatement of the reference's native feature-space distances --
TEST INFRASTRUCTURE (see oracle/__init__.py).

Follows enspara/geometry/libdist.pyx: _euclidean :122-145, _manhattan
:100-117, _hamming :77-95, as compiled (float32 input: float32 difference and
float32 square, float64 running sum in feature order).  Pinned against outputs
of the reference's own compiled module (tests/golden/features_golden.npz)."""
import numpy as np


def _work(X, y):
    X = np.asarray(X)
    y = np.asarray(y)
    if X.dtype == np.float32:
        return X, y.astype(np.float32)
    return X.astype(np.float64), y.astype(np.float64)


def euclidean(X, y):
    X, y = _work(X, y)
    acc = np.zeros(len(X), dtype=np.float64)
    for j in range(X.shape[1]):
        d = X[:, j] - y[j]                 # in the working precision
        acc = acc + (d * d).astype(np.float64)
    return np.sqrt(acc)


def manhattan(X, y):
    X, y = _work(X, y)
    acc = np.zeros(len(X), dtype=np.float64)
    for j in range(X.shape[1]):
        acc = acc + np.abs((X[:, j] - y[j]).astype(np.float64))
    return acc


def hamming(X, y):
    X = np.asarray(X)
    y = np.asarray(y)
    acc = np.zeros(len(X), dtype=np.float64)
    for j in range(X.shape[1]):
        acc = acc + (X[:, j] != y[j])
    return acc / X.shape[1]


def assign_to_nearest_center(trajectory, cluster_centers, distance_method):
    """enspara_amd.cluster.util.assign_to_nearest_center (reference
    util.py:159-205) around one of the three callables above, restated with
    one numpy pass per feature instead of one call per center: the m x K table
    of distances is built feature by feature with the operations of the
    callable (working precision, float64 sum in feature order), then the
    ascending-center strict-< scan from label 0 and distance +inf -- the first
    minimum; NaN is never taken, and a row with no distance below +inf keeps
    label 0.  Returns (assignments int64, distances float64)."""
    if distance_method not in (euclidean, manhattan, hamming):
        raise ValueError("not an oracle metric: %r" % (distance_method,))
    X = np.asarray(trajectory)
    C = np.asarray(cluster_centers)
    m, K = len(X), len(C)
    if m == 0 or K == 0:
        return np.zeros(m, dtype=np.int64), np.full(m, np.inf)
    acc = np.zeros((m, K), dtype=np.float64)
    if distance_method is hamming:
        for j in range(X.shape[1]):
            acc = acc + (X[:, j, None] != C[None, :, j])
        table = acc / X.shape[1]
    else:
        X, C = _work(X, C)
        for j in range(X.shape[1]):
            d = X[:, j, None] - C[None, :, j]
            if distance_method is euclidean:
                acc = acc + (d * d).astype(np.float64)
            else:
                acc = acc + np.abs(d.astype(np.float64))
        table = np.sqrt(acc) if distance_method is euclidean else acc
    table = np.where(np.isnan(table), np.inf, table)
    labels = np.argmin(table, axis=1).astype(np.int64)
    return labels, table[np.arange(m), labels]
