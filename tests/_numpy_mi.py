"""A numpy restatement of joint counts and mutual information (reference
enspara/info_theory/libinfo.pyx matrix_bincount2d and mutual_info.py:290-327), the
expected values of tests/test_gpu_mi.py.

Counts: the float64 product of two one-hot matrices, exact below 2^53.  Mutual
information: the reference's numpy operations in the reference's order (marginals as
integer sums, P = count / n_obs, terms with a zero P skipped, P_xy * log(P_xy / (P_x *
P_y)) added u outer, v inner), plus S[i, j] = the sum of the terms' magnitudes, the
scale of the error bound.
"""
import numpy as np

U = 2.0 ** -52


def one_hot(X, n):
    """[frames, F] codes -> [frames, F * n] float64, column f * n + u = [X[:, f] == u]"""
    X = np.asarray(X)
    if X.ndim == 1:
        X = X[:, None]
    return (X[:, :, None] == np.arange(n)[None, None, :]).reshape(len(X), -1).astype(
        np.float64)


def joint_counts(X, Y=None, n_x=None, n_y=None):
    X = np.asarray(X)
    if X.ndim == 1:
        X = X[:, None]
    if n_x is None:
        n_x = int(X.max()) + 1
    if Y is None:
        Y, n_y = X, n_x
    else:
        Y = np.asarray(Y)
        if Y.ndim == 1:
            Y = Y[:, None]
        if n_y is None:
            n_y = int(Y.max()) + 1
    fx, fy = X.shape[1], Y.shape[1]
    jc = np.zeros((fx * n_x, fy * n_y))
    # (in slabs of frames: the one-hot matrices of a long trajectory are large)
    for t in range(0, len(X), 1 << 16):
        jc += one_hot(X[t:t + (1 << 16)], n_x).T @ one_hot(Y[t:t + (1 << 16)], n_y)
    assert jc.max(initial=0) < 2.0 ** 32
    return jc.reshape(fx, n_x, fy, n_y).transpose(0, 2, 1, 3).astype(np.uint32)


def mutual_information(jc, perturb=None):
    """-> (mi [Fx, Fy], S [Fx, Fy]).  perturb (a RandomState): every log moved by one
    ulp in a random direction, to see how far a log that is 1 ulp off can carry."""
    jc = np.asarray(jc)
    n_obs_a_i = jc.sum(axis=-1)
    n_obs_b_i = jc.sum(axis=-2)
    n_obs = n_obs_a_i.sum(axis=-1)
    safe = np.where(n_obs > 0, n_obs, 1)
    P_a = np.divide(n_obs_a_i, safe[..., None])
    P_b = np.divide(n_obs_b_i, safe[..., None])
    P_a_b = np.divide(jc, safe[..., None, None])
    mi = np.zeros(shape=jc.shape[0:2])
    S = np.zeros(shape=jc.shape[0:2])
    for i in range(jc.shape[0]):
        for j in range(jc.shape[1]):
            P_x_y, P_x, P_y = P_a_b[i, j], P_a[i, j], P_b[i, j]
            for u in range(P_x_y.shape[0]):
                for v in range(P_x_y.shape[1]):
                    if P_x_y[u, v] == 0 or P_x[u] == 0 or P_y[v] == 0:
                        continue
                    lg = np.log(P_x_y[u, v] / (P_x[u] * P_y[v]))
                    if perturb is not None:
                        lg = np.nextafter(lg, np.inf if perturb.rand() < 0.5 else -np.inf)
                    term = P_x_y[u, v] * lg
                    mi[i, j] += term
                    S[i, j] += abs(term)
    return mi, S


def mi_bound(n_x, n_y, S):
    """|mi_dev - mi_np| <= (n_x n_y + 4) 2^-52 S: each log within one ulp of numpy's,
    so each term within ~3 roundings of itself; n_x n_y sequential adds of slightly
    different terms round differently by at most one ulp of the running sum each."""
    return (n_x * n_y + 4) * U * S


def biased_codes(rng, frames, F, n, dtype=np.int64):
    """feature i biased towards state i % n: asymmetric on purpose"""
    X = rng.randint(0, n, size=(frames, F))
    hit = rng.rand(frames, F) < 0.4
    X = np.where(hit, (np.arange(F) % n)[None, :], X)
    return X.astype(dtype)


def noisy_copy(rng, Y, X, ycol, xcol, n_y, flip=0.1):
    """column ycol of Y = column xcol of X (mod n_y), a tenth of it redrawn"""
    c = X[:, xcol] % n_y
    redraw = rng.rand(len(c)) < flip
    Y[:, ycol] = np.where(redraw, rng.randint(0, n_y, size=len(c)), c)
    return Y
