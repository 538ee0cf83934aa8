"""The eigensolver's device primitives (enspara_amd/csrc/ek_krylov.hip, through
transition_matrices.DeviceKrylov) one operation at a time against the same
operation in long double, and the solver on the device at the sizes and paths the
end-to-end tests (tests/test_gpu_msm.py) never reach.

A restarted Krylov iteration corrects itself: a wrong term in a recurrence, a norm
that misses a block, a rotation read in the wrong order still converge to the right
eigenvalues, only later.  So every check here is on ONE operation, its reference
taken from the inputs as the device holds them (what was uploaded, or downloaded
with get_vector), and every tolerance is a rounding bound of the kernel's own
summation order, written out where it is used:  u = 2^-53, and a factor 2 on every
bound for the rounding of inputs and outputs.  Where no closed bound exists
(Chebyshev recurrence, loss of orthogonality) the bound is a stated multiple of the
float64 numpy stand-in's error against the same long-double reference, measured in
the test itself."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _numpy_krylov import NumpyKrylov, NumpyKrylovExpand  # noqa: E402
from _msm_cases import _check_solver_case, _rowstoch  # noqa: E402
from enspara_amd import _lib  # noqa: E402
from enspara_amd.msm import transition_matrices as tm  # noqa: E402

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 1023, 5000, 70001]
# row lengths, cycled over the rows: empty, one entry, round the 64 lanes of the wave
# that sums a row, several trips of its loop
ROW_LENGTHS = [0, 1, 63, 64, 65, 300, 2, 7]


@pytest.fixture(scope="module", autouse=True)
def _long_double_is_wide():
    """the reference's format: 64 bits of mantissa (x87 extended), 2^11 times finer
    than the format under test"""
    assert np.finfo(LD).eps <= 2.0 ** -63


def _device(A, m_max):
    return tm.DeviceKrylov(A, m_max)


# ---- inputs ---------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _matrix(n, stochastic):
    """Seeded n x n CSR, as DeviceKrylov holds it (float64, sorted indices).  Rows of
    ROW_LENGTHS entries (capped at n), one fully dense row where 255 <= n <= 5000;
    values of mixed sign over six decades, or (stochastic) positive with unit row
    sums and no empty row."""
    rng = np.random.RandomState(1000 + n + (7 if stochastic else 0))
    lens = np.minimum(np.array(ROW_LENGTHS)[np.arange(n) % len(ROW_LENGTHS)], n)
    if stochastic:
        lens = np.maximum(lens, 1)
    if 255 <= n <= 5000:
        lens[n // 2] = n
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = np.repeat(np.arange(n), lens)
    pos = np.arange(indptr[-1]) - indptr[rows]
    # distinct columns: start + pos * stride (mod n) with len * stride <= n
    stride = 1 + rng.randint(0, np.maximum(1, n // np.maximum(lens, 1)))
    cols = (rng.randint(0, n, size=n)[rows] + pos * stride[rows]) % n
    if stochastic:
        vals = rng.uniform(0.05, 1.0, size=len(rows))
    else:
        vals = rng.standard_normal(len(rows)) * 10.0 ** rng.uniform(-3, 3, size=len(rows))
    A = scipy.sparse.csr_matrix((vals, (rows, cols)), shape=(n, n))
    if stochastic:
        A = scipy.sparse.diags(1.0 / np.asarray(A.sum(axis=1)).ravel()) @ A
    A = scipy.sparse.csr_matrix(A).astype(np.float64)
    A.sort_indices()
    assert np.array_equal(np.diff(A.indptr), lens)
    return A


def _contraction(n, stochastic):
    """_matrix scaled into the unit disc (inf-norm 1), so that a polynomial of
    degree 48 of it stays in range"""
    A = _matrix(n, stochastic)
    return scipy.sparse.csr_matrix(A / abs(A).sum(axis=1).max())


def _unit(n, seed):
    x = np.random.RandomState(seed).standard_normal(n)
    return x / np.linalg.norm(x)


def _orthonormal(cnt, n, seed):
    """[cnt, n] orthonormal rows (cnt <= n)"""
    q, _ = np.linalg.qr(np.random.RandomState(seed).standard_normal((n, cnt)))
    return np.ascontiguousarray(q.T)


def _upload(space, V, j0=0):
    for i, v in enumerate(V):
        space.set_vector(j0 + i, v)


def _download(space, lo, hi):
    return np.array([space.get_vector(j) for j in range(lo, hi)])


# ---- the operations in long double -------------------------------------------------
def _ld_product(A, x):
    """-> (A x, |A| |x|, row lengths), long double"""
    n = A.shape[0]
    t = A.data.astype(LD) * np.asarray(x, dtype=LD)[A.indices]
    y, s = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    k = np.diff(A.indptr)
    full = np.flatnonzero(k)
    if len(full):
        y[full] = np.add.reduceat(t, A.indptr[full])
        s[full] = np.add.reduceat(np.abs(t), A.indptr[full])
    return y, s, k


def _product_bound(s, k):
    """kr_spmv_kernel / kr_spmv_norm_kernel / kr_spmv_cheb_kernel: a lane adds
    ceil(k / 64) products by FMA, six levels of shuffles add the lanes"""
    return (np.ceil(k / 64.0) + 6) * U * s


def _ld_cheb(A, x, d, a, b):
    """T_d((A - c) / e) x by the three-term recurrence; c, e as the device holds them
    (float64), the arithmetic in long double"""
    c, e = LD(0.5 * (a + b)), LD(0.5 * (b - a))
    y0 = np.asarray(x, dtype=LD)
    y1 = (_ld_product(A, y0)[0] - c * y0) / e
    for _ in range(2, d + 1):
        y0, y1 = y1, 2 * (_ld_product(A, y1)[0] - c * y1) / e - y0
    return y1


def _ld_step(V, w, w_err):
    """One Arnoldi step's orthogonalisation in long double: classical Gram-Schmidt
    twice of w (long double) against the rows of V (float64, as on the device).
    w_err: elementwise bound of the device's own w against w (zero where the device
    was given w itself).
    -> (h, bound of h per entry, norm, bound of the norm); the bounds carry their
    factor 2 already.

    Coefficients (kr_dots_kernel): a thread adds ceil(n / 256) products by FMA,
    eight levels of the LDS tree add the 256 threads: (ceil(n/256) + 8) u sum|v w| on
    the first pass, the same on the second with the updated w, and what the error of
    w itself contributes, sum |v_e| w_err_e.
    Norm: the device's orthogonalised w is w - V h_dev + rho, the reference's
    w - V h_ref, so they differ by at most sum_i |dh_i| ||V_i|| + ||rho|| (+ ||w_err||),
    rho the rounding of the two chains of cnt FMAs per element (kr_axpy_kernel):
    (cnt + 1) u (|w| + |h| |V|) each; the norm of that vector is taken with a relative
    error of (ceil(n/256) + 8) u / 2 under the root, u of the root itself."""
    n = V.shape[1]
    cnt = V.shape[0]
    Vl = V.astype(LD)
    aV = np.abs(Vl)
    c = np.ceil(n / 256.0) + 8
    h1 = Vl @ w
    w1 = w - h1 @ Vl
    h2 = Vl @ w1
    w2 = w1 - h2 @ Vl
    h = h1 + h2
    hb = 2 * (c * U * (aV @ np.abs(w) + aV @ np.abs(w1)) + aV @ w_err)
    nrm = np.sqrt(w2 @ w2)
    rho = 2 * (cnt + 1) * U * (np.abs(w) + np.abs(h) @ aV)
    d = hb @ np.sqrt((Vl * Vl).sum(axis=1)) + np.sqrt(rho @ rho) + np.sqrt(w_err @ w_err)
    nb = 2 * (d + (c / 2 + 1) * U * nrm)
    return h, hb, nrm, nb


def _ld_norm(v):
    v = np.asarray(v, dtype=LD)
    return np.sqrt(v @ v)


def _assert_within(got, ref, bound, what):
    """|got - ref| <= bound elementwise; the worst ratio is printed first"""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    bound = np.asarray(bound, dtype=LD)
    bad = err > bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print("%s: max err %.3g, worst err/bound %.3g" % (what, float(err.max(initial=0)),
                                                      float(ratio.max(initial=0))))
    assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))), what
    assert not bad.any(), "%s: %d of %d outside their bound, worst err/bound %.3g" % (
        what, int(bad.sum()), bad.size, float(ratio.max()))


# ---- sparse product --------------------------------------------------------------------
def _check_product(A, seed):
    """step(0): A V[0] = h[0] V[0] + h[1] V[1].  Per element
    (ceil(k_row/64) + 6) u sum_j |a_ij x_j| for the product and 4 u (|h0 V0| + |h1 V1|)
    for the reconstruction (one rounding per pass of the update, two of the scaling
    by 1 / h1, one of h0 = h0' + h0''; on the reconstruction's own terms, not the
    row's: an empty row has an exact zero product but a rounded h0 V0 to take back)."""
    n = A.shape[0]
    space = _device(A, 1)
    try:
        x = _unit(n, 11 + n)
        space.set_vector(0, x)
        space.set_vector(1, np.zeros(n))
        h = space.step(0)
        V = _download(space, 0, 2)
    finally:
        space.close()
    assert np.array_equal(V[0], x)
    y, s, k = _ld_product(A, x)
    Vl = V.astype(LD)
    recon = LD(h[0]) * Vl[0] + LD(h[1]) * Vl[1]
    r = np.abs(LD(h[0]) * Vl[0]) + np.abs(LD(h[1]) * Vl[1])
    _assert_within(recon, y, 2 * (_product_bound(s, k) + 4 * U * r), "A x, n = %d" % n)
    return h


@pytest.mark.parametrize("stochastic", [False, True], ids=["general", "stochastic"])
@pytest.mark.parametrize("n", SIZES)
def test_sparse_product(n, stochastic):
    """kr_spmv_kernel: rows of 0, 1, 63, 64, 65, 300 and n entries, n not a multiple
    of the four rows of a workgroup"""
    A = _matrix(n, stochastic)
    if n >= 255:
        assert {0 if not stochastic else 1, 63, 64, 65}.issubset(set(np.diff(A.indptr)))
        assert np.diff(A.indptr).max() == (n if n <= 5000 else 300)
    _check_product(A, n)


def test_sparse_product_of_an_empty_matrix():
    """nnz == 0: the product is an exact zero vector, the step reports a zero norm"""
    for n in (1, 5, 257):
        h = _check_product(scipy.sparse.csr_matrix((n, n)), n)
        assert h[0] == 0.0 and h[1] == 0.0


# ---- coefficients, norm, scaling ------------------------------------------------------
@pytest.mark.parametrize("stochastic", [False, True], ids=["general", "stochastic"])
@pytest.mark.parametrize("n", SIZES)
def test_step_coefficients_norm_and_scaling(n, stochastic):
    """step(j) over bases of 1, 2, 17 and m_max orthonormal vectors, on a vector of
    its own (apply=False: w is what was uploaded, bit for bit) and on A V[j]:
    h[:j+1] against V^T w twice over, h[j+1] against the norm of what is left, and
    ||V[j+1]|| = 1 within (ceil(n/256) + 10) u (the sum's (ceil(n/256) + 8) u / 2 under
    the root, the root, the reciprocal, the product).  kr_dots_kernel, kr_axpy_kernel,
    kr_scale_kernel; n not a multiple of 256, more than 64 blocks at 70001."""
    A = _matrix(n, stochastic)
    m_max = min(n, 24)
    space = _device(A, m_max)
    try:
        for b in sorted({1, 2, 17, m_max}):
            if b > min(n, m_max):
                continue
            V = _orthonormal(b, n, 100 * n + b)
            for apply in (False, True):
                _upload(space, V)
                if apply:
                    w, s, k = _ld_product(A, V[b - 1])
                    w_err = _product_bound(s, k)
                else:
                    x = np.random.RandomState(b).standard_normal(n) * 3.0
                    space.set_vector(b, x)
                    w, w_err = x.astype(LD), np.zeros(n, dtype=LD)
                h = space.step(b - 1, apply)
                assert np.array_equal(_download(space, 0, b), V)   # the basis is read only
                ref, hb, nrm, nb = _ld_step(V, w, w_err)
                tag = "n = %d, %d vectors, apply=%s" % (n, b, apply)
                # (+ u |h|: the two passes' coefficients are added in float64)
                _assert_within(h[:b], ref, hb + U * np.abs(ref), "h " + tag)
                _assert_within(h[b:], nrm, nb, "norm " + tag)
                if h[b] > 0:
                    one = _ld_norm(space.get_vector(b))
                    _assert_within(one, LD(1), 2 * (np.ceil(n / 256.0) + 10) * U,
                                   "||V[j+1]|| " + tag)
    finally:
        space.close()


# ---- rotation --------------------------------------------------------------------------
def _rotation_bound(V, Q):
    """kr_rotate_kernel: m FMAs per element: m u sum_r |V_re Q_rc|"""
    return 2 * V.shape[0] * U * (np.abs(Q.T).astype(LD) @ np.abs(V).astype(LD))


@pytest.mark.parametrize("n", SIZES)
def test_rotate_and_combine(n):
    """rotate / combine against Q^T V in long double with a general (non-symmetric,
    non-square) Q, so that the major order of Q matters: kk = 1, kk = m, m = m_max + 1,
    combine over more columns than one call takes (DeviceKrylov.combine's chunks); what
    each must leave alone stays bit-identical; the slot move_last has no vector for is
    refused."""
    m_max = 12
    rng = np.random.RandomState(n)
    space = _device(scipy.sparse.csr_matrix((n, n)), m_max)
    try:
        V = rng.standard_normal((m_max + 1, n)) * 10.0 ** rng.uniform(-2, 2, size=(m_max + 1, 1))
        _upload(space, V)
        # combine: 2 (m_max + 1) + 3 columns, over the whole basis and over part of it
        for m in (m_max + 1, 5):
            Q = rng.standard_normal((m, 2 * (m_max + 1) + 3))
            out = space.combine(m, Q)
            assert out.shape == (Q.shape[1], n)
            _assert_within(out, Q.T.astype(LD) @ V[:m].astype(LD), _rotation_bound(V[:m], Q),
                           "combine m = %d, n = %d" % (m, n))
            assert np.array_equal(_download(space, 0, m_max + 1), V)
        # rotate, move_last=False: (m, kk) = (m_max + 1, 1), (m_max + 1, m_max + 1), (7, 3)
        for m, kk in ((m_max + 1, 1), (m_max + 1, m_max + 1), (7, 3)):
            _upload(space, V)
            Q = rng.standard_normal((m, kk))
            space.rotate(m, Q, False)
            got = _download(space, 0, m_max + 1)
            _assert_within(got[:kk], Q.T.astype(LD) @ V[:m].astype(LD), _rotation_bound(V[:m], Q),
                           "rotate m = %d, kk = %d, n = %d" % (m, kk, n))
            assert np.array_equal(got[kk:], V[kk:])
        # move_last=True: the old V[m] lands in V[kk] bit for bit
        for m, kk in ((m_max, 1), (m_max, m_max), (6, 4)):
            _upload(space, V)
            Q = rng.standard_normal((m, kk))
            space.rotate(m, Q, True)
            got = _download(space, 0, m_max + 1)
            _assert_within(got[:kk], Q.T.astype(LD) @ V[:m].astype(LD), _rotation_bound(V[:m], Q),
                           "rotate + move m = %d, kk = %d, n = %d" % (m, kk, n))
            assert np.array_equal(got[kk], V[m])
            assert np.array_equal(got[kk + 1:], V[kk + 1:])
        # there is no V[m_max + 1] to move
        _upload(space, V)
        with pytest.raises(_lib.HipError, match="error -1"):
            space.rotate(m_max + 1, rng.standard_normal((m_max + 1, 2)), True)
        assert np.array_equal(_download(space, 0, m_max + 1), V)
    finally:
        space.close()


# ---- the Chebyshev operator ---------------------------------------------------------------
CHEB_INTERVAL = (-1.0, 0.9)         # a + b != 0: the centre c = -0.05 matters


def _relation_error(A, V, H, j, flt):
    """max over the elements of | op(V[j]) - sum_i H[i, j] V[i] |, op in long double
    from V[j] as downloaded"""
    Vl = V[:j + 2].astype(LD)
    recon = H[:j + 2, j].astype(LD) @ Vl
    ref = _ld_cheb(A, V[j], flt[0], flt[1], flt[2]) if flt else _ld_product(A, V[j])[0]
    return float(np.abs(recon - ref).max())


def _standin_error(A, x, flt, ref=None):
    """the float64 numpy stand-in's operator on the same vector against the same
    long-double reference"""
    twin = NumpyKrylov(A, 1)
    twin.set_filter(*flt)
    ref = _ld_cheb(A, x, *flt) if ref is None else ref
    return float(np.abs(twin._apply(x).astype(LD) - ref).max())


def _operator(A, x, flt):
    """-> (op(x) in long double, elementwise bound of the device's own op(x)): the
    product's bound, or 8 times the stand-in's error for the polynomial"""
    if flt:
        w = _ld_cheb(A, x, *flt)
        return w, np.full(len(x), 8 * _standin_error(A, x, flt, w), dtype=LD)
    w, s, k = _ld_product(A, x)
    return w, _product_bound(s, k)


def _check_column(A, V, H, j, flt, what):
    """column j of expand, whole: the Arnoldi relation (plain: _plain_relation_bound;
    filtered: 8 times the stand-in's error), h[:j+1] and h[j+1] against _ld_step from
    V[0..j] as downloaded, ||V[j+1]|| = 1 within (ceil(n/256) + 10) u.
    -> (op(V[j]), its bound), for the caller's further checks"""
    n = V.shape[1]
    w, w_err = _operator(A, V[j], flt)
    recon = H[:j + 2, j].astype(LD) @ V[:j + 2].astype(LD)
    if flt:
        dev = float(np.abs(recon - w).max())
        print("%s column %d: relation device %.3g, stand-in %.3g"
              % (what, j, dev, float(w_err[0]) / 8))
        assert dev <= float(w_err[0]), (what, j)
    else:
        _assert_within(recon, w, _plain_relation_bound(A, V, H, j),
                       "%s column %d" % (what, j))
    ref, hb, nrm, nb = _ld_step(V[:j + 1], w, w_err)
    _assert_within(H[:j + 1, j], ref, hb + U * np.abs(ref), "%s h of column %d" % (what, j))
    _assert_within(H[j + 1:j + 2, j], nrm, nb, "%s norm of column %d" % (what, j))
    if H[j + 1, j] > 0:
        _assert_within(_ld_norm(V[j + 1]), LD(1), 2 * (np.ceil(n / 256.0) + 10) * U,
                       "%s ||V[%d]||" % (what, j + 1))
    return w, w_err


@pytest.mark.parametrize("d", [2, 3, 4, 7, 48])
@pytest.mark.parametrize("stochastic", [False, True], ids=["general", "stochastic"])
def test_chebyshev_operator(d, stochastic):
    """set_filter(d, a, b): column j of step and of expand satisfies
    T_d((A - c) / e) V[j] = sum_i H[i, j] V[i], the left side by the long-double
    recurrence from the downloaded V[j].  The recurrence's forward error grows with d
    and has no closed bound: the bound is 8 times the error of the float64 stand-in
    (NumpyKrylov._apply) against the same reference on the same vector, for the
    different order inside the row sums.  d = 2 reads V[j] as y_0, higher degrees the
    ping-pong vector; expand's columns past the first normalise on the way
    (kr_spmv_cheb_kernel with `part`).  n = 1023: the last workgroup of rows is
    partial, rows of 0 .. 1023 entries.

    Measured on the MI355X, largest error over the columns and steps of a case,
    device / stand-in (largest ratio of the two on one vector):
        d     general                     stochastic
        2     5.6e-17 / 1.4e-17 (4.1)     5.5e-17 / 7.1e-17 (1.0)
        3     1.5e-17 / 3.7e-17 (0.4)     1.3e-16 / 9.9e-17 (1.5)
        4     5.6e-17 / 2.6e-17 (2.3)     2.9e-16 / 2.5e-16 (3.9)
        7     1.9e-17 / 4.1e-17 (0.7)     1.4e-15 / 1.3e-15 (1.7)
        48    1.8e-16 / 1.6e-16 (1.6)     6.8e-06 / 4.5e-06 (2.4)
    (at d = 48 the stochastic matrix's values are 1e9).  Before the kernel divided by
    e -- it multiplied by a rounded 1 / e, the same relative error at every step --
    the device was at 11.9 times the stand-in at d = 48, stochastic
    (1.66e-5 against 1.40e-6, column 1) and this test failed."""
    n = 1023
    A = _contraction(n, stochastic)
    flt = (d,) + CHEB_INTERVAL
    m = 4
    space = _device(A, m)
    try:
        x = _unit(n, 5)
        space.set_vector(0, x)
        plain = space.step(0)
        plain_v1 = space.get_vector(1)
        space.set_filter(*flt)
        H = space.expand(0, m)
        V = _download(space, 0, m + 1)
        for j in range(m):
            dev = _relation_error(A, V, H, j, flt)
            ref = _standin_error(A, V[j], flt)
            print("T_%d expand column %d (%s): device %.3g, stand-in %.3g"
                  % (d, j, "stochastic" if stochastic else "general", dev, ref))
            assert dev <= 8 * ref
        for j in (0, m - 1):
            _upload(space, V)
            h = space.step(j)
            Hs = np.zeros((m + 1, m))
            Hs[:j + 2, j] = h
            Vs = _download(space, 0, j + 2)
            assert np.array_equal(Vs[:j + 1], V[:j + 1])
            dev = _relation_error(A, Vs, Hs, j, flt)
            ref = _standin_error(A, V[j], flt)
            print("T_%d step %d: device %.3g, stand-in %.3g" % (d, j, dev, ref))
            assert dev <= 8 * ref
        # the degree is sticky state: degree 0 gives the plain product back
        space.set_filter(0)
        again = space.step(0)
        assert np.array_equal(again, plain)
        assert np.array_equal(space.get_vector(1), plain_v1)
    finally:
        space.close()


def test_filter_arguments():
    space = _device(_matrix(5, True), 2)
    try:
        for args in ((1, -1.0, 0.9), (4097, -1.0, 0.9), (-1, -1.0, 0.9), (4, 0.5, 0.5),
                     (4, 0.9, -1.0), (4, 0.0, float("nan"))):
            with pytest.raises(_lib.HipError, match="error -1"):
                space.set_filter(*args)
        space.set_filter(4096, -1.0, 0.9)
        space.set_filter(0)
    finally:
        space.close()


# ---- expand as a whole ---------------------------------------------------------------------
def _plain_relation_bound(A, V, H, j):
    """column j of the plain iteration, per element: the product's bound and
    (j + 4) u sum_i |H_ij V_ie| for taking the column apart again (j + 1 FMAs per
    pass, counted once with the one rounding each of h = h' + h'', 1 / norm, the
    scaling; at j = 0 the 4 u of _check_product)"""
    _, s, k = _ld_product(A, V[j])
    r = np.abs(H[:j + 2, j]).astype(LD) @ np.abs(V[:j + 2]).astype(LD)
    return 2 * (_product_bound(s, k) + (j + 4) * U * r)


def _orthogonality_loss(V):
    Vl = V.astype(LD)
    return float(np.abs(Vl @ Vl.T - np.eye(len(V), dtype=LD)).max())


@pytest.mark.parametrize("flt", [None, (7,) + CHEB_INTERVAL], ids=["plain", "filtered"])
@pytest.mark.parametrize("m", [1, 2, 40, 60])
def test_expand(m, flt):
    """expand(0, m) for m = 1, 2, 40 and m_max = 60 on a 5000-state stochastic matrix:
    every column satisfies the Arnoldi relation (plain: the product's bound plus the
    reconstruction's; filtered: 8 times the stand-in's error, as in
    test_chebyshev_operator), H is exactly zero below the sub-diagonal, and the loss of
    orthogonality max |V^T V - I| over the m + 1 vectors is within 16 times the loss of
    the float64 stand-in on the same matrix and start vector (floor (m + 1) u): it has
    no closed bound either.

    Measured loss on the MI355X, device / stand-in:
        m     plain                  filtered
        1     2.3e-16 / 1.5e-16      8.0e-17 / 8.0e-17
        2     2.3e-16 / 2.1e-16      8.0e-17 / 5.4e-16
        40    2.5e-16 / 4.9e-16      2.5e-16 / 5.4e-16
        60    3.3e-16 / 7.7e-16      2.5e-16 / 5.4e-16
    With the rounded 1 / e, column 39 of the filtered run missed its relation bound
    (9.1e-15 against 8 x 1.1e-15)."""
    n = 5000
    A = _matrix(n, True)
    x = _unit(n, 3)
    space = _device(A, 60)
    try:
        space.set_vector(0, x)
        if flt:
            space.set_filter(*flt)
        H = space.expand(0, m)
        V = _download(space, 0, m + 1)
    finally:
        space.close()
    assert H.shape == (m + 1, m) and np.all(np.isfinite(H))
    assert np.all(np.tril(H, -2) == 0.0)
    assert np.all(np.diag(H, -1) > 0)
    for j in range(m):
        if flt:
            dev = _relation_error(A, V, H, j, flt)
            ref = _standin_error(A, V[j], flt)
            assert dev <= 8 * ref, (j, dev, ref)
        else:
            recon = H[:j + 2, j].astype(LD) @ V[:j + 2].astype(LD)
            _assert_within(recon, _ld_product(A, V[j])[0], _plain_relation_bound(A, V, H, j),
                           "expand column %d of %d" % (j, m))
    twin = NumpyKrylovExpand(A, 60)
    twin.set_vector(0, x)
    if flt:
        twin.set_filter(*flt)
    twin.expand(0, m)
    loss, loss_twin = _orthogonality_loss(V), _orthogonality_loss(twin.V[:m + 1])
    print("expand m = %d %s: loss of orthogonality device %.3g, stand-in %.3g"
          % (m, "filtered" if flt else "plain", loss, loss_twin))
    assert loss <= max(16 * loss_twin, (m + 1) * U)


@pytest.mark.parametrize("flt", [None, (7,) + CHEB_INTERVAL], ids=["plain", "filtered"])
def test_restart_shape(flt):
    """What every large solve does: expand(0, m), rotate(m, Z[:, :p], move_last=True)
    with the orthogonal Z of a Schur form, expand(p, m).  The second expand leaves
    V[0..p] bit-identical, returns exact zeros in the columns below p, its columns
    p .. m-1 satisfy the relation, and each agrees with step(j) from the same state
    (V[0..j] as expand left them) within the sum of the two's own bounds: the
    coefficients' and the norm's of _ld_step, once for each, plain and filtered.  (Not
    bitwise: expand sums the norm per block and then over the blocks, step in one
    strided pass.)"""
    n, m, p = 5000, 30, 11
    A = _matrix(n, True)
    space = _device(A, m)
    try:
        space.set_vector(0, _unit(n, 4))
        if flt:
            space.set_filter(*flt)
        H0 = space.expand(0, m)
        S, Z = scipy.linalg.schur(H0[:m, :m], output="real")
        while S[p, p - 1] != 0.0:       # not through a 2 x 2 block
            p += 1
        space.rotate(m, Z[:, :p], True)
        before = _download(space, 0, p + 1)
        H = space.expand(p, m)
        V = _download(space, 0, m + 1)
        assert np.array_equal(V[:p + 1], before)
        assert np.all(H[:, :p] == 0.0) and np.all(np.tril(H, -2) == 0.0)
        assert np.all(np.isfinite(H))
        ops = {j: _check_column(A, V, H, j, flt, "restart") for j in range(p, m)}
        # step(j) from the state expand(p, m) left: V[0..j] are read only
        for j in range(p, m):
            h = space.step(j)
            _, hb, _, nb = _ld_step(V[:j + 1], *ops[j])
            _assert_within(h[:j + 1], H[:j + 1, j].astype(LD), 2 * hb + 2 * U * np.abs(h[:j + 1]),
                           "step against expand, column %d" % j)
            _assert_within(h[j + 1:], H[j + 1:j + 2, j].astype(LD), 2 * nb,
                           "step against expand, norm %d" % j)
            space.set_vector(j + 1, V[j + 1])
    finally:
        space.close()


@pytest.mark.parametrize("flt", [None, (4,) + CHEB_INTERVAL], ids=["plain", "filtered"])
def test_expand_over_more_than_64_partial_sums(flt):
    """expand(j0, m) with j0 = 2, m = 5 at n = 70001: kr_axpy_hsum_kernel leaves 274
    per-block sums of ||w||^2, so kr_total's lane loop makes five trips (the last one
    partial: 274 = 4 * 64 + 18) in each of its readers -- kr_spmv_norm_kernel (plain,
    columns 3 and 4), kr_spmv_cheb_kernel with `part` (filtered) and kr_finish_kernel
    (V[5]).  Every other expand in the suite has at most 20 partial sums, one trip.
    Per column: the relation, the coefficients, h[j+1] against the long-double norm of
    the orthogonalised vector, ||V[j+1]|| = 1 (_check_column); V[0..2] bit-identical,
    the columns below j0 exact zeros.  Plain on the mixed-sign matrix, filtered on the
    stochastic one scaled into the unit disc.

    Measured on the MI355X: plain, relation within 0.2 of its bound, norms within
    3e-4 of theirs; filtered, relation 4.6e-17 .. 2.5e-16 against the stand-in's
    3.8e-17 .. 1.5e-16.  A kr_total that adds only its first trip fails both cases."""
    n, j0, m = 70001, 2, 5
    assert int(np.ceil(n / 256.0)) == 274
    A = _contraction(n, True) if flt else _matrix(n, False)
    V0 = _orthonormal(j0 + 1, n, 70)
    space = _device(A, m)
    try:
        _upload(space, V0)
        if flt:
            space.set_filter(*flt)
        H = space.expand(j0, m)
        V = _download(space, 0, m + 1)
    finally:
        space.close()
    assert np.array_equal(V[:j0 + 1], V0)
    assert np.all(np.isfinite(H)) and np.all(H[:, :j0] == 0.0)
    assert np.all(np.tril(H, -2) == 0.0) and np.all(np.diag(H, -1)[j0:] > 0)
    for j in range(j0, m):
        _check_column(A, V, H, j, flt, "n = 70001 %s" % ("filtered" if flt else "plain"))


# ---- zero norm ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flt", [None, (3,) + CHEB_INTERVAL], ids=["plain", "filtered"])
@pytest.mark.parametrize("n", [5, 257, 1023])
def test_zero_norm(n, flt):
    """The strict upper shift matrix (A[i, i+1] = 1) sends e_0 to an exact zero vector.
    step: h[1] == 0.0 and V[1] stays what it was, bit for bit; expand: finite values
    only, zero vectors from there on, no NaN in the basis (the guards of
    kr_spmv_norm_kernel, kr_spmv_cheb_kernel and kr_finish_kernel).  With the filter
    A - c is not nilpotent; there the zero norm comes from a zero start vector."""
    A = scipy.sparse.diags(np.ones(n - 1), 1, format="csr")
    m = 4
    space = _device(A, m)
    try:
        e0 = np.zeros(n)
        e0[0] = 1.0
        marker = np.arange(n, dtype=np.float64) + 0.25
        for j in range(1, m + 1):
            space.set_vector(j, marker)
        space.set_vector(0, np.zeros(n) if flt else e0)
        if flt:
            space.set_filter(*flt)
        h = space.step(0)
        assert h[0] == 0.0 and h[1] == 0.0
        assert np.array_equal(space.get_vector(1), marker)
        H = space.expand(0, m)
        V = _download(space, 0, m + 1)
        assert np.all(np.isfinite(H)) and np.all(H == 0.0)
        assert np.all(np.isfinite(V)) and np.all(V[1:] == 0.0)
        # a norm that becomes zero in the middle of expand: e_2 -> e_1 -> e_0 -> 0
        if not flt:
            e2 = np.zeros(n)
            e2[2] = 1.0
            space.set_vector(0, e2)
            H = space.expand(0, m)
            V = _download(space, 0, m + 1)
            assert np.all(np.isfinite(H)) and np.all(np.isfinite(V))
            want = np.zeros((m + 1, m))
            want[1, 0] = want[2, 1] = 1.0
            assert np.array_equal(H, want)
            assert V[1][1] == 1.0 and V[2][0] == 1.0 and np.all(V[3:] == 0.0)
    finally:
        space.close()


# ---- lifetime ------------------------------------------------------------------------------------
def _run_once(n, m_max, space=None):
    A = _matrix(n, True)
    own = space is None
    space = space or _device(A, m_max)
    try:
        space.set_vector(0, _unit(n, 9))
        H = space.expand(0, m_max)
        return H, _download(space, 0, m_max + 1)
    finally:
        if own:
            space.close()


def test_create_destroy_create():
    """three spaces of different n and m_max created, used and closed one after the
    other while a fourth stays open and is used in between: each gives what a fresh
    run of it gives, bit for bit (every reduction has a fixed order)"""
    shapes = [(257, 7), (5000, 30), (64, 3)]
    fresh = [_run_once(n, m) for n, m in shapes]
    fresh4 = _run_once(1000, 12)
    fourth = _device(_matrix(1000, True), 12)
    try:
        for (n, m), want in zip(shapes, fresh):
            got = _run_once(n, m)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            again = _run_once(1000, 12, fourth)
            assert np.array_equal(again[0], fresh4[0]) and np.array_equal(again[1], fresh4[1])
    finally:
        fourth.close()
    fourth.close()      # (closing twice is harmless)


# ---- the solver on the device -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 257, 999, 1000, 1001, 1500])
def test_eigenspectrum_sizes(n):
    """all eigenvalues through the full-basis branch up to its limit of 1000 states,
    the top 8 through the restarted iteration just above it; against LAPACK at the
    project's 1e-9, the stationary vector to 1e-9 with unit sum to 1e-12"""
    _check_solver_case(n, tm.DeviceKrylov)


@pytest.mark.parametrize("kind", ["four_cycles", "rank_one", "kron"])
def test_eigenspectrum_real_breakdowns(kind):
    """matrices whose Krylov space closes exactly: expand's tiny sub-diagonal entry,
    the tail redone with step, a fresh direction through step(apply=False), counted"""
    _check_solver_case(kind, tm.DeviceKrylov)


@pytest.mark.parametrize("n", [257, 1500])
def test_eigenspectrum_right_vectors_of_a_dense_array(n):
    """left=False and an ndarray: T x = lambda x"""
    T = _rowstoch(n, min(1, 6 / n), n).toarray()
    vals, vecs = tm.eigenspectrum(T, n_eigs=None if n <= 1000 else 8, left=False)
    w = np.linalg.eigvals(T)
    w = w[np.argsort(-w.real, kind="stable")][:len(vals)]
    np.testing.assert_allclose(vals, w.real, rtol=0, atol=1e-9)
    checked = 0
    for i in range(len(vals)):
        if abs(w[i].imag) > 1e-12:
            continue        # (the real part of a complex pair's vector: phase is arbitrary)
        x = vecs[:, i]
        assert np.linalg.norm(T @ x - vals[i] * x) <= 1e-9 * np.linalg.norm(x)
        checked += 1
    assert checked >= 1
