"""enspara_amd.tpt on the device: committors, mean first passage times and fluxes
(csrc/ek_tpt.hip) on the LU of csrc/ek_lu.hip.

No expected value comes from a device call.  Values are held to two
criteria, both relative to the reference's own error:
  backward  eta = ||B - A X||inf / (||A||inf ||X||inf + ||B||inf), residual in long
            double, eta_dev <= 8 max(eta_ref, u), eta_ref that of numpy.linalg.solve
            on the same system, u = 2^-53
  forward   max|x_dev - x_hp| <= 32 max(err_ref, u max|x_hp|) with the high-precision
            x_hp and the real reference's error err_ref of tests/golden/tpt_golden.npz
Shapes: the reference's 3- and 4-state tables; n = 17 (one MFMA tile and a bit); 63,
64, 65 around the panel width; 130 (two panels and a ragged third, once with
cross = 1e-5: ill-conditioned); 300.  tests/test_gpu_lu_large.py goes on where the
kernels of the LU change form, at the constants LU_PANEL_WG = 1024, LU_SUB_RPT = 4 and
LU_COL_WG = 256 (enspara_amd/tpt/core.py): n = 1100 (rows in a thread's second register
slot), 4200 (all four slots and rows left in memory), and 257 / 300 right-hand sides at
n = 300 (two workgroups of them).  Every test prints the ratios it measures."""
import os

import numpy as np
import pytest
import scipy.sparse

import _numpy_tpt as nt
from enspara_amd import tpt
from enspara_amd.exception import DataInvalid
from enspara_amd.tpt.core import LU_COL_WG, LU_PANEL, LU_PANEL_WG, LU_SUB_RPT, _solve

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "tpt_golden.npz")
G = np.load(GOLDEN)
RESULTS = sorted(k[3:] for k in G.files if k.startswith("hp_"))
CHAINS = [str(c) for c in G["chains"]]

T3 = np.array([[0.5, 0.4, 0.1], [0.25, 0.5, 0.25], [0.1, 0.5, 0.4]])
T4 = np.array([[0.5, 0.4, 0.1, 0.], [0.25, 0.5, 0.2, 0.05], [0.1, 0.15, 0.5, 0.25],
               [0., 0.1, 0.4, 0.5]])
TFLUX = np.array([[0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
TCOUNTS = np.array([[2, 1, 1], [2, 1, 2], [3, 2, 1]])
MFPT_ALL = np.array([[0., 3.71428571, 3.5], [2.3125, 0., 3.], [2.125, 3.42857143, 0.]])
ARR_TYPES = [np.array, scipy.sparse.csr_matrix, scipy.sparse.coo_matrix,
             scipy.sparse.lil_matrix]
# exact elimination with ties in three pivot columns and the pivots (3, 3, 4, 3, 4):
# every intermediate is a dyadic rational of a few bits
TIES5 = np.array([[0, -4, 4, -4, -2], [1, 3, -4, 2, 4], [-1, 0, 1, -3, -4],
                  [-2, -2, 1, -1, 0], [-2, 2, 3, -3, 4]], dtype=np.float64)


def test_panel_width_is_the_one_the_shapes_assume():
    assert LU_PANEL == 64 and [G["C_" + c].shape[0] for c in CHAINS] == [
        17, LU_PANEL - 1, LU_PANEL, LU_PANEL + 1, 130, 130, 300]


def test_large_sizes_straddle_the_constants_of_the_kernels():
    """tests/test_gpu_lu_large.py: if this fails the kernels were retuned, and the
    sizes (and the tables of rows there) move with the constants named here"""
    def pad(n):
        return -(-n // LU_PANEL) * LU_PANEL
    n1, n4, tail = nt.LU_N_SLOTS, nt.LU_N_TAIL, LU_PANEL_WG * LU_SUB_RPT
    # rows in slot 1 and in no other; n still affordable for nt.lu_solve
    assert LU_PANEL_WG + LU_PANEL < n1 and pad(n1) <= 2 * LU_PANEL_WG and n1 <= 1200
    # real rows in the tail for more than a panel of columns, one per thread at most
    assert tail + LU_PANEL < n4 and pad(n4) <= tail + LU_PANEL_WG
    # the golden n300: a second, ragged block of right-hand sides
    assert LU_COL_WG < 257 < 300 and pad(300) <= 2 * LU_COL_WG


def _chain(chain):
    C = G["C_" + chain]
    return nt.tprob_from_counts(C), nt.pops_from_counts(C)


def _device(chain, what, **kw):
    T, pops = _chain(chain)
    r = "%s_%s" % (chain, what)
    if what[0] == "q":
        return tpt.committors(T, G["src_" + r], G["snk_" + r])
    if what in ("t1", "t3"):
        return tpt.mfpts(T, sinks=G["snk_" + r], **kw)
    if what == "tall":
        return tpt.mfpts(T, populations=pops, **kw)
    rq = chain + "_qA"
    fn = tpt.reactive_fluxes if what == "fA" else tpt.net_fluxes
    return fn(T, G["src_" + rq], G["snk_" + rq], populations=pops)


# ---- the reference's tables -----------------------------------------------------------------
@pytest.mark.parametrize("arr_type", ARR_TYPES)
def test_committors_tables(arr_type):
    for src, snk in ((0, 2), ([0], [2])):
        q = tpt.committors(arr_type(T3), src, snk)
        assert q.dtype == np.float64 and q.shape == (3,)
        assert np.array_equal(np.around(q, 5), [0, 0.5, 1.])
        assert q[0] == 0 and q[2] == 1 and abs(q[1] - 0.5) <= 4 * nt.U
    q = tpt.committors(arr_type(T4), 0, 3)
    assert np.array_equal(np.around(q, 5), [0, 0.34091, 0.60227, 1.])
    q = tpt.committors(arr_type(T4), [0, 2], [3])
    assert q[0] == 0 and q[2] == 0 and q[3] == 1 and abs(q[1] - 0.1) <= 4 * nt.U


@pytest.mark.parametrize("arr_type", ARR_TYPES)
def test_mfpts_tables(arr_type):
    T = arr_type(TCOUNTS / TCOUNTS.sum(axis=1)[:, None])
    # (populations=None: enspara_amd.msm.eq_probs on the device)
    m = tpt.mfpts(T)
    assert m.dtype == np.float64 and m.shape == (3, 3)
    np.testing.assert_array_almost_equal(m, MFPT_ALL, 5)
    np.testing.assert_array_almost_equal(tpt.mfpts(T, sinks=[0]), [0., 2.3125, 2.125], 5)
    np.testing.assert_array_almost_equal(tpt.mfpts(T, sinks=0), [0., 2.3125, 2.125], 5)
    t = tpt.mfpts(T, sinks=[0, 1])
    np.testing.assert_array_almost_equal(t, [0., 0., 1.2], 5)
    assert np.array_equal(tpt.mfpts(T, sinks=[0, 1], lagtime=4.0), 4.0 * t)


@pytest.mark.parametrize("arr_type", ARR_TYPES)
def test_fluxes_tables(arr_type):
    pops = np.zeros(3) + 1 / 3.
    true = np.zeros((3, 3))
    true[0, 1] = true[1, 2] = np.around(1 / 12., 5)
    for kw in ({"populations": pops}, {}):
        f = tpt.reactive_fluxes(arr_type(TFLUX), 0, 2, **kw)
        nf = tpt.net_fluxes(arr_type(TFLUX), [0], [2], **kw)
        if arr_type is np.array:
            assert isinstance(f, np.ndarray) and isinstance(nf, np.ndarray)
        else:
            assert isinstance(f, scipy.sparse.lil_matrix)
            assert isinstance(nf, scipy.sparse.lil_matrix)
            f, nf = f.toarray(), nf.toarray()
        assert f.dtype == np.float64
        assert np.array_equal(np.around(f, 5), true)
        assert np.array_equal(np.around(nf, 5), true)
    rp = tpt.reactive_populations(arr_type(TFLUX), 0, 2, populations=pops)
    assert rp.dtype == np.float64
    np.testing.assert_allclose(rp, [0, 1, 0], atol=4 * nt.U)


# ---- the goldens: forward error -----------------------------------------------------------------
@pytest.mark.parametrize("r", RESULTS)
def test_forward_error_against_the_high_precision_result(r):
    chain, what = r.split("_")
    n = G["C_" + chain].shape[0]
    x = _device(chain, what)
    hp, err = G["hp_" + r], float(G["err_" + r])
    assert x.dtype == np.float64 and x.shape == hp.shape
    got = np.abs(x - hp).max()
    bound = nt.forward_bound(err, hp)
    print("%-12s device %.3e  reference %.3e  device / max(err_ref, u max|x|) = %.3f (<= 32)"
          % (r, got, err, 32 * got / bound))
    assert got <= bound
    if what[0] == "q":
        assert np.all(x[G["src_" + r]] == 0) and np.all(x[G["snk_" + r]] == 1)
        assert x.min() >= 0 and x.max() <= 1
    if what in ("t1", "t3"):
        assert np.all(x[G["snk_" + r]] == 0)
        assert np.array_equal(_device(chain, what, lagtime=0.25), 0.25 * x)
    if what == "tall":
        assert np.all(np.diag(x) == 0)
        if n <= 65:
            assert np.array_equal(_device(chain, what, lagtime=8.0), 8.0 * x)
    if what in ("fA", "nA"):
        assert np.all(np.diag(x) == 0) and x.min() >= 0
    if what == "nA":
        assert np.all((x == 0) | (x.T == 0))


@pytest.mark.parametrize("chain", ["n17", "n130"])
def test_reactive_populations(chain):
    T, pops = _chain(chain)
    r = chain + "_qA"
    rp = tpt.reactive_populations(T, G["src_" + r], G["snk_" + r], populations=pops)
    q = G["hp_" + r].astype(nt.LD)
    d = pops.astype(nt.LD) * q * (1 - q)
    hp = d / d.sum()
    assert rp.dtype == np.float64 and rp.shape == pops.shape
    assert rp[0] == 0 and rp[-1] == 0
    got = float(np.abs(rp - hp).max())
    # d rp_i = (pi_i (1 - 2 q_i) dq_i - rp_i sum_j pi_j (1 - 2 q_j) dq_j) / sum(d), so an
    # error err in q allows err (max pi + max rp) / sum(d) in rp: the reference's own
    # committor error, carried through the reference's own formula
    err = float(G["err_" + r]) * float((pops.max() + hp.max()) / d.sum())
    bound = nt.forward_bound(err, hp)
    print("%s reactive populations: %.3e, bound %.3e" % (chain, got, bound))
    assert got <= bound


# ---- the solver: backward error ------------------------------------------------------------------
_check_backward = nt.check_backward


@pytest.mark.parametrize("chain", CHAINS)
def test_backward_error_on_the_golden_systems(chain):
    T, pops = _chain(chain)
    n = T.shape[0]
    for tag in ("A", "M"):
        r = "%s_q%s" % (chain, tag)
        A, b = nt.committor_system(T, G["src_" + r], G["snk_" + r])
        # (the committors ARE the system's solution: its absorbing rows are identities)
        _check_backward(r, A, b, _device(chain, "q" + tag))
        x = _solve(A, b)
        assert x.dtype == np.float64 and x.shape == (n,)
        _check_backward(r + " _solve", A, b, x)
    for what in ("t1", "t3"):
        A, c = nt.mfpt_sink_system(T, G["snk_%s_%s" % (chain, what)])
        _check_backward("%s_%s" % (chain, what), A, c, _device(chain, what))
    # (the long-double residual of n right-hand sides; n300's all-to-all system, with its
    # two workgroups of right-hand sides, is tests/test_gpu_lu_large.py's)
    if n <= 130:
        A, eye = nt.mfpt_all_system(T, pops)
        Z = _solve(A, eye)
        assert Z.shape == (n, n)
        _check_backward(chain + " all-to-all Z", A, eye, Z)
        B3 = np.stack([np.ones(n), np.arange(n) / n, np.cos(np.arange(n))], axis=1)
        _check_backward(chain + " nrhs 3", A, B3, _solve(A, B3))


@pytest.mark.parametrize("n", [17, 65, 130])
def test_solve_needs_its_pivoting(n):
    rng = np.random.RandomState(n)
    # a tiny leading entry: O(1) wrong without an exchange
    A = rng.rand(n, n) + np.eye(n)
    A[:, 0] = 1.0
    A[0, 0] = 1e-20
    for B in (rng.rand(n), rng.rand(n, 3), rng.rand(n, n)):
        X, piv, info = _solve(A, B, return_pivots=True)
        assert info == -1 and piv[0] == 1 and X.shape == B.shape
        _check_backward("tiny pivot n %d nrhs %d" % (n, B.size // n), A, B, X)
    # a diagonally dominant matrix with its rows permuted: the pivots undo it
    D = rng.rand(n, n) + n * np.eye(n)
    perm = rng.permutation(n)
    A = D[perm]
    B = rng.rand(n, 3)
    X, piv, info = _solve(A, B, return_pivots=True)
    assert info == -1
    rows = np.arange(n)
    for k in range(n):
        rows[[k, piv[k]]] = rows[[piv[k], k]]
    assert np.array_equal(perm[rows], np.arange(n))
    _check_backward("permuted dominant n %d" % n, A, B, X)


@pytest.mark.parametrize("blocks", [4, 13, 26])
def test_solve_breaks_ties_by_the_lowest_row(blocks):
    """5 x 5 integer blocks (5 does not divide the panel width: blocks straddle the
    panels) whose elimination is exact (every intermediate a dyadic rational of a few
    bits), so the pivots are a matter of the rule alone"""
    n = 5 * blocks
    A = np.zeros((n, n))
    for b in range(blocks):
        A[5 * b:5 * b + 5, 5 * b:5 * b + 5] = TIES5 * (1 + b % 3)
    B = np.arange(2 * n, dtype=np.float64).reshape(n, 2) % 7 - 3
    X0, piv0, info0 = nt.lu_solve(A, B)
    assert info0 == -1 and list(piv0[:5]) == [3, 3, 4, 3, 4]
    X, piv, info = _solve(A, B, return_pivots=True)
    assert info == -1
    assert np.array_equal(piv, piv0)
    # (the factors are exact; the back substitution divides by pivots such as 17)
    _check_backward("tied pivots n %d" % n, A, B, X)


@pytest.mark.parametrize("n,k", [(17, 9), (130, 64), (130, 100)])
def test_solve_reports_the_first_zero_pivot(n, k):
    """A = L U in integers with L unit lower triangular, entries in {-1, 0, 1}, and
    |u_jj| = 4 but u_kk = 0: rank n - 1, the elimination exact, every pivot row j
    itself (the first of the tied candidates) and the zero pivot exactly at column k"""
    rng = np.random.RandomState(k)
    L = np.tril(rng.randint(-1, 2, size=(n, n)).astype(np.float64), -1) + np.eye(n)
    Uu = np.triu(rng.randint(-3, 4, size=(n, n)).astype(np.float64), 1)
    Uu += np.diag(4.0 * rng.choice([-1, 1], size=n))
    Uu[k, k] = 0.0
    A = L @ Uu
    # (rank n - 1 by construction: det L = 1 and U has exactly one zero on its diagonal)
    _, piv0, info0 = nt.lu_solve(A, np.ones(n))
    assert info0 == k
    _, piv, info = _solve(A, np.ones(n), return_pivots=True)
    assert info == k
    assert np.array_equal(piv[:k], np.arange(k)) and np.array_equal(piv[:k], piv0[:k])
    with pytest.raises(DataInvalid, match="column %d" % k):
        _solve(A, np.ones(n))


@pytest.mark.parametrize("n", [17, 130])
def test_closed_class_without_an_absorbing_state_is_invalid(n):
    T, pops = _chain("n%d" % n)
    T = T.copy()
    closed = [3, 4, 5]
    T[closed] = 0.0
    T[np.ix_(closed, closed)] = np.array([[0.5, 0.25, 0.25], [0.25, 0.5, 0.25],
                                          [0.25, 0.25, 0.5]])
    with pytest.raises(DataInvalid, match="singular"):
        tpt.committors(T, 0, n - 1)
    with pytest.raises(DataInvalid, match="column"):
        tpt.mfpts(T, sinks=[n - 1])
    with pytest.raises(DataInvalid):
        tpt.net_fluxes(T, 0, n - 1, populations=pops)


def test_two_runs_give_the_same_bits():
    for chain, what in (("n130", "qM"), ("n130", "t3"), ("n65", "tall"), ("n130", "nA"),
                        ("n300", "qA")):
        a, b = _device(chain, what), _device(chain, what)
        assert a.tobytes() == b.tobytes(), (chain, what)
    rng = np.random.RandomState(5)
    A, B = rng.rand(130, 130), rng.rand(130, 130)
    (x1, p1, i1), (x2, p2, i2) = (_solve(A, B, return_pivots=True) for _ in range(2))
    assert x1.tobytes() == x2.tobytes() and np.array_equal(p1, p2) and i1 == i2 == -1
