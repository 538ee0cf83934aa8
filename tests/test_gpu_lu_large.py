"""The LU of csrc/ek_lu.hip where its kernels change form, above the n = 300 of
tests/test_gpu_tpt.py.  Three constants of the kernels decide the shapes
(enspara_amd/tpt/core.py states them): a sub-panel's thread t keeps rows
c0 + t + LU_PANEL_WG i (1024), i < LU_SUB_RPT (4), in registers -- "slots" 0..3 --
and the rows from tail0 = c0 + 4096 on stay in memory -- the "tail"; the back
substitution runs one workgroup per LU_COL_WG (256) right-hand sides.

  n = 1100 (padded to 1152)  slot 1 for sub-panels c0 < 128; the unblocked
                             restatement nt.lu_solve is still affordable here
  n = 4200 (padded to 4224)  slots 1-3 wherever they occur; a tail for c0 < 128
                             (at c0 = 0: rows 4096..4199 real, 4200..4223 padding;
                             from c0 = 104 on padding only); tail0 moves with c0, so
                             a row is memory for one sub-panel and slot 3 for the next
  n = 300, 257 and 300 right-hand sides (padded to 320): two workgroups of right-hand
                             sides, the second ragged; tpt_mfpt_all_kernel on two
                             blocks of columns

No expected value comes from a device call (one exception, said where it is made):
pivots are known by construction or from the restatement, solutions are held to
the backward criterion of tests/test_gpu_tpt.py, eta_dev <= 8 max(eta_ref, u), or
are exact in integers.  Every test prints the ratios it measures."""
import functools
import os

import numpy as np
import pytest

import _numpy_tpt as nt
from enspara_amd import tpt
from enspara_amd.exception import DataInvalid
from enspara_amd.tpt.core import LU_COL_WG, LU_PANEL, LU_PANEL_WG, LU_SUB_RPT, _solve

pytestmark = pytest.mark.gpu

N1, N4 = nt.LU_N_SLOTS, nt.LU_N_TAIL
SUB = 8         # columns of a sub-panel: c0 = SUB * (k // SUB)
TAIL = LU_PANEL_WG * LU_SUB_RPT


def where(k, r):
    """'slot i' or 'tail': where lu_subpanel_kernel keeps row r while it works on
    column k; and the thread that owns it"""
    d = r - SUB * (k // SUB)
    return ("tail" if d >= TAIL else "slot %d" % (d // LU_PANEL_WG)), d % LU_PANEL_WG


# ---- 1. known pivots: rows exchanged in disjoint pairs ---------------------------------
# (k, r, where row r is for column k's sub-panel c0 = 8 (k // 8))
PAIRS_4200 = [
    # c0 = 0, the first sub-panel of panel 0
    (0, 1024, "slot 1"),        # its first row
    (2, 2047, "slot 1"),        # its last row
    (3, 2048, "slot 2"),
    (4, 3072, "slot 3"),
    (5, 4095, "slot 3"),        # the last row in registers
    (6, 4096, "tail"),          # the first row in memory
    (7, 4199, "tail"),          # the last real row
    (1, 4100, "tail"),          # ... slot 3 for c0 = 8: written there by c0 = 0, read here
    # c0 = 8
    (8, 4103, "slot 3"),        # c0 + 4095
    (9, 4110, "tail"),          # ... slot 3 for c0 = 16
    (10, 4104, "tail"),         # c0 + 4096
    # c0 = 24 and 56: an interior and the last sub-panel of panel 0
    (24, 1048, "slot 1"),       # c0 + 1024
    (27, 4120, "tail"),         # c0 + 4096
    (30, 3096, "slot 3"),       # c0 + 3072
    (56, 2103, "slot 1"),       # c0 + 2047
    (60, 4151, "slot 3"),       # c0 + 4095
    (63, 4152, "tail"),         # c0 + 4096
    # panel 1: c0 = 64, and c0 = 120 whose tail (from 4216) is padding only
    (64, 4160, "tail"),         # c0 + 4096
    (66, 4198, "tail"),
    (70, 2112, "slot 2"),       # c0 + 2048
    (121, 4197, "slot 3"),
    (125, 1144, "slot 1"),      # c0 + 1024
    # panels without a tail
    (130, 3200, "slot 3"),      # c0 + 3072
    (200, 2248, "slot 2"),      # c0 + 2048
    (2000, 3024, "slot 1"),     # c0 + 1024
    (3500, 4190, "slot 0"),
]
PAIRS_1100 = [
    (0, 1024, "slot 1"),        # c0 + 1024
    (2, 1099, "slot 1"),        # the last real row
    (3, 1023, "slot 0"),        # the last row of slot 0
    (9, 1032, "slot 1"),        # c0 + 1024
    (24, 1048, "slot 1"),
    (60, 1080, "slot 1"),       # the last sub-panel of panel 0
    (64, 1088, "slot 1"),       # panel 1
    (70, 1090, "slot 1"),
    (121, 1095, "slot 0"),      # slot 1 (from 1144) is padding only
    (130, 600, "slot 0"),       # no slot 1 at all
]


@pytest.mark.parametrize("n,pairs", [(N1, PAIRS_1100), (N4, PAIRS_4200)])
def test_pivots_undo_disjoint_row_exchanges(n, pairs):
    """D = rand + n I with rows exchanged in disjoint pairs (k, r): the pivots are
    pivots[k] = r and the identity elsewhere, exactly, wherever row r is kept"""
    for k, r, regime in pairs:
        assert where(k, r)[0] == regime, (k, r)
    A, want = nt.swapped_dominant(n, [p[:2] for p in pairs], seed=n)
    B = np.random.RandomState(n + 1).rand(n, 3)
    X, piv, info = _solve(A, B, return_pivots=True)
    wrong = np.flatnonzero(piv != want)
    assert info == -1
    assert np.array_equal(piv, want), [(int(k), int(piv[k]), int(want[k])) for k in wrong[:8]]
    nt.check_backward("exchanged pairs n %d" % n, A, B, X)


# ---- 2. ties across slots, waves and the tail ------------------------------------------
# (k, r1, r2, s): column k holds s in row r1 and -s in row r2 and nothing else
TIES_4200 = [
    (0, 1000, 1029, 1),         # slot 0 of thread 1000 before slot 1 of thread 5
    (10, 308, 1332, -1),        # slots 0 and 1 of one thread (c0 = 8, thread 300)
    (17, 2141, 3165, 1),        # slots 2 and 3 of one thread (c0 = 16, thread 77)
    (3, 50, 4146, -1),          # slot 0 and the tail entry of one thread
    (26, 4125, 4195, 1),        # both in the tail (c0 = 24: from 4120), waves 0 and 1
    (33, 4004, 4130, -1),       # slot 3 of thread 900 before the tail of thread 2
    (41, 110, 740, 1),          # slot 0, waves 1 and 10
    (70, 2111, 4161, -1),       # panel 1: slot 1 of thread 1023 before the tail of thread 1
    (130, 2175, 2176, 1),       # no tail: slot 1 of thread 1023 before slot 2 of thread 0
]
TIES_1100 = [
    (0, 1000, 1029, 1),         # slot 0 of thread 1000 before slot 1 of thread 5
    (10, 28, 1052, -1),         # slots 0 and 1 of one thread (c0 = 8, thread 20)
    (41, 110, 740, 1),          # slot 0, waves 1 and 10
    (50, 1071, 1072, -1),       # slot 0 of thread 1023 before slot 1 of thread 0
    (130, 1028, 1088, 1),       # no slot 1: threads 900 and 960 of slot 0
]


@pytest.mark.parametrize("n,triples", [(N1, TIES_1100), (N4, TIES_4200)])
def test_ties_go_to_the_lowest_row_across_slots_waves_and_the_tail(n, triples):
    """A 0 / +-1 matrix whose column k has exactly two candidates, equal in |a|, in
    rows r1 < r2 kept in different places: pivots[k] = r1, not the lower lane's, the
    lower slot's or the register's row; the elimination and the solution are exact"""
    for k, r1, r2, s in triples:
        (w1, t1), (w2, t2) = where(k, r1), where(k, r2)
        assert (w1, t1 // 64) != (w2, t2 // 64), "kept in different places or waves"
    A, want = nt.tie_system(n, triples)
    B = nt.small_integer_rhs(n)
    X, piv, info = _solve(A, B, return_pivots=True)
    wrong = np.flatnonzero(piv != want)
    assert info == -1
    assert np.array_equal(piv, want), [(int(k), int(piv[k]), int(want[k])) for k in wrong[:8]]
    assert np.array_equal(A @ X, B)


# ---- 3. a general matrix held to the restatement's pivots ------------------------------
def test_general_matrix_takes_the_pivots_of_the_restatement():
    """rand - 0.5, n = 1100: no structure helps the search.  The restatement says how
    far every choice is from a tie; where that is far above rounding (asserted on the
    restatement alone) the device has no other row to pick"""
    A = np.random.RandomState(N1).rand(N1, N1) - 0.5
    B = np.random.RandomState(N1 + 1).rand(N1, 3)
    _, piv0, info0, gaps = nt.lu_solve(A, B, return_gaps=True)
    slot1 = int(np.sum(piv0 - SUB * (np.arange(N1) // SUB) >= LU_PANEL_WG))
    print("n %d: smallest relative gap %.2e, %d exchanges, %d pivots from slot 1"
          % (N1, gaps.min(), int(np.sum(piv0 != np.arange(N1))), slot1))
    assert info0 == -1 and gaps.min() >= 1e-9 and slot1 >= 1
    X, piv, info = _solve(A, B, return_pivots=True)
    wrong = np.flatnonzero(piv != piv0)
    assert info == -1
    assert np.array_equal(piv, piv0), [(int(k), int(piv[k]), int(piv0[k])) for k in wrong[:8]]
    nt.check_backward("rand - 0.5 n %d" % N1, A, B, X)


# ---- 4. backward error ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain(n):
    T, pops = nt.weighted_chain(n)
    T.setflags(write=False)
    pops.setflags(write=False)
    return T, pops


def test_unstructured_system_with_pivots_from_the_tail():
    """rand - 0.5, n = 4200.  The pivots of the first two panels depend on their 128
    columns alone, which the restatement eliminates in no time: they come from every
    slot and from the tail, none is near a tie, and the device's must be the same"""
    rng = np.random.RandomState(N4)
    A = rng.rand(N4, N4) - 0.5
    B = rng.rand(N4, 3)
    piv0, info0, gaps = nt.leading_pivots(A, 2 * LU_PANEL)
    d = piv0 - SUB * (np.arange(2 * LU_PANEL) // SUB)
    kept = [int(np.sum((d >= LU_PANEL_WG * i) & (d < LU_PANEL_WG * (i + 1)))) for i in range(4)]
    print("n %d, columns 0..127: smallest relative gap %.2e, pivots from slots %s, from "
          "the tail %d" % (N4, gaps.min(), kept, int(np.sum(d >= TAIL))))
    assert info0 == -1 and gaps.min() >= 1e-9 and min(kept) >= 1 and np.sum(d >= TAIL) >= 1
    X, piv, info = _solve(A, B, return_pivots=True)
    assert info == -1 and X.shape == B.shape
    wrong = np.flatnonzero(piv[:2 * LU_PANEL] != piv0)
    assert not len(wrong), [(int(k), int(piv[k]), int(piv0[k])) for k in wrong[:8]]
    nt.check_backward("rand - 0.5 n %d" % N4, A, B, X)


@pytest.mark.parametrize("n", [N1, N4])
def test_backward_error_of_committors(n):
    T, _ = chain(n)
    A, b = nt.committor_system(T, [0], [n - 1])
    q = tpt.committors(T, [0], [n - 1])
    assert q.dtype == np.float64 and q.shape == (n,)
    assert q[0] == 0 and q[n - 1] == 1 and q.min() >= 0 and q.max() <= 1
    # (the committors ARE the system's solution: its absorbing rows are identities)
    nt.check_backward("committors n %d" % n, A, b, q)


@pytest.mark.parametrize("n", [N1, N4])
def test_backward_error_of_mfpts_to_three_sinks(n):
    T, _ = chain(n)
    sinks = [0, n // 2, n - 1]
    A, c = nt.mfpt_sink_system(T, sinks)
    t = tpt.mfpts(T, sinks=sinks)
    assert t.dtype == np.float64 and t.shape == (n,) and np.all(t[sinks] == 0)
    nt.check_backward("mfpts 3 sinks n %d" % n, A, c, t)


# ---- 5. a zero pivot late in the matrix ------------------------------------------------
def test_zero_pivot_is_reported_from_a_late_column():
    """the integer L U of test_solve_reports_the_first_zero_pivot at n = 1100 with
    u_kk = 0 at k = 1030: sub-panel c0 = 1024 of the seventeenth panel, past every
    row of slot 1"""
    n, k = N1, 1030
    rng = np.random.RandomState(k)
    L = np.tril(rng.randint(-1, 2, size=(n, n)).astype(np.float64), -1) + np.eye(n)
    Uu = np.triu(rng.randint(-3, 4, size=(n, n)).astype(np.float64), 1)
    Uu += np.diag(4.0 * rng.choice([-1, 1], size=n))
    Uu[k, k] = 0.0
    A = L @ Uu
    _, piv, info = _solve(A, np.ones(n), return_pivots=True)
    assert info == k
    assert np.array_equal(piv[:k], np.arange(k))
    with pytest.raises(DataInvalid, match="column %d" % k):
        _solve(A, np.ones(n))


# ---- 6. more than 256 right-hand sides; the all-to-all epilogue ------------------------
@pytest.fixture(scope="module")
def n300():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                             "tpt_golden.npz"))
    C = g["C_n300"]
    return nt.tprob_from_counts(C), nt.pops_from_counts(C)


def test_two_blocks_of_right_hand_sides(n300):
    T, pops = n300
    n = T.shape[0]
    assert n == 300 and LU_COL_WG < 257 < n
    A, eye = nt.mfpt_all_system(T, pops)
    Z = _solve(A, eye)
    assert Z.shape == (n, n)
    nt.check_backward("n300 all-to-all Z", A, eye, Z)
    # a ragged second block: one column in it, the same as the first block's first
    B = np.random.RandomState(257).rand(n, 257)
    B[:, 256] = B[:, 0]
    X = _solve(A, B)
    nt.check_backward("n300 nrhs 257", A, B, X)
    assert X[:, 256].tobytes() == X[:, 0].tobytes()
    # The one expectation made from a device value, Z, itself held to the criterion
    # above: the assembled (I - T) + pi has numpy's bits, the solver is deterministic
    # and the epilogue's order of operations is the restatement's
    m = tpt.mfpts(T, populations=pops, lagtime=2.5)
    want = (2.5 * (np.diag(Z)[None, :] - Z)) / pops[None, :]
    assert m.dtype == np.float64 and np.all(np.diag(m) == 0)
    assert np.array_equal(m, want), "%d entries differ" % int(np.sum(m != want))


def test_many_right_hand_sides_at_the_block_edges():
    """Z = A^-1 at n = 1100, five blocks of right-hand sides: the backward error on
    64 of its columns, those at the edges of the blocks among them (the long-double
    residual of all 1100 takes the host 14 s)"""
    n = N1
    T, pops = chain(n)
    A, eye = nt.mfpt_all_system(T, pops)
    Z = _solve(A, eye)
    edges = [0, 255, 256, 257, 511, 512, 1023, 1024, 1099]
    rest = np.setdiff1d(np.arange(n), edges)
    cols = np.sort(np.append(edges, np.random.RandomState(64).choice(
        rest, 64 - len(edges), replace=False)))
    assert len(cols) == 64 and set(edges) <= set(cols.tolist())
    nt.check_backward("n %d inverse, 64 columns" % n, A, eye[:, cols], Z[:, cols])
