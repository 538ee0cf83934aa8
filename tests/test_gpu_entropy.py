"""enspara_amd.info_theory.entropy on the device (csrc/ek_entropy.hip), through the
public functions and so through the C ABI.

No expected KL, JS or Shannon value comes from a device call: they are computed in numpy
by tests/_numpy_entropy.py (held to the real reference by tests/test_entropy_host.py), and
a row of c terms is held to
    |dev - numpy| <= (c + 4) 2^-52 sum_j |t_j| / ln(base)
(_numpy_entropy.kl_bound, derived there; js_bound and shannon_norm_bound likewise).  Rows
that are +inf must be +inf exactly.  Counts are integers and array_equal to numpy's
bincount.  The resident `assignments=` path is held bit for bit to the two-step path.
Every bounded test prints the largest ratio to its bound that it sees.

Shapes.  The row kernels take one lane a row up to 8 columns, eight lanes up to 128, a
wave beyond; a lane's vector load is 2 columns, a group's step 2 G columns (16 resp. 128),
a workgroup is 256 / G rows.  COLS brackets each of these; rows are 1, 3 and one past a
workgroup.  Every second odd-width row starts on an odd element, so heads and tails of the
16-byte path are walked.  The state-count kernels take 64 features and chunks of 8192
frames a workgroup, 4 states in registers."""
import functools
import os

import numpy as np
import pytest

import _numpy_entropy as ne
from enspara_amd import cards, info_theory, ra
from enspara_amd.exception import DataInvalid
from enspara_amd.info_theory import entropy
from enspara_amd.msm import builders, transition_matrices

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "entropy_golden.npz"))

COLS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 255, 256, 257]
SC_CHUNK = 8192


def _rows_for(cols):
    """1, 3 and one past the rows of a workgroup of this width's form"""
    group = 1 if cols <= 8 else 8 if cols <= 128 else 64
    return [1, 3, 256 // group + 1]


@functools.lru_cache(maxsize=None)
def _case(rows, cols):
    """(P, Q): row r plain (r % 5 == 0), zeros in P (1), zeros in P and in Q at the same
    places and further zeros in P (2), all of P zero (3), all of P and Q zero (r % 10 ==
    8), Q zero where P is not: +inf (4)"""
    rng = np.random.RandomState(1000 * rows + cols)
    P, Q = ne.random_rows(rng, rows, cols), ne.random_rows(rng, rows, cols)
    for r in range(rows):
        z = rng.rand(cols) < 0.4
        if r % 5 == 1:
            P[r, z] = 0.0
        elif r % 5 == 2:
            P[r, z] = 0.0
            Q[r, z & (rng.rand(cols) < 0.5)] = 0.0
        elif r % 5 == 3:
            P[r] = 0.0
            if r % 10 == 8:
                Q[r] = 0.0
        elif r % 5 == 4:
            Q[r, cols - 1] = 0.0
    P.setflags(write=False)
    Q.setflags(write=False)
    return P, Q


def _hold(got, want, bound, what, worst):
    got, want, bound = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(bound)
    inf = np.isposinf(want)
    assert np.array_equal(np.isposinf(got), inf), what
    assert not np.isnan(got).any(), what
    fin = ~inf
    diff = np.abs(got[fin] - want[fin])
    ok = diff <= bound[fin]
    ratio = np.max(diff / np.where(bound[fin] > 0, bound[fin], 1.0), initial=0.0)
    worst[0] = max(worst[0], ratio)
    assert ok.all(), "%s: |dev - numpy| %s over the bound %s" % (what, diff[~ok], bound[fin][~ok])


@pytest.mark.parametrize("base", [2, np.e, 10])
def test_kl_rows(base):
    worst = [0.0]
    n_inf = 0
    for cols in COLS:
        for rows in _rows_for(cols):
            P, Q = _case(rows, cols)
            want, S = ne.kl_divergence(P, Q, base)
            got = entropy.kl_divergence(P, Q, base=base)
            assert got.shape == (rows,) and got.dtype == np.float64
            _hold(got, want, ne.kl_bound(cols, S), "kl %d x %d" % (rows, cols), worst)
            n_inf += int(np.isposinf(want).sum())
            if rows > 8:
                assert want[3] == 0 and got[3] == 0 and got[8] == 0      # the all-zero rows
                assert np.isposinf(got[4]) and np.isfinite(got[5])
    assert n_inf > 0
    print("kl base %s: largest |dev - numpy| / bound = %.3f" % (base, worst[0]))


def test_kl_one_dimensional_and_golden():
    worst = [0.0]
    for cols in COLS:
        P, Q = _case(3, cols)
        for r in range(3):
            want, S = ne.kl_divergence(P[r], Q[r])
            got = entropy.kl_divergence(P[r], Q[r])
            assert np.ndim(got) == 0
            _hold(got, want, ne.kl_bound(cols, S), "1-D %d" % cols, worst)
    for tag, base in (("2", 2), ("e", np.e), ("10", 10)):
        got = entropy.kl_divergence(G["kl_P"], G["kl_Q"], base=base)
        np.testing.assert_array_almost_equal(got, G["kl_base_" + tag], 7)
        for r in range(3):
            np.testing.assert_almost_equal(
                entropy.kl_divergence(G["kl_P"][r], G["kl_Q"][r], base=base),
                G["kl_base_" + tag][r], 7)
    # lists, as the reference takes them
    assert entropy.kl_divergence([0.5, 0.5], [0.25, 0.75]) == \
        entropy.kl_divergence(np.array([0.5, 0.5]), np.array([0.25, 0.75]))


@pytest.mark.parametrize("rows, cols", [(257, 3), (33, 65), (5, 129), (1, 1), (3, 130)])
def test_negative_entry_in_the_last_element(rows, cols):
    P, Q = _case(rows, cols)
    for which in (0, 1):
        M = [P.copy(), Q.copy()]
        M[which][rows - 1, cols - 1] = -0.25
        with pytest.raises(DataInvalid, match="negative probability"):
            entropy.kl_divergence(M[0], M[1])
        with pytest.raises(DataInvalid, match="negative probability"):
            entropy.js_divergence(M[0], M[1])
    entropy.kl_divergence(P, Q)         # (the flag does not stick)


def test_kl_js_shannon_same_bits_twice():
    for cols in (3, 65, 129, 257):
        rows = _rows_for(cols)[-1]
        P, Q = _case(rows, cols)
        for f in (lambda: entropy.kl_divergence(P, Q), lambda: entropy.js_divergence(P, Q),
                  lambda: entropy.shannon_entropy_rows(P + Q)):
            assert f().tobytes() == f().tobytes()


def test_js_rows():
    worst = [0.0]
    for cols in COLS:
        for rows in _rows_for(cols):
            P, Q = _case(rows, cols)
            want, Sa, Sb = ne.js_divergence(P, Q)
            got = entropy.js_divergence(P, Q)
            assert got.shape == (rows,) and np.isfinite(got).all()
            _hold(got, want, ne.js_bound(cols, Sa, Sb), "js %d x %d" % (rows, cols), worst)
    got = entropy.js_divergence(G["js_p"], G["js_q"])
    np.testing.assert_array_almost_equal(got, G["js_out"], 12)
    assert np.ndim(entropy.js_divergence(G["js_p"][0], G["js_q"][0])) == 0
    print("js: largest |dev - numpy| / bound = %.3f" % worst[0])


def test_shannon_rows():
    worst = [0.0]
    for cols in COLS:
        for rows in _rows_for(cols):
            P, Q = _case(rows, cols)
            p = P + Q                               # zeros where both have them
            p[p.sum(axis=1) == 0] = 1.0             # (no all-zero row: that is 0 / 0)
            want, S = ne.shannon_rows(p, normalize=True)
            got = entropy.shannon_entropy_rows(p, normalize=True)
            assert got.shape == (rows,)
            _hold(got, want, ne.shannon_norm_bound(cols, S), "H norm %dx%d" % (rows, cols),
                  worst)
            # as given: rows that do not sum to one, a negative element that counts as 0
            raw = 3.0 * P + 0.5 * Q
            raw[rows - 1, cols // 2] = -0.5
            want, S = ne.shannon_rows(raw, normalize=False)
            got = entropy.shannon_entropy_rows(raw, normalize=False)
            _hold(got, want, ne.kl_bound(cols, S), "H raw %dx%d" % (rows, cols), worst)
    assert entropy.shannon_entropy_rows(np.zeros((3, 5)), normalize=False).tolist() == [0, 0, 0]
    print("shannon: largest |dev - numpy| / bound = %.3f" % worst[0])


def test_shannon_entropy_scalar():
    p = G["sh_p"]
    want, S = ne.shannon_entropy(p)
    got = entropy.shannon_entropy(p)
    assert isinstance(got, float)
    assert abs(got - want) <= ne.shannon_norm_bound(p.size, S)
    np.testing.assert_almost_equal(got, G["sh_H"], 12)
    q = p / p.sum()
    np.testing.assert_almost_equal(entropy.shannon_entropy(q, normalize=False),
                                   G["sh_H_raw"], 12)
    # a matrix is one distribution over all its cells
    M = ne.random_rows(np.random.RandomState(3), 6, 11)
    want, S = ne.shannon_entropy(M)
    assert abs(entropy.shannon_entropy(M) - want) <= ne.shannon_norm_bound(M.size, S)
    assert entropy.shannon_entropy([0.5, 0.5]) == pytest.approx(np.log(2), abs=1e-15)


# ---- Q from assignments, the resident path -------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain(n):
    if n == 3:
        return G["ts_P"], G["ts_assignments"]
    rng = np.random.RandomState(n)
    T = ne.metastable_chain(rng, n)
    return T, ne.sample_chain(rng, T, 3, 250)


@pytest.mark.parametrize("n", [3, 65, 130])
@pytest.mark.parametrize("prior", ["default", "zero", "explicit"])
def test_resident_path_is_the_two_step_path(n, prior, monkeypatch):
    P, A = _chain(n)
    kw = {"default": {}, "zero": {"prior_counts": 0}, "explicit": {"prior_counts": 0.37}}[prior]
    Q = entropy.Q_from_assignments(A, n_states=n, **kw)
    # Q is this package's builder on the dense counts + prior, bit for bit ...
    p = ne.default_prior(A) if prior == "default" else kw["prior_counts"]
    dense = ne.dense_counts(A, n) + p
    assert Q.tobytes() == builders.normalize(dense, calculate_eq_probs=False)[1].tobytes()
    # ... and the reference's to its 7 decimals
    np.testing.assert_array_almost_equal(Q, ne.Q_from_assignments(A, n_states=n, **kw), 7)
    two_step = entropy.kl_divergence(P, Q)
    resident = entropy.relative_entropy_per_state(P, assignments=A, **kw)
    assert resident.tobytes() == two_step.tobytes()
    assert resident.tobytes() == entropy.relative_entropy_per_state(
        P, assignments=A, builder=builders.normalize, lag_time=1, **kw).tobytes()
    if prior == "zero":
        assert np.isposinf(resident).any()
    if prior != "zero" or n == 3:
        assert np.isfinite(resident[1:]).all()
    worst = [0.0]
    want, S = ne.kl_divergence(P, Q)
    _hold(resident, want, ne.kl_bound(n, S), "resident %d" % n, worst)
    # the weighted sum is numpy on the [n] vector: subset and populations
    sub = np.arange(n)[::2]
    pops = np.linspace(1.0, 2.0, len(sub))
    pops /= pops.sum()
    got = entropy.relative_entropy_msm(P, assignments=A, populations=pops, state_subset=sub, **kw)
    want = np.sum(resident[sub] * pops)
    assert got == want or (np.isposinf(got) and np.isposinf(want))
    assert entropy.relative_entropy_per_state(
        P, assignments=A, weights=pops, state_subset=sub, **kw).tobytes() == \
        (resident[sub] * pops).tobytes()
    # populations absent: this package's eq_probs of P, on the subset, renormalised --
    # the very vector the call drew, recorded as it passes
    drawn = []

    def recording(T, **kwargs):
        drawn.append(transition_matrices.eq_probs(T, **kwargs))
        return drawn[-1].copy()

    monkeypatch.setattr(entropy, "eq_probs", recording)
    for s in (None, sub):
        pick = Ellipsis if s is None else s
        for kw2 in (dict(assignments=A, **kw), dict(Q=Q)):
            got = entropy.relative_entropy_msm(P, state_subset=s, **kw2)
            w = drawn[-1][pick]
            want = np.sum(resident[pick] * (w / w.sum()))
            assert got == want or (np.isposinf(got) and np.isposinf(want))
    assert len(drawn) == 4


def test_resident_path_lag_and_ragged_input():
    P, A = _chain(65)
    rows = [A[0], A[1][:101], A[2][:7]]
    for assigns in (rows, ra.RaggedArray(rows)):
        Q = entropy.Q_from_assignments(assigns, n_states=65, lag_time=3)
        dense = ne.dense_counts(rows, 65, 3) + 1 / (250 + 101 + 7 - 3)
        assert Q.tobytes() == builders.normalize(dense, calculate_eq_probs=False)[1].tobytes()
        assert entropy.relative_entropy_per_state(P, assignments=assigns, lag_time=3).tobytes() \
            == entropy.kl_divergence(P, Q).tobytes()


@pytest.mark.parametrize("tag", ["raw", "prior", "transpose"])
def test_reference_three_state_cases(tag):
    """the reference's test_entropy.py, restated against this package, to its decimals"""
    kw = {"raw": {"prior_counts": 0}, "prior": {},
          "transpose": {"builder": builders.transpose}}[tag]
    P, A = G["ts_P"], G["ts_assignments"]
    np.testing.assert_array_almost_equal(entropy.Q_from_assignments(A, **kw),
                                         G["ts_Q_" + tag], 7)
    for per in (entropy.relative_entropy_per_state(P, assignments=A, **kw),
                entropy.relative_entropy_per_state(P, Q=G["ts_Q_" + tag])):
        np.testing.assert_array_almost_equal(per, G["ts_per_" + tag], 6)
        assert np.array_equal(np.isposinf(per), np.isposinf(G["ts_per_" + tag]))
    for msm in (entropy.relative_entropy_msm(P, assignments=A, **kw),
                entropy.relative_entropy_msm(P, Q=G["ts_Q_" + tag])):
        np.testing.assert_almost_equal(msm, G["ts_msm_" + tag], 7)


@pytest.mark.parametrize("b", ["normalize", "transpose", "mle"])
def test_chains_against_the_reference(b):
    for n in (5, 17, 40):
        k = "chain%d_" % n
        T, A, pops = G[k + "T"], G[k + "assignments"], G[k + "pops"]
        kw = {"builder": getattr(builders, b)}
        np.testing.assert_array_almost_equal(
            entropy.Q_from_assignments(A, n_states=n, **kw), G[k + "Q_" + b], 7)
        np.testing.assert_array_almost_equal(
            entropy.relative_entropy_per_state(T, assignments=A, **kw), G[k + "per_" + b], 6)
        np.testing.assert_almost_equal(
            entropy.relative_entropy_msm(T, assignments=A, populations=pops, **kw),
            G[k + "msm_" + b], 7)


# ---- state counts ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _codes(n):
    X = np.random.RandomState(n).randint(0, n, size=(SC_CHUNK + 1, 130)).astype(np.uint8)
    X[:, 7] = n - 1                         # a feature that stays in its last state
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("n", [2, 3, 4, 5, 255])
def test_state_counts(n):
    X = _codes(n)
    for frames in (1, 63, 64, 65, SC_CHUNK + 1):
        for F in (1, 63, 64, 65, 130):
            x = X[:frames, :F]
            got = entropy.state_counts(x, n)
            assert got.shape == (F, n) and got.dtype == np.int64
            want = np.stack([np.bincount(x[:, j], minlength=n) for j in range(F)])
            assert np.array_equal(got, want), (frames, F)


def test_state_counts_accumulate_ragged_and_types():
    X = _codes(3)
    trajs = [X[:300, :65], X[300:341, :65], X[341:SC_CHUNK + 1, :65]]
    want = ne.state_counts(trajs, 3)
    assert np.array_equal(entropy.state_counts(trajs, 3), want)
    assert np.array_equal(entropy.state_counts([t.astype(np.int64) for t in trajs], 3), want)
    assert np.array_equal(entropy.state_counts(ra.RaggedArray(trajs), 3), want)
    with entropy.StateCounts(65, 3) as sc:
        for t in trajs:
            sc.add(t)
        assert np.array_equal(sc.counts(), want)
        sc.add(trajs[1])
        assert np.array_equal(sc.counts(), want + ne.state_counts(trajs[1:2], 3))
    # 1-D input is one feature
    assert np.array_equal(entropy.state_counts([X[:100, 0]], 3)[0],
                          np.bincount(X[:100, 0], minlength=3))


def test_state_counts_invalid_codes():
    X = np.array(_codes(3)[:200, :5])
    X[199, 4] = 3
    with pytest.raises(DataInvalid):
        entropy.state_counts([X], 3)
    with pytest.raises(DataInvalid):
        entropy.state_counts([X.astype(np.int64) - 1], 4)
    # per-feature numbers of states: feature 4 has 3, holds a 3; feature 0 has 2, holds a 2
    with pytest.raises(DataInvalid, match="feature 4"):
        entropy.state_counts([X], [4, 4, 4, 4, 3])
    with pytest.raises(DataInvalid, match="feature 0"):
        entropy.state_counts([X[:199]], [2, 3, 3, 3, 3])


def test_state_counts_are_the_diagonal_of_joint_counts():
    X = _codes(3)[:1000, :5]
    jc = info_theory.joint_counts(X, n_x=3)
    want = np.stack([jc[i, i].sum(axis=-1) for i in range(5)])
    assert np.array_equal(entropy.state_counts(X, 3), want)


# ---- CARDS entropies -----------------------------------------------------------------------
def test_cards_entropies_against_the_golden():
    ends = np.cumsum(G["rot_lengths"])
    trajs = [G["rot_X"][e - m:e] for e, m in zip(ends, G["rot_lengths"])]
    n_states = G["rot_n_states"]
    counts = entropy.state_counts(trajs, n_states)
    assert np.array_equal(counts, G["rot_counts"])
    H = cards.shannon_entropies(trajs, n_states)
    want, S = ne.dihedral_entropies(G["rot_counts"])
    bound = ne.shannon_norm_bound(3, S)
    assert np.all(np.abs(H - want) <= bound)
    np.testing.assert_array_almost_equal(H, G["rot_H"], 12)
    assert H[4] == 0                                    # the dihedral that never moves
    res = G["rot_atom_residue"][G["rot_atom_indices"][:, 1]]
    per = cards.residue_shannon_entropies(H, n_states, res, 5)
    assert np.isnan(per[2]) and np.isnan(G["rot_residue_H"][2])
    # each residue: at most 3 entropies off by their bounds, over a capacity >= log 2, and
    # the roundings of two short sums and a division
    tol = 3 * bound.max() / np.log(2) + 8 * ne.U
    keep = np.arange(5) != 2
    assert np.all(np.abs(per[keep] - G["rot_residue_H"][keep]) <= tol)
