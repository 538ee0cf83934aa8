"""info_theory.weighted_joint_probabilities and weighted_mi on the device (csrc/
ek_wmi.hip: the float64 matrix cores, chunk partials summed in a fixed order).

No expected value comes from a device call.  The expected values are tests/
_numpy_wmi.py's, whose sums are math.fsum (correctly rounded).

* Dyadic weights -- integers in [1, 1024) times 2^-20, not renormalised: every partial
  sum is a multiple of 2^-20 below 2^33 * 2^-20, exact in any order, so the joint
  probabilities must be array_equal.
* General weights: |P_dev - P| <= T 2^-52 P and, before normalisation and clipping,
  |mi_dev - mi| <= 2^-52 (T (L + 3) + (S^2 + 4) sum |terms|) (_numpy_wmi.p_bound,
  mi_bound); every such test prints the largest ratio it sees.

Shapes (F, S): (1, 2) one pair; (8, 2) exactly a 16 x 16 tile; (5, 3) one row short of
it, a tile boundary inside a feature; (40, 3) 120 rows: every wave of a workgroup, two
workgroups a side, the last ragged; (17, 1) single-state features; (3, 255) the state
limit, 765 rows.  Frames: 1, 3, 4, 5 around the four frames of one MFMA, and the chunk
length, its neighbours and two chunks and a bit."""
import functools

import numpy as np
import pytest

import _numpy_wmi as nw
from enspara_amd import info_theory
from enspara_amd.info_theory import WMI_CHUNK, mutual_info

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2), (8, 2), (5, 3), (40, 3), (17, 1), (3, 255)]
FRAMES = [1, 3, 4, 5, WMI_CHUNK - 1, WMI_CHUNK, WMI_CHUNK + 1, 2 * WMI_CHUNK + 7]
T_MAX = max(FRAMES)


@functools.lru_cache(maxsize=None)
def _data(F, S):
    """codes, dyadic weights, general weights of T_MAX frames; tests take prefixes"""
    rng = np.random.RandomState(100 * F + S)
    X = nw.codes(rng, T_MAX, F, S)
    dy = rng.randint(1, 1024, size=T_MAX) * 2.0 ** -20
    ge = rng.rand(T_MAX) * np.exp(3 * rng.randn(T_MAX))
    ge[rng.rand(T_MAX) < 0.05] = 0.0
    ge[0] = 0.7
    for a in (X, dy, ge):
        a.setflags(write=False)
    return X, dy, ge


def _mi_raw(X, w, S):
    """the device's mutual information of weights used as given, before normalisation
    and clipping (what weighted_mi goes on from)"""
    return mutual_info._weighted_run(X, np.asarray(w), S, False, True, 0)[1]


@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("F,S", SHAPES)
def test_dyadic_weights_are_summed_exactly(F, S, T):
    X, w, _ = _data(F, S)
    X, w = X[:T], w[:T]
    P = info_theory.weighted_joint_probabilities(X, w, S)
    assert P.dtype == np.float64 and P.shape == (F, F, S, S)
    assert np.array_equal(P, nw.joint_probabilities(X, w, S))


@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("F,S", SHAPES)
def test_general_weights_within_the_bounds(F, S, T):
    X, _, w = _data(F, S)
    X, w = X[:T], nw.normalise(w[:T])
    want = nw.joint_probabilities(X, w, S)
    P = info_theory.weighted_joint_probabilities(X, w, S)
    err, bound = np.abs(P - want), nw.p_bound(T, want)
    ratio_p = (err[bound > 0] / bound[bound > 0]).max()
    mi_want, L, A = nw.mutual_information(want)
    mi = _mi_raw(X, w, S)
    mb = nw.mi_bound(T, S, L, A)
    ratio_mi = (np.abs(mi - mi_want) / mb).max()
    print("F %d S %d T %d: P error / bound %.3g, MI error / bound %.3g"
          % (F, S, T, ratio_p, ratio_mi))
    assert np.all(err <= bound)
    assert np.all(P[want == 0] == 0)
    assert np.all(np.abs(mi - mi_want) <= mb)
    # the public function: the same, clipped (clipping brings no two values apart)
    if S > 1:
        pub = info_theory.weighted_mi(X, w, n_feature_states=np.full(F, S), normalize=False)
        assert np.all(np.abs(pub - np.clip(mi_want, 0, np.inf)) <= mb)


def test_two_calls_give_the_same_bits():
    X, _, w = _data(40, 3)
    w = nw.normalise(w)
    a = info_theory.weighted_joint_probabilities(X, w, 3)
    b = info_theory.weighted_joint_probabilities(X, w, 3)
    assert a.tobytes() == b.tobytes()
    assert _mi_raw(X, w, 3).tobytes() == _mi_raw(X, w, 3).tobytes()


def test_repeated_frames_equal_weights():
    """the reference's own test: frames [a, a, b] with uniform weights against [a, b]
    with weights [2, 1]"""
    X, _, _ = _data(8, 2)
    a, b = X[:700], X[700:1500]
    rep, w_rep = np.vstack([a, a, b]), np.full(2200, 1.0)
    nor, w_nor = np.vstack([a, b]), np.r_[np.full(700, 2.0), np.full(800, 1.0)]
    want = nw.joint_probabilities(nor, nw.normalise(w_nor), 2)
    mi_want, L, A = nw.mutual_information(want)
    mi_rep = info_theory.weighted_mi(rep, w_rep, normalize=False)
    mi_nor = info_theory.weighted_mi(nor, w_nor, normalize=False)
    want_c = np.clip(mi_want, 0, np.inf)
    r1 = np.abs(mi_rep - want_c) / nw.mi_bound(2200, 2, L, A)
    r2 = np.abs(mi_nor - want_c) / nw.mi_bound(1500, 2, L, A)
    print("repeated / weighted: error / bound %.3g, %.3g" % (r1.max(), r2.max()))
    assert r1.max() <= 1 and r2.max() <= 1


def test_bool_features_and_the_default_number_of_states():
    X, _, w = _data(8, 2)
    X, w = X[:300], w[:300]
    want = nw.joint_probabilities(X, nw.normalise(w), 2)
    mi_want, L, A = nw.mutual_information(want)
    mi = info_theory.weighted_mi(X.astype(bool), w)
    assert np.all(np.abs(mi - nw.finish(mi_want, 2)) <= nw.mi_bound(300, 2, L, A) / np.log(2))
    assert np.array_equal(mi, info_theory.weighted_mi(X.astype(np.int16), w))
    assert np.array_equal(
        mi, info_theory.weighted_mi(X, w, n_feature_states=[2] * 8))


def test_per_feature_states_normalise_by_the_narrower():
    X, _, w = _data(5, 3)
    X, w = X[:500].copy(), w[:500]
    X[:, 1] = X[:, 1] % 2
    n = np.array([3, 2, 3, 3, 3])
    raw = info_theory.weighted_mi(X, w, n_feature_states=n, normalize=False)
    got = info_theory.weighted_mi(X, w, n_feature_states=n)
    assert np.array_equal(got, nw.finish(raw, n))


def test_feature_stuck_in_one_state_gives_a_zero_row():
    """With weights 2^-10 on 1024 frames every sum is exact, the stuck feature's
    probability is 1 and its terms are P log(1) = 0: a row of zeros.  With general
    weights the sum of the weights is 1 only to rounding, and the row is zero to within
    the bound."""
    X, _, w = _data(5, 3)
    X = X[:1024].copy()
    X[:, 2] = 1
    mi = info_theory.weighted_mi(X, np.full(1024, 2.0 ** -10), n_feature_states=[3] * 5)
    assert np.all(mi[2] == 0) and np.all(mi[:, 2] == 0)
    assert mi[0, 0] > 0
    wn = nw.normalise(w[:1024])
    mi_want, L, A = nw.mutual_information(nw.joint_probabilities(X, wn, 3))
    assert np.abs(mi_want[2]).max() <= 2.0 ** -50
    mi = _mi_raw(X, wn, 3)
    assert np.all(np.abs(mi - mi_want) <= nw.mi_bound(1024, 3, L, A))


def test_weights_with_zeros():
    X, _, w = _data(5, 3)
    X, w = X[:1000], w[:1000].copy()
    w[::2] = 0.0
    wn = nw.normalise(w)
    want = nw.joint_probabilities(X, wn, 3)
    assert np.array_equal(want, nw.joint_probabilities(X[1::2], wn[1::2], 3))
    P = info_theory.weighted_joint_probabilities(X, wn, 3)
    assert np.all(np.abs(P - want) <= nw.p_bound(500, want))
    mi_want, L, A = nw.mutual_information(want)
    mi = info_theory.weighted_mi(X, w, normalize=False)
    assert np.all(np.abs(mi - np.clip(mi_want, 0, np.inf)) <= nw.mi_bound(500, 3, L, A))


def test_normalize_false():
    X, _, w = _data(8, 2)
    X, w = X[:400], w[:400]
    raw = info_theory.weighted_mi(X, w, normalize=False)
    assert np.array_equal(info_theory.weighted_mi(X, w), nw.finish(raw, 2))
    assert raw.min() >= 0
