"""enspara_amd.info_theory without a device: the numpy restatement the GPU tests
expect from (tests/_numpy_mi.py) against the real reference's outputs
(tests/golden/mi_golden.npz), the host-side conversions against the reference's
known answers and golden outputs, every validator's DataInvalid, and the argument
errors that are raised before any device call."""
import os
import warnings

import numpy as np
import pytest

import _numpy_mi as nm
from enspara_amd import info_theory
from enspara_amd.exception import DataInvalid, PerformanceWarning
from enspara_amd.info_theory import mutual_info

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "mi_golden.npz"))


# ---- the restatement against the reference ------------------------------------------------
@pytest.mark.parametrize("tag,nx,ny", [("rag", 3, 5), ("self", 3, 3)])
def test_restatement_equals_the_reference(tag, nx, ny):
    X = G[tag + "_X"]
    Y = G["rag_Y"] if tag == "rag" else None
    jc = nm.joint_counts(X, Y, nx, ny)
    assert jc.dtype == np.uint32
    assert np.array_equal(jc, G[tag + "_jc"])
    mi, S = nm.mutual_information(jc)
    assert np.array_equal(mi, G[tag + "_mi"])
    assert np.all(S >= np.abs(mi))


def test_restatement_binning_table():
    """the reference's test_joint_count_binning"""
    trj1 = np.array([1] * 3 + [2] * 6 + [1] * 6)
    trj2 = np.array([1] * 9 + [0] * 3 + [2] * 3)
    expected = np.array([[0, 0, 0], [3, 3, 3], [0, 6, 0]])[None, None, ...]
    assert np.array_equal(nm.joint_counts(trj1, trj2), expected)
    assert np.array_equal(nm.joint_counts(trj1, trj2, 3, 3), expected)


def test_golden_is_asymmetric_as_the_reference_is():
    """X against itself: symmetric only to rounding (nothing mirrors it)"""
    mi = G["self_mi"]
    assert np.any(mi != mi.T)
    assert np.abs(mi - mi.T).max() < 1e-15


# ---- host-side conversions ----------------------------------------------------------------------
def test_mi_to_apc_table():
    mi = np.array([[1.0, 0.5, 0.1], [0.5, 0.7, 0.1], [0.1, 0.1, 0.7]])
    apc = info_theory.mi_to_apc(mi)
    expected = np.array([[0.1400, 0.0955, 0.0244], [0.0955, 0.0833, 0.0211],
                         [0.0244, 0.0211, 0.0566]])
    np.testing.assert_allclose(apc[0, 0], np.sum(mi[0, :] ** 2) / 9)
    np.testing.assert_almost_equal(apc, expected, decimal=4)


def test_conversions_equal_the_reference():
    mi = G["conv_mi"]
    keep = mi.copy()
    assert np.array_equal(info_theory.mi_to_apc(mi), G["conv_apc"])
    assert np.array_equal(info_theory.mi_to_nmi(mi), G["conv_nmi"])
    assert np.array_equal(info_theory.mi_to_nmi_apc(mi), G["conv_nmi_apc"])
    assert np.array_equal(mi, keep)


def test_nmi_tables():
    mi = np.array([[1.0, 0.1], [0.1, 1.0]])
    nmi = info_theory.mi_to_nmi(mi)
    np.testing.assert_allclose(nmi, [[1.0, 0.052632], [0.052632, 1.0]], rtol=1e-4)
    mi[0, 0] = mi[1, 1] = 0
    np.testing.assert_allclose(info_theory.mi_to_nmi(mi, H_marginal=np.array([1, 1])), nmi)
    np.testing.assert_allclose(info_theory.mi_to_nmi(np.diag([1.7, 1.7])), np.eye(2))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        z = info_theory.mi_to_nmi(np.array([[0.0001, 0.1], [0.1, -0]]))
    assert len(w) > 0 and np.all(~np.isnan(z))


def test_nmi_apc_tables():
    np.testing.assert_almost_equal(info_theory.mi_to_nmi_apc(np.diag([1.7, 1.7])),
                                   [[0.575, 0.0], [0, 0.575]])
    np.testing.assert_almost_equal(
        info_theory.mi_to_nmi_apc(np.array([[1.7, 0.2], [0.2, 1.7]])),
        [[0.574, 0.005], [0.005, 0.574]], decimal=2)


def test_network_deconvolution():
    G_dir = np.array([[0.5, 0.4, 0.1], [0.2, 0.7, 0.1], [0.1, 0.2, 0.7]])
    G_obs = G_dir.copy()
    for i in range(2, 1000):
        G_obs += np.linalg.matrix_power(G_dir, i)
    np.testing.assert_allclose(G_dir, info_theory.deconvolute_network(G_obs), atol=1e-3)


def test_channel_capacity_normalization():
    mi = G["self_mi"]
    assert np.array_equal(info_theory.channel_capacity_normalization(mi, 3, 3),
                          G["self_mimat"])
    assert np.array_equal(info_theory.channel_capacity_normalization(mi, [3] * 24, [3] * 24),
                          G["self_mimat"])
    # not square: [i, j] over log(min(n_x[i], n_y[j]))
    out = info_theory.channel_capacity_normalization(np.ones((2, 3)), [2, 5], [3, 4, 9])
    assert np.array_equal(out, 1 / np.log([[2, 2, 2], [3, 4, 5]]))


def test_check_features_states():
    same = [np.zeros((2, 3), dtype=int), np.zeros((2, 3), dtype=int)]
    info_theory.check_features_states(same, [2, 2, 2])
    with pytest.raises(DataInvalid):
        info_theory.check_features_states(same, [2, 2])
    info_theory.check_features_states([np.zeros((2, 3), dtype=int),
                                       np.zeros((1, 3), dtype=int)], [2, 2, 2])
    with pytest.raises(DataInvalid):
        info_theory.check_features_states([np.zeros((2, 2), dtype=int),
                                           np.zeros((2, 3), dtype=int)], [3])


# ---- validators -------------------------------------------------------------------------------------
def test_joint_counts_matrix_validator():
    with pytest.raises(DataInvalid, match="2D"):
        mutual_info._validate_joint_counts_matrix(np.zeros((3, 3), dtype=int))
    with pytest.raises(DataInvalid, match="4D"):
        mutual_info._validate_joint_counts_matrix(np.zeros((3, 3, 3), dtype=int))
    jc = np.zeros((1, 1, 3, 3), dtype=int)
    assert mutual_info._validate_joint_counts_matrix(jc) is jc
    # (mutual_information validates before it opens a device)
    with pytest.raises(DataInvalid):
        info_theory.mutual_information(np.zeros((3, 3), dtype=int))


def test_mutual_information_matrix_validator():
    with pytest.raises(DataInvalid, match="2D"):
        info_theory.mi_to_apc(np.zeros(3))
    with pytest.raises(DataInvalid, match="square"):
        info_theory.mi_to_apc(np.zeros((2, 3)))
    with pytest.raises(DataInvalid, match="symmetric"):
        info_theory.mi_to_nmi(np.array([[1., 0.2], [0.1, 1.]]))
    with pytest.raises(DataInvalid, match="symmetric"):
        info_theory.mi_to_nmi_apc(np.array([[1., 0.2], [0.1, 1.]]))


def test_feature_states_validator():
    v = mutual_info._validate_feature_states_array
    assert np.array_equal(v(3, 4), [3, 3, 3, 3])
    assert np.array_equal(v([2, 3], 2), [2, 3])
    with pytest.raises(DataInvalid, match="n_states < 1"):
        v(1, 3)
    with pytest.raises(DataInvalid, match="n_states < 1"):
        v([2, 0], 2)
    with pytest.raises(DataInvalid, match="must match"):
        v([2, 2], 3)
    with pytest.raises(DataInvalid, match="integral"):
        v([2.0, 2.5], 2)
    with pytest.raises(DataInvalid):
        info_theory.channel_capacity_normalization(np.zeros((2, 2)), 2, [2, 2, 2])


def test_nmi_marginal_errors():
    mi = np.array([[1.0, 0.1], [0.1, 1.0]])
    with pytest.raises(DataInvalid, match="same length"):
        info_theory.mi_to_nmi(mi, H_marginal=np.array([1., 1., 1.]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(DataInvalid, match="non-zero"):
            info_theory.mi_to_nmi(mi, H_marginal=np.array([0., 0.]))
        with pytest.raises(DataInvalid, match="nan"):
            info_theory.mi_to_nmi(mi, H_marginal=np.array([1., np.nan]))


# ---- argument errors raised before any device call --------------------------------------------
def test_state_limit_is_named():
    X = np.zeros((4, 2), dtype=np.int64)
    with pytest.raises(DataInvalid, match="255"):
        info_theory.joint_counts(X, n_x=256)
    with pytest.raises(DataInvalid, match="255"):
        info_theory.joint_counts(X, X, 3, 256)
    X[2, 1] = 255           # max + 1 = 256 states
    with pytest.raises(DataInvalid, match="255"):
        info_theory.joint_counts(X)
    with pytest.raises(DataInvalid):
        info_theory.joint_counts(X, n_x=0)
    assert info_theory.MAX_STATES == 255 and info_theory.MI_CHUNK % 64 == 0


def test_code_checks_need_no_device():
    check = mutual_info._codes
    with pytest.raises(DataInvalid, match=r"\[0, 3\)"):
        check(np.array([[0, 3]]), 3, "X")
    with pytest.raises(DataInvalid, match=r"\[0, 3\)"):
        check(np.array([[0, -1]]), 3, "X")
    with pytest.raises(DataInvalid, match="state indices"):
        check(np.array([[0.5, 1.0]]), 3, "X")
    with pytest.raises(DataInvalid):
        check(np.zeros((2, 2, 2), dtype=int), 3, "X")
    for dt in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64,
               np.uint64):
        c = check(np.array([[0, 126], [7, 1]], dtype=dt).T, 127, "X")
        assert c.dtype == np.uint8 and c.flags.c_contiguous
        assert np.array_equal(c, [[0, 7], [126, 1]])


def test_prepare_xy_follows_the_reference():
    p = mutual_info._prepare_xy
    x = np.array([0, 2, 1])
    X, Y, nx, ny = p(x, None, None, None)
    assert X.shape == (3, 1) and Y is None and (nx, ny) == (3, 3)
    with pytest.warns(UserWarning, match="n_y unused"):
        p(x, None, 3, 4)
    with pytest.warns(PerformanceWarning, match="uptyped"):
        X, Y, nx, ny = p(x.astype(np.int8), np.array([0, 4, 1], dtype=np.int32), None, None)
    assert (nx, ny) == (3, 5) and Y.shape == (3, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        p(x, x.copy(), None, None)


def test_feature_limit_is_named():
    assert mutual_info.MAX_FEATURES == 65535 * 64
    with pytest.raises(DataInvalid, match=str(mutual_info.MAX_FEATURES)):
        mutual_info.JointCounts(mutual_info.MAX_FEATURES + 1, 1, 1, 2)
    with pytest.raises(DataInvalid, match=str(mutual_info.MAX_FEATURES)):
        mutual_info.JointCounts(1, mutual_info.MAX_FEATURES + 1, 1, 2)
    with pytest.raises(DataInvalid):
        mutual_info.JointCounts(0, 1, 2, 2)


def test_conversions_on_small_cases_by_hand():
    """mi_to_nmi and mi_to_nmi_apc entry by entry from their definitions"""
    mi = np.array([[0.9, 0.2, 0.0], [0.2, 0.7, 0.1], [0.0, 0.1, 0.5]])
    H = np.diag(mi)
    nmi = info_theory.mi_to_nmi(mi)
    apc = info_theory.mi_to_apc(mi)
    out = info_theory.mi_to_nmi_apc(mi)
    for i in range(3):
        for j in range(3):
            hj = H[i] + H[j] - mi[i, j]
            assert nmi[i, j] == (1.0 if i == j else mi[i, j] / hj)
            assert apc[i, j] == pytest.approx(sum(mi[i, r] * mi[r, j] for r in range(3)) / 9,
                                              rel=1e-15)
            want = 0.0 if mi[i, j] == 0 else (mi[i, j] - apc[i, j]) / hj
            assert out[i, j] == pytest.approx(want, rel=1e-14, abs=0)
    # given marginals replace the diagonal; a list is fine
    assert np.array_equal(info_theory.mi_to_nmi(mi, H_marginal=list(H)), nmi)
