"""The host side of exposons: sphere points, sidechain selection, condensing, affinity
propagation, argument errors, and the numpy restatement of Shrake-Rupley
(tests/_numpy_sasa.py) on cases with a known answer.  No device is needed.

Affinity propagation is held to scikit-learn's labels and iteration counts as recorded
in tests/golden/exposons_golden.npz (make_exposons_golden.py), and to scikit-learn
itself where it is installed."""
import math
import os
import warnings

import numpy as np
import pytest

import _numpy_sasa as ns
from enspara_amd.exception import DataInvalid
from enspara_amd.geometry import sasa
from enspara_amd.info_theory import _affinity, exposons, mutual_info

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "exposons_golden.npz"))
SC_IDS = [G["bp_sc_atoms"][a:b] for a, b in zip(G["bp_sc_offsets"][:-1],
                                                G["bp_sc_offsets"][1:])]
AP_MATRICES = [0, 1, 2, 3]


# ---- sphere points -------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 960])
def test_sphere_points(n):
    s = sasa.sphere_points(n)
    assert s.dtype == np.float32 and s.shape == (n, 3)
    norm = np.sqrt((s.astype(np.float64) ** 2).sum(axis=1))
    # three components each rounded to float32: within 2^-24 relative each
    assert np.abs(norm - 1).max() <= 3 * 2.0 ** -24
    y = np.arange(n) * (2.0 / n) - 1.0 + 1.0 / n
    assert np.array_equal(s[:, 1], y.astype(np.float32))
    assert np.array_equal(s, ns.sphere_points(n))


def test_radii_from_elements():
    r = sasa.radii_from_elements(["H", "c", "N", "O", "CL", " S"])
    assert r.dtype == np.float32
    assert np.array_equal(r, np.array([0.12, 0.17, 0.155, 0.152, 0.175, 0.18], np.float32))
    for sym in ("H", "C", "N", "O", "F", "P", "S", "Cl"):
        assert sasa.ATOMIC_RADII[sym] > 0
    with pytest.raises(DataInvalid):
        sasa.radii_from_elements(["C", "Xx"])


# ---- sidechains ----------------------------------------------------------------------
def test_sidechain_atom_ids_equal_the_reference_lists():
    ids = exposons.get_sidechain_atom_ids(G["bp_names"], G["bp_resid"])
    assert len(ids) >= 10
    for got, want in zip(ids, SC_IDS):
        assert np.array_equal(got, want)
    assert int(G["bp_sc_offsets"][-1]) == sum(len(i) for i in SC_IDS)
    with pytest.raises(DataInvalid):
        exposons.get_sidechain_atom_ids(["N", "CA"], [0])


def test_condense_sidechain_sasas():
    rng = np.random.RandomState(3)
    sasas = rng.rand(5, 175).astype(np.float32)
    got = exposons.condense_sidechain_sasas(sasas, SC_IDS)
    assert got.dtype == np.float32 and got.shape == (5, 10)
    for f in range(5):
        for g, ids in enumerate(SC_IDS):
            acc = np.float32(0.0)
            for a in ids:
                acc = np.float32(acc + sasas[f, a])
            assert got[f, g] == acc
            # n - 1 additions (the first, to 0, is exact), each within 2^-24 of a partial
            # sum no larger than the whole; np.sum's pairwise tree is held to the same
            n = len(ids)
            assert abs(float(got[f, g]) - float(np.sum(sasas[f, ids]))) <= \
                2 * (n - 1) * 2.0 ** -24 * float(np.sum(sasas[f, ids], dtype=np.float64))
    # any order, overlap
    odd = [np.array([7, 3, 7]), np.array([174])]
    got = exposons.condense_sidechain_sasas(sasas, odd)
    assert np.array_equal(got[:, 0], (sasas[:, 7] + sasas[:, 3]) + sasas[:, 7])
    assert np.array_equal(got, ns.group_sums(sasas, odd))
    with pytest.raises(DataInvalid):
        exposons.condense_sidechain_sasas(sasas[:, :100], SC_IDS)
    with pytest.raises(DataInvalid):
        exposons.condense_sidechain_sasas(sasas, [np.array([1]), np.array([], dtype=int)])


# ---- affinity propagation ---------------------------------------------------------------
@pytest.mark.parametrize("k", AP_MATRICES)
def test_affinity_propagation_equals_the_golden(k):
    S = G["ap_S_%d" % k]
    keep = S.copy()
    for d, labels, n_iter in zip(G["ap_damping"], G["ap_labels_%d" % k], G["ap_iter_%d" % k]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got, it = _affinity.affinity_propagation(S, d, return_n_iter=True)
        assert np.array_equal(got, labels), (k, d)
        assert it == n_iter, (k, d)
    assert np.array_equal(S, keep)


def test_affinity_propagation_of_equal_similarities():
    with pytest.warns(UserWarning, match="equal similarities"):
        got = _affinity.affinity_propagation(np.zeros((6, 6)), 0.9)
    assert np.array_equal(got, G["ap_zero_labels"])
    with pytest.warns(UserWarning):
        assert np.array_equal(_affinity.affinity_propagation(np.zeros((1, 1)), 0.9), [0])
    # a preference above the similarities: every point its own cluster
    with pytest.warns(UserWarning):
        got = _affinity.affinity_propagation(np.full((4, 4), -1.0), 0.9)
    assert np.array_equal(got, np.arange(4))


def test_affinity_propagation_that_does_not_converge():
    with pytest.warns(_affinity.ConvergenceWarning):
        got, it = _affinity.affinity_propagation(G["ap_S_0"], 0.9, max_iter=5,
                                                 return_n_iter=True)
    assert np.array_equal(got, G["ap_short_labels"])
    assert it == int(G["ap_short_iter"]) == 5


def test_affinity_propagation_equals_sklearn():
    cluster = pytest.importorskip("sklearn.cluster")
    rng = np.random.RandomState(11)
    mats = [G["ap_S_%d" % k] for k in AP_MATRICES]
    for n in (2, 3, 9, 30):
        a = rng.rand(n, n) * (rng.rand(n, n) < 0.7)
        mats.append(a + a.T)
    for S in mats:
        for d in (0.5, 0.75, 0.9, 0.95):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                c = cluster.AffinityPropagation(damping=d, affinity="precomputed",
                                                preference=0, max_iter=10000,
                                                random_state=0).fit(S)
                got, it = _affinity.affinity_propagation(S, d, return_n_iter=True)
            assert np.array_equal(got, c.labels_), (S.shape, d)
            assert it == c.n_iter_, (S.shape, d)


def test_affinity_propagation_argument_errors():
    with pytest.raises(ValueError):
        _affinity.affinity_propagation(np.zeros((3, 4)), 0.9)
    with pytest.raises(ValueError):
        _affinity.affinity_propagation(np.zeros((3, 3)), 0.3)
    with pytest.raises(ValueError):
        _affinity.affinity_propagation(np.zeros((3, 3)), 1.0)


# ---- argument errors (all raised before the device is touched) -----------------------------
def test_shrake_rupley_argument_errors():
    xyz = np.zeros((2, 4, 3), dtype=np.float32)
    xyz[:, :, 0] = np.arange(4)
    radii = np.full(4, 0.17)
    bad = xyz.copy()
    bad[1, 2, 1] = np.nan
    far = xyz.copy()
    far[0, 0, 2] = np.nextafter(np.float32(sasa.MAX_COORD), np.float32(np.inf))
    inf = xyz.copy()
    inf[0, 3, 0] = -np.inf
    cases = [
        dict(xyz=bad), dict(xyz=far), dict(xyz=inf), dict(xyz=xyz[0]),
        dict(xyz=xyz.astype(np.float64)),
        dict(radii=np.array([0.17, 0.0, 0.17, 0.17])),
        dict(radii=np.array([0.17, -0.1, 0.17, 0.17])),
        dict(radii=np.full(3, 0.17)),
        dict(radii=np.full(4, 5.0)),
        dict(n_sphere_points=0), dict(n_sphere_points=sasa.MAX_POINTS + 1),
        dict(n_sphere_points=9.5),
        dict(atom_groups=[[0, 1], []]), dict(atom_groups=[[0, 4]]),
        dict(atom_groups=[[-1]]), dict(atom_groups=[]),
        dict(chunk_frames=0),
    ]
    for kw in cases:
        args = dict(xyz=xyz, radii=radii)
        args.update(kw)
        with pytest.raises(DataInvalid):
            sasa.shrake_rupley(**args)


def test_weighted_mi_argument_errors():
    X = np.array([[0, 1], [1, 0], [1, 1]])
    w = np.array([0.5, 0.25, 0.25])
    with pytest.raises(DataInvalid, match="didn't match the number of weights"):
        mutual_info.weighted_mi(X, w[:2])
    with pytest.raises(DataInvalid, match="feature states number vector"):
        mutual_info.weighted_mi(X, w, n_feature_states=[2, 2, 2])
    for kw in [dict(weights=np.array([0.5, -0.25, 0.75])), dict(weights=np.zeros(3)),
               dict(weights=np.array([0.5, np.nan, 0.5])),
               dict(features=X[:, 0]), dict(weights=w[:, None]),
               dict(features=np.array([[0, 2], [1, 0], [1, 1]]), n_feature_states=[2, 2]),
               dict(features=np.array([[0, -1], [1, 0], [1, 1]])),
               dict(features=X * 300),
               dict(features=X.astype(float))]:
        args = dict(features=X, weights=w)
        args.update(kw)
        with pytest.raises(DataInvalid):
            mutual_info.weighted_mi(**args)
    with pytest.raises(DataInvalid):
        mutual_info.weighted_joint_probabilities(X, w, 1)
    with pytest.raises(DataInvalid):
        mutual_info.weighted_joint_probabilities(X, w, mutual_info.MAX_STATES + 1)
    with pytest.raises(DataInvalid):
        mutual_info.weighted_joint_probabilities(X, w[:2], 2)


# ---- the numpy Shrake-Rupley on cases with a known answer ----------------------------------
def test_numpy_sasa_of_an_isolated_atom():
    xyz = np.array([[[0.3, -0.2, 0.1]]], dtype=np.float32)
    for n in (1, 96, 960):
        c = ns.counts(xyz, [0.17], 0.14, n)
        assert c[0, 0] == n
        a = ns.areas(c, [0.17], 0.14, n)
        R = float(np.float32(0.17) + np.float32(0.14))
        # c, c R, c R R and the product with n: four float32 roundings (a fifth for their products)
        assert abs(float(a[0, 0]) - 4 * math.pi * R * R) <= 5 * 2.0 ** -24 * 4 * math.pi * R * R


@pytest.mark.parametrize("d", [0.05, 0.2, 0.31, 0.5, 0.61, 0.63, 1.0])
def test_numpy_sasa_of_two_equal_spheres(d):
    """Two spheres of radius R at distance d < 2 R: the cap of each inside the other has
    height R - d / 2, so the fraction 1 / 2 + d / (4 R) of its points stays accessible."""
    n = 960
    xyz = np.array([[[0.0, 0.0, 0.0], [0.0, d, 0.0]]], dtype=np.float32)
    c = ns.counts(xyz, [0.17, 0.17], 0.14, n)
    R = float(np.float32(0.17) + np.float32(0.14))
    frac = 1.0 if d >= 2 * R else 0.5 + d / (4 * R)
    # the spiral has one point per band of height 2 / n in y, the axis of the pair: a cap
    # holds its share of the points to within one band at its edge (2 / n with rounding)
    assert abs(c[0, 0] / n - frac) <= 2.0 / n
    assert abs(c[0, 1] / n - frac) <= 2.0 / n


def test_numpy_sasa_repeats_the_golden_counts():
    """the recorded counts of the beta-peptide frames are the brute-force helper's"""
    radii = sasa.radii_from_elements(G["bp_elements"])
    for f in (0, len(G["bp_xyz"]) - 1):
        c = ns.counts(G["bp_xyz"][f:f + 1], radii, 0.28, 960)
        assert np.array_equal(c[0], G["bp_counts"][f])
