"""info_theory.exposons on the device: sidechain solvent accessibility (geometry.sasa),
weighted mutual information, affinity propagation.

No expected value comes from a device call: solvent accessibilities come from the
recorded counts of the brute-force restatement (tests/_numpy_sasa.py through tests/
golden/exposons_golden.npz), mutual information from tests/_numpy_wmi.py, labels from
scikit-learn as recorded in the golden.  Settings as the reference's test_exposons.py:
beta-peptide, threshold 1.0, damping 0.9."""
import os
import warnings

import numpy as np
import pytest

import _numpy_sasa as ns
import _numpy_wmi as nw
from enspara_amd.geometry import sasa
from enspara_amd.info_theory import exposons

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "exposons_golden.npz"))
SC_IDS = [G["bp_sc_atoms"][a:b] for a, b in zip(G["bp_sc_offsets"][:-1],
                                                G["bp_sc_offsets"][1:])]
RADII = sasa.radii_from_elements(G["bp_elements"])
DAMPING = list(G["ap_damping"])


def _golden_sasas(frames):
    counts = G["bp_counts"][frames].astype(np.int32)
    return ns.group_sums(ns.areas(counts, RADII, 0.28, 960), SC_IDS)


def _pipeline_weights(weights, n):
    """as exposons() prepares them"""
    return np.full((n,), 1 / n) if weights is None else np.array(weights) / sum(weights)


def _expected_mi(sasas, weights, threshold):
    w = nw.normalise(weights)
    P = nw.joint_probabilities(sasas > threshold, w, 2)
    mi, L, A = nw.mutual_information(P)
    return nw.finish(mi, 2), nw.mi_bound(len(w), 2, L, A) / np.log(2)


def test_exposons_from_sasas_on_the_golden():
    sasas = _golden_sasas(np.arange(6))
    want, bound = _expected_mi(sasas, np.full(6, 1 / 6), 1.0)
    # (the matrix scikit-learn's labels were recorded for: the same restatement where the
    # golden was made, whose libm may round a log the other way)
    assert np.all(np.abs(want - G["ap_S_3"]) <= bound)
    for d, labels in zip(DAMPING, G["ap_labels_3"]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            mi, got = exposons.exposons_from_sasas(sasas, d, np.full(6, 1 / 6), 1.0)
        ratio = np.abs(mi - want)[bound > 0] / bound[bound > 0]
        print("damping %g: MI error / bound %.3g" % (d, ratio.max(initial=0)))
        assert np.all(np.abs(mi - want) <= bound)
        assert np.array_equal(got, labels)


def test_exposons_from_coordinates():
    xyz = G["bp_xyz"][:6]
    want, bound = _expected_mi(_golden_sasas(np.arange(6)), _pipeline_weights(None, 6), 1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mi, labels = exposons.exposons(xyz, RADII, SC_IDS, damping=0.9, threshold=1.0)
    assert np.all(np.abs(mi - want) <= bound)
    assert np.array_equal(labels, G["ap_labels_3"][DAMPING.index(0.9)])


def test_exposons_pipeline_weighting():
    """the reference's test_exposons_pipeline_weighting: frames [0:3, 0:3, 3:6] against
    [0:3, 3:6] with weights [2, 2, 2, 1, 1, 1]"""
    xyz = G["bp_xyz"]
    rep = np.concatenate([xyz[0:3], xyz[0:3], xyz[3:6]])
    nor = np.concatenate([xyz[0:3], xyz[3:6]])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mi_u, exp_u = exposons.exposons(rep, RADII, SC_IDS, damping=0.9, threshold=1.0)
        mi_w, exp_w = exposons.exposons(nor, RADII, SC_IDS, damping=0.9, threshold=1.0,
                                        weights=[2, 2, 2, 1, 1, 1])
    want, bound = _expected_mi(_golden_sasas(np.arange(6)),
                               _pipeline_weights([2, 2, 2, 1, 1, 1], 6), 1.0)
    assert np.all(np.abs(mi_w - want) <= bound)
    want_u, bound_u = _expected_mi(_golden_sasas(np.array([0, 1, 2, 0, 1, 2, 3, 4, 5])),
                                   _pipeline_weights(None, 9), 1.0)
    assert np.all(np.abs(mi_u - want_u) <= bound_u)
    assert np.array_equal(exp_w, exp_u)
    assert exp_w.min() >= 0


def test_exposons_of_many_frames_with_weights():
    """all recorded frames, random weights, the default threshold's neighbour 0.5"""
    rng = np.random.RandomState(2)
    w = rng.rand(len(G["bp_xyz"]))
    sasas = _golden_sasas(np.arange(len(w)))
    want, bound = _expected_mi(sasas, _pipeline_weights(w, len(w)), 0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mi, labels = exposons.exposons(G["bp_xyz"], RADII, SC_IDS, damping=0.9, weights=w,
                                       threshold=0.5)
    assert np.all(np.abs(mi - want) <= bound)
    assert labels.shape == (10,)
