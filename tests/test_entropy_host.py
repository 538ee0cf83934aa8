"""enspara_amd.info_theory.entropy without a device: the numpy restatement the GPU tests
expect from (tests/_numpy_entropy.py) reproduces what the real reference recorded in
tests/golden/entropy_golden.npz to the reference's own decimals (7 for Q, 6 per state, 7
for whole models: its test_entropy.py), the argument errors, the parts that are numpy
here as there, and what the modules export."""
import inspect
import os

import numpy as np
import pytest
import scipy.sparse

import _numpy_entropy as ne
from enspara_amd import cards, info_theory
from enspara_amd.exception import DataInvalid
from enspara_amd.info_theory import entropy
from enspara_amd.msm import builders

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "entropy_golden.npz"))

# the literals of the reference's test_entropy.py, as the generator recomputed them
TS = {"raw": ({"prior_counts": 0}, [np.inf, 0.20751875, 0.84983615], np.inf),
      "prior": ({}, [3.05675367, 0.20484462, 0.84793052], 0.979737855),
      "transpose": ({"builder": "transpose"}, [2.9341145, 0.15950137, 0.91261408],
                    0.98622475852)}


def test_golden_holds_the_references_literals():
    for tag, (_, per, msm) in TS.items():
        np.testing.assert_array_almost_equal(G["ts_per_" + tag], per, 6)
        np.testing.assert_almost_equal(G["ts_msm_" + tag], msm, 7)
    np.testing.assert_array_almost_equal(G["kl_base_2"], [1., 0.0, 0.84409397], 7)
    np.testing.assert_array_almost_equal(G["kl_base_e"], [0.6931472, 0.0, 0.58508136], 7)
    np.testing.assert_array_almost_equal(G["kl_base_10"], [0.3010299957, 0.0, 0.25409760], 7)
    np.testing.assert_array_almost_equal(
        G["ts_Q_raw"], [[0., 0.57142857, 0.42857143], [0.375, 0.375, 0.25],
                        [0.28571429, 0.42857143, 0.28571429]], 7)


@pytest.mark.parametrize("tag", sorted(TS))
def test_restatement_three_state(tag):
    kw = TS[tag][0]
    P, A = G["ts_P"], G["ts_assignments"]
    Q = ne.Q_from_assignments(A, **kw)
    np.testing.assert_array_almost_equal(Q, G["ts_Q_" + tag], 7)
    per, _ = ne.relative_entropy_per_state(P, Q)
    np.testing.assert_array_almost_equal(per, G["ts_per_" + tag], 6)
    assert np.array_equal(np.isposinf(per), np.isposinf(G["ts_per_" + tag]))
    pops = G["ts_pops"] / G["ts_pops"].sum()
    np.testing.assert_almost_equal(ne.relative_entropy_msm(P, Q, pops), G["ts_msm_" + tag], 7)
    # ... and from the recorded Q, as the reference's test does
    np.testing.assert_array_almost_equal(
        ne.relative_entropy_per_state(P, G["ts_Q_" + tag])[0], G["ts_per_" + tag], 6)


@pytest.mark.parametrize("tag, base", [("2", 2), ("e", np.e), ("10", 10)])
def test_restatement_kl_bases(tag, base):
    want = G["kl_base_" + tag]
    np.testing.assert_array_almost_equal(ne.kl_divergence(G["kl_P"], G["kl_Q"], base)[0],
                                         want, 7)
    for r in range(3):
        np.testing.assert_almost_equal(
            ne.kl_divergence(G["kl_P"][r], G["kl_Q"][r], base)[0], want[r], 7)


def test_restatement_js_and_shannon():
    np.testing.assert_array_almost_equal(ne.js_divergence(G["js_p"], G["js_q"])[0],
                                         G["js_out"], 12)
    np.testing.assert_almost_equal(ne.shannon_entropy(G["sh_p"])[0], G["sh_H"], 12)
    p = G["sh_p"] / G["sh_p"].sum()
    np.testing.assert_almost_equal(ne.shannon_entropy(p, False)[0], G["sh_H_raw"], 12)


@pytest.mark.parametrize("n", [5, 17, 40])
@pytest.mark.parametrize("b", ["normalize", "transpose", "mle"])
def test_restatement_chains(n, b):
    k = "chain%d_" % n
    T, A, pops = G[k + "T"], G[k + "assignments"], G[k + "pops"]
    if b != "mle":      # (mle's Q is an iteration; its restatement is tests/_numpy_prinz.py)
        np.testing.assert_array_almost_equal(
            ne.Q_from_assignments(A, n_states=n, builder=b), G[k + "Q_" + b], 7)
    per, _ = ne.relative_entropy_per_state(T, G[k + "Q_" + b])
    np.testing.assert_array_almost_equal(per, G[k + "per_" + b], 6)
    np.testing.assert_almost_equal(ne.relative_entropy_msm(T, G[k + "Q_" + b], pops),
                                   G[k + "msm_" + b], 7)


def test_restatement_rotamers():
    ends = np.cumsum(G["rot_lengths"])
    trajs = [G["rot_X"][e - m:e] for e, m in zip(ends, G["rot_lengths"])]
    counts = ne.state_counts(trajs, 3)
    assert np.array_equal(counts, G["rot_counts"])
    H, _ = ne.dihedral_entropies(counts)
    np.testing.assert_array_almost_equal(H, G["rot_H"], 12)
    res = G["rot_atom_residue"][G["rot_atom_indices"][:, 1]]
    np.testing.assert_array_almost_equal(
        ne.residue_entropies(H, G["rot_n_states"], res, 5), G["rot_residue_H"], 12)


def test_residue_entropies_against_the_golden():
    """Host numpy: NaN where a residue has no dihedral; elsewhere within 8 * 2^-52
    relative of the reference's value.  A residue here has at most 3 dihedrals: its sum
    of entropies and its sum of logarithms take at most 2 adds each (half an ulp an add,
    on either side, whatever the order), each logarithm is within an ulp on either side
    (2), and the division rounds once on each side (1): 2 + 2 + 2 + 1 = 7 < 8."""
    res = G["rot_atom_residue"][G["rot_atom_indices"][:, 1]]
    got = cards.residue_shannon_entropies(G["rot_H"], G["rot_n_states"], res, 5)
    want = G["rot_residue_H"]
    assert np.isnan(got[2]) and np.isnan(want[2])
    keep = np.arange(5) != 2
    assert np.isfinite(got[keep]).all()
    assert np.all(np.abs(got[keep] - want[keep]) <= 8 * ne.U * np.abs(want[keep]))
    assert max(np.bincount(res)) <= 3
    with pytest.raises(DataInvalid):
        cards.residue_shannon_entropies(G["rot_H"], G["rot_n_states"], res.astype(float), 5)
    with pytest.raises(DataInvalid):
        cards.residue_shannon_entropies(G["rot_H"], G["rot_n_states"], res, 4)
    with pytest.raises(DataInvalid):
        cards.residue_shannon_entropies(G["rot_H"][:-1], G["rot_n_states"], res, 5)


def test_energy_to_probability():
    u = np.array([0.0, 1.0, 2.5, -0.3])
    p = entropy.energy_to_probability(u)
    w = np.exp(-(u - u.mean()) / 2.479)
    assert np.array_equal(p, w / w.sum())
    np.testing.assert_allclose(entropy.energy_to_probability(u, kT=1.0).sum(), 1.0, rtol=1e-15)


def test_argument_errors_before_any_device_call():
    P = G["kl_P"]
    with pytest.raises(DataInvalid, match="same shape"):
        entropy.kl_divergence(P, P[:2])
    with pytest.raises(DataInvalid, match="same shape"):
        entropy.js_divergence(P[0], P[0, :2])
    with pytest.raises(DataInvalid, match="sparse"):
        entropy.kl_divergence(scipy.sparse.csr_matrix(P), P)
    with pytest.raises(DataInvalid):
        entropy.kl_divergence(np.zeros((2, 2, 2)), np.zeros((2, 2, 2)))
    with pytest.raises(DataInvalid):
        entropy.kl_divergence(np.zeros((0, 3)), np.zeros((0, 3)))
    with pytest.raises(DataInvalid, match="pass Q"):
        entropy.relative_entropy_per_state(P)
    with pytest.raises(DataInvalid, match="pass Q"):
        entropy.relative_entropy_msm(P, populations=np.ones(3) / 3)
    for f in (entropy.relative_entropy_per_state, entropy.relative_entropy_msm):
        with pytest.raises(DataInvalid, match="sparse"):
            f(scipy.sparse.csr_matrix(P), Q=P)
        with pytest.raises(DataInvalid, match="sparse"):
            f(P, Q=scipy.sparse.csr_matrix(P), populations=np.ones(3) / 3)
    with pytest.raises(DataInvalid, match="sparse"):
        entropy.shannon_entropy(scipy.sparse.csr_matrix(P))
    with pytest.raises(DataInvalid):
        entropy.shannon_entropy_rows(np.ones(3))
    with pytest.raises(DataInvalid):
        entropy.shannon_entropy(np.zeros(0))
    with pytest.raises(DataInvalid):
        entropy.state_counts([], 3)
    with pytest.raises(DataInvalid):
        entropy.state_counts([np.zeros((4, 2), dtype=int)], [3, 3, 3])
    with pytest.raises(DataInvalid):
        entropy.state_counts([np.zeros((4, 2), dtype=int)], 3.0)
    with pytest.raises(DataInvalid):
        entropy.StateCounts(3, 256)
    with pytest.raises(DataInvalid):
        entropy.StateCounts(0, 3)


def test_exports_and_signatures():
    assert sorted(entropy.__all__) == sorted([
        "Q_from_assignments", "relative_entropy_per_state", "relative_entropy_msm",
        "energy_to_probability", "shannon_entropy", "shannon_entropy_rows",
        "kl_divergence", "js_divergence", "state_counts", "StateCounts", "last_timing"])
    assert info_theory.entropy is entropy and "entropy" in info_theory.__all__
    assert "Absent" not in info_theory.__doc__
    for name in ("shannon_entropies", "residue_shannon_entropies"):
        assert name in cards.__all__ and callable(getattr(cards, name))

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()
                if p.kind != p.VAR_KEYWORD]

    E = inspect.Parameter.empty
    assert params(entropy.Q_from_assignments) == [
        ("assignments", E), ("n_states", None), ("lag_time", 1),
        ("builder", builders.normalize), ("prior_counts", None), ("device", 0)]
    assert params(entropy.relative_entropy_per_state) == [
        ("P", E), ("Q", None), ("assignments", None), ("weights", 1), ("state_subset", None),
        ("base", 2.0), ("device", 0)]
    assert params(entropy.relative_entropy_msm) == [
        ("P", E), ("Q", None), ("assignments", None), ("populations", None),
        ("state_subset", None), ("base", 2.0), ("device", 0)]
    assert params(entropy.kl_divergence) == [("P", E), ("Q", E), ("base", 2), ("device", 0)]
    assert params(entropy.js_divergence) == [("p", E), ("q", E), ("device", 0)]
    assert params(entropy.shannon_entropy) == [("p", E), ("normalize", True), ("device", 0)]
    assert params(entropy.energy_to_probability) == [("u", E), ("kT", 2.479)]
    for f in (entropy.relative_entropy_per_state, entropy.relative_entropy_msm):
        assert any(p.kind == p.VAR_KEYWORD for p in inspect.signature(f).parameters.values())


def test_bounds_are_what_their_docstrings_derive():
    assert ne.kl_bound(10, 2.0) == 14 * 2.0 ** -52 * 2.0
    assert ne.js_bound(10, 1.0, 3.0) == 0.5 * 15 * 2.0 ** -52 * 4.0
    assert ne.shannon_norm_bound(3, 1.0) == 7 * 2.0 ** -52 + 3 * 2.0 ** -52 * 2.0
    assert np.isinf(ne.kl_bound(3, np.inf))
