"""The host side of BACE (enspara_amd/msm/bace.py) and the numpy restatement the
device tests lean on (tests/_numpy_bace.py), without a device.

The restatement must reproduce the real reference's outputs
(tests/golden/bace_golden.npz): pairs and labels exactly, Bayes factors to rtol
1e-6.  `absorb`, the prune's host logic, the key convention with pruned states
and the input checks are the package's own code; where a device call would be
needed (the prune's factors) the restatement's are put in its place."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]
import _numpy_bace as nb  # noqa: E402
from enspara_amd import msm  # noqa: E402
from enspara_amd.exception import DataInvalid  # noqa: E402
from enspara_amd.msm import bace as B  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "bace_golden.npz"))
CASES = [str(c) for c in G["cases"]]
SPARSE_TYPES = [np.array, scipy.sparse.csr_matrix, scipy.sparse.coo_matrix,
                scipy.sparse.lil_matrix, scipy.sparse.csc_matrix, scipy.sparse.dia_matrix]
T3 = np.array([[100, 10, 1], [10, 100, 0], [1, 0, 5]])
T3_PRUNED = np.array([[107, 10, 0], [10, 100, 0], [0, 0, 0]])


@pytest.fixture
def host_prune(monkeypatch):
    """the prune's factors from the restatement instead of the device"""
    monkeypatch.setattr(B, "_prune_factors",
                        lambda dense, device=0: nb.prune_factors(dense))


def _dense(a):
    return a.toarray() if scipy.sparse.issparse(a) else np.asarray(a)


def test_the_module_is_exported_with_the_references_names():
    assert msm.bace is B
    for name in ("bace", "baysean_prune", "absorb"):
        assert callable(getattr(B, name))


def test_golden_file_holds_the_cases_and_their_gaps():
    assert set(CASES) == {"tcounts9", "n2", "n24_p2", "n24_nomerge", "n70",
                          "n300_sparse", "asym16"}
    for name in CASES:
        assert G["C_" + name].shape[0] <= 300
        assert len(G["gap_" + name]) == len(G["rec_" + name]) == len(G["bfk_" + name])
        if name != "tcounts9":
            assert G["gap_" + name].min() >= 1e-6, name
    assert G["gap_tcounts9"].min() == 0             # the paper's table ties exactly


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    p = int(G["p_" + name])
    r = nb.bace_steps(G["C_" + name], int(G["nmacro_" + name]))
    assert r["stopped"] is None and r["m"] == G["C_" + name].shape[0] - p
    assert np.array_equal(np.array([x[:2] for x in r["records"]]).reshape(-1, 2),
                          G["rec_" + name])
    assert sorted(r["labels"]) == sorted(int(k) - p for k in G["labk_" + name])
    for k, want in zip(G["labk_" + name], G["lab_" + name]):
        assert np.array_equal(r["labels"][int(k) - p], want), k
    got = np.array([r["bayes_factors"][int(k)] for k in G["bfk_" + name]])
    np.testing.assert_allclose(got, G["bfv_" + name], rtol=1e-6)
    np.testing.assert_allclose(r["prune_d"], G["pd_" + name], rtol=1e-6)
    assert np.array_equal(r["kept"], G["pk_" + name])
    gaps = np.array([nb.gap(d) for d in r["dmats"]])
    # (entries are float32: a gap moves by a few 1.2e-7 at the most)
    np.testing.assert_allclose(gaps, G["gap_" + name], rtol=0, atol=5e-7)


def test_restatement_reproduces_the_recorded_table():
    r = nb.bace_steps(G["C_tcounts9"], 2)
    exp = G["exp_bf_tcounts9"]
    np.testing.assert_allclose([r["bayes_factors"][int(k)] for k in exp[:, 0]], exp[:, 1],
                               rtol=1e-6)
    for k, want in zip(G["exp_labk_tcounts9"], G["exp_lab_tcounts9"]):
        assert np.array_equal(r["labels"][int(k)], want)


@pytest.mark.parametrize("kind", [np.array, scipy.sparse.csr_matrix])
def test_absorb_the_references_table(kind):
    c, labels = B.absorb(kind(T3), [2])
    assert np.array_equal(_dense(c), T3_PRUNED)
    assert np.array_equal(labels, [0, 1, 0])
    assert np.array_equal(T3, [[100, 10, 1], [10, 100, 0], [1, 0, 5]])   # not in place


@pytest.mark.parametrize("kind", [np.array, scipy.sparse.csr_matrix])
def test_absorb_an_island_raises(kind):
    island = np.array([[100, 10, 0], [10, 100, 0], [0, 0, 5]])
    with pytest.raises(DataInvalid, match="disconnected"):
        B.absorb(kind(island), [2])


def test_absorb_matches_the_restatement_on_a_chain_of_absorptions():
    C = nb.block_chain_counts(12, 2, 800, seed=5)
    order = [7, 2, 3, 9]
    c, labels = B.absorb(C, order)
    c2, labels2 = nb.absorb(C, order)
    assert np.array_equal(c, c2) and np.array_equal(labels, labels2)
    assert c.sum() == C.sum() and not c[order].any() and not c[:, order].any()
    assert sorted(set(labels)) == list(range(8))


@pytest.mark.parametrize("kind", SPARSE_TYPES)
def test_prune_host_logic_in_every_type(host_prune, kind):
    pruned, labels, kept = B.baysean_prune(kind(T3), n_procs=4)
    if kind is not np.array:
        assert type(pruned) is kind
    assert np.array_equal(_dense(pruned), T3_PRUNED)
    assert np.array_equal(labels, [0, 1, 0]) and np.array_equal(kept, [0, 1])
    assert np.array_equal(_dense(pruned), G["pc_prune3"])
    # an empty row is labelled -1 and left alone
    T4 = np.zeros((4, 4), dtype=int)
    T4[:3, :3] = T3
    pruned, labels, kept = B.baysean_prune(kind(T4), n_procs=4)
    want = np.zeros((4, 4), dtype=int)
    want[:3, :3] = T3_PRUNED
    assert np.array_equal(_dense(pruned), want)
    assert np.array_equal(labels, [0, 1, 0, -1]) and np.array_equal(kept, [0, 1])


def test_prune_at_factor_1_3(host_prune):
    pruned, labels, kept = B.baysean_prune(T3, factor=1.3)
    want = np.zeros((3, 3))
    want[1, 1] = 227
    assert np.array_equal(pruned, want) and np.array_equal(pruned, G["pc_prune3f13"])
    assert np.array_equal(labels, [0, 0, 0]) and np.array_equal(kept, [1])
    assert pruned.dtype == T3.dtype                 # the type the counts came in


def _records(r):
    rec = np.zeros(len(r["records"]), dtype=B._RECORD)
    for i, (x, y, bf) in enumerate(r["records"]):
        rec[i] = (x, y, bf, 1 if bf == np.inf else 0)
    return rec


def test_key_convention_with_pruned_states():
    """p = 2 of n = 24: m = 22 kept; labels[21 .. 2], bayes_factors[21 .. 1]; the
    reference's labels[k + 2]"""
    name = "n24_p2"
    r = nb.bace_steps(G["C_" + name], 2)
    _, state_map, kept, _ = nb.prune(G["C_" + name].astype(np.float64))
    bf, labels = B._results_from_records(state_map, len(kept), 2, _records(r))
    assert sorted(labels) == list(range(2, 22)) and sorted(bf) == list(range(1, 22))
    assert [int(k) for k in G["labk_" + name]] == list(range(23, 3, -1))
    for k, want in zip(G["labk_" + name], G["lab_" + name]):
        assert np.array_equal(labels[int(k) - 2], want)
    assert all(lab[5] == -1 for lab in labels.values())
    assert all(bf[int(k)] == v for k, v in zip(G["bfk_" + name], G["bfv_" + name]))
    assert state_map[5] == -1                       # the argument is not written to


def test_no_pair_left_raises_and_names_the_macrostates_reached():
    rec = np.zeros(4, dtype=B._RECORD)
    rec[0] = (0, 1, 2.0, 0)
    rec[1] = (2, 3, 3.0, 0)
    rec[2] = (0, 0, np.inf, 1)          # two merges done: 2 of 4 states left, no pair
    rec[3] = (-1, -1, 0.0, 2)
    with pytest.raises(DataInvalid, match="at 2 macrostates"):
        B._results_from_records(np.arange(4), 4, 1, rec)
    bf, labels = B._results_from_records(np.arange(4), 4, 2, rec[:3])
    assert np.array_equal(labels[3], [0, 0, 1, 2]) and np.array_equal(labels[2], [0, 0, 1, 1])
    assert bf[1] == np.inf and sorted(bf) == [1, 2, 3]


@pytest.mark.parametrize("bad", [
    np.ones((3, 4)), np.ones(4), np.ones((1, 1)),
    np.array([[1., np.nan], [2., 3.]]), np.array([[1., np.inf], [2., 3.]]),
    np.array([[1., -1.], [2., 3.]])])
def test_input_checks(bad):
    with pytest.raises(DataInvalid):
        B.bace(bad, 2)
    with pytest.raises(DataInvalid):
        B.baysean_prune(bad)
    with pytest.raises(DataInvalid):
        B.bace(scipy.sparse.csr_matrix(np.atleast_2d(bad)), 2)
