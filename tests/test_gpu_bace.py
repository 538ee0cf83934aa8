"""BACE on the device (enspara_amd/msm/bace.py, csrc/ek_msm_bace.hip) against
outputs of the real reference (tests/golden/bace_golden.npz, written by
tests/golden/make_bace_golden.py) and, for intermediate results, against the plain
numpy restatement of tests/_numpy_bace.py.  No expected value comes from a device
call.

Parity rule.  The device sums a pair's float64 terms in its own order, so it can
choose another pair than the reference only where two candidates lie within about
a float32 ulp (1.2e-7 relative) of each other.  Every case below therefore first
asserts, from the golden file, that each step's largest and second-largest matrix
entries are at least 1e-6 (8 float32 ulps) apart; under that condition (minX,
minY) of EVERY step and all labels must equal the reference's exactly.  Bayes
factors agree to rtol 1e-6: three float32 roundings of 6e-8 each plus one ulp from a
float64 sum that straddles a float32 rounding boundary; it is also the tolerance
of the reference's own test.  The paper's 9-state table has exact float32 ties
between symmetric pairs; it is exempt from the gap condition and pins the
first-index tie rule instead.

Shapes: n = 2 (one pair, no merge); the 9-state table; n = 24 with an all-zero
row and an under-sampled state (p = 2: prune on the device, kept != all, label
-1, the key shift); n = 70 (a row longer than a wave); n = 300 with about 20
non-zeros per row (longer than the workgroup, several arg-max blocks, work lists
of very different lengths, every merge down to 2); one-sided pairs; no merge."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]
import _numpy_bace as nb  # noqa: E402
from enspara_amd.exception import DataInvalid  # noqa: E402
from enspara_amd.msm import bace as B  # noqa: E402

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(HERE, "golden", "bace_golden.npz"))
GAP_CASES = ["n2", "n24_p2", "n24_nomerge", "n70", "n300_sparse", "asym16"]
MIN_GAP = 1e-6
RTOL = 1e-6


@functools.lru_cache(maxsize=None)
def _device(name, dmat_steps=0):
    return B._bace_full(G["C_" + name], int(G["nmacro_" + name]), dmat_steps=dmat_steps)


@functools.lru_cache(maxsize=None)
def _restated(name):
    return nb.bace_steps(G["C_" + name], int(G["nmacro_" + name]))


def _assert_matches_reference(name, bf, labels, records):
    p = int(G["p_" + name])
    n = G["C_" + name].shape[0]
    m = n - p
    nmacro = int(G["nmacro_" + name])
    rec = np.stack([records["x"], records["y"]], axis=1)
    print(name, "steps", len(rec), "first difference",
          np.flatnonzero((rec != G["rec_" + name]).any(axis=1))[:1])
    assert np.array_equal(records["status"], np.zeros(len(rec), dtype=np.int32))
    assert np.array_equal(rec, G["rec_" + name])
    # the reference's label keys are shifted by p, its factor keys are not
    assert sorted(labels) == sorted(int(k) - p for k in G["labk_" + name])
    assert sorted(labels) == list(range(nmacro, m))
    for k, want in zip(G["labk_" + name], G["lab_" + name]):
        assert np.array_equal(labels[int(k) - p], want), k
    assert sorted(bf) == sorted(int(k) for k in G["bfk_" + name])
    assert sorted(bf) == list(range(min(nmacro, m) - 1, m))
    got = np.array([bf[int(k)] for k in G["bfk_" + name]])
    print(name, "largest relative difference of a Bayes factor",
          np.abs(got / G["bfv_" + name] - 1).max())
    assert all(type(v) is np.float32 for v in bf.values())
    np.testing.assert_allclose(got, G["bfv_" + name], rtol=RTOL)


@pytest.mark.parametrize("name", GAP_CASES)
def test_every_merge_label_and_factor_is_the_references(name):
    gaps = G["gap_" + name]
    assert len(gaps) == len(G["rec_" + name]) and gaps.min() >= MIN_GAP, gaps.min()
    bf, labels, records, _ = _device(name)
    _assert_matches_reference(name, bf, labels, records)


def test_two_states_are_one_pair_and_no_merge():
    bf, labels, records, _ = _device("n2")
    assert int(G["p_n2"]) == 0 and len(records) == 1 and labels == {}
    assert list(bf) == [1] and (records["x"][0], records["y"][0]) == (0, 1)


def test_two_states_merged_leave_an_empty_matrix():
    """n_macrostates = 1: after the only merge no pair is left; that is the last
    record, and its factor is the reference's 1 / 0"""
    want = nb.bace_steps(G["C_n2"], 1)
    bf, labels = B.bace(G["C_n2"], 1)
    assert sorted(bf) == [0, 1] and bf[0] == np.float32(np.inf) == want["bayes_factors"][0]
    np.testing.assert_allclose(bf[1], want["bayes_factors"][1], rtol=RTOL)
    assert list(labels) == [1] and np.array_equal(labels[1], [0, 0])


def test_the_papers_nine_state_table():
    """the reference's TCOUNTS with its recorded Bayes factors and its seven label
    vectors; symmetric pairs tie exactly in float32, so this is the test of the
    first-index tie rule: every step's pair is the reference's"""
    bf, labels, records, _ = _device("tcounts9")
    exp = G["exp_bf_tcounts9"]
    got = np.array([bf[int(k)] for k in exp[:, 0]])
    print("tcounts9 factors", got, "pairs", list(zip(records["x"], records["y"])))
    np.testing.assert_allclose(got, exp[:, 1], rtol=RTOL)
    assert sorted(labels) == [int(k) for k in G["exp_labk_tcounts9"]] == list(range(2, 9))
    for k, want in zip(G["exp_labk_tcounts9"], G["exp_lab_tcounts9"]):
        assert np.array_equal(labels[int(k)], want), k
    _assert_matches_reference("tcounts9", bf, labels, records)


def test_pruned_states_shift_the_keys_and_keep_their_labels():
    bf, labels, records, _ = _device("n24_p2")
    kept = G["pk_n24_p2"]
    assert int(G["p_n24_p2"]) == 2 and len(kept) == 22
    assert sorted(labels) == list(range(2, 22)) and sorted(bf) == list(range(1, 22))
    for lab in labels.values():
        assert lab[5] == -1                       # the all-zero row
        assert lab[17] == lab[3]                  # the under-sampled state's neighbour
    assert not np.isin([5, 17], np.r_[records["x"], records["y"]]).any()
    # two macrostates besides -1.  Their labels are the reference's: its absorb does
    # not renumber for an all-zero row, so the labels above state 5 stay one higher
    # than a gapless numbering would make them (0 and 2 here, not 0 and 1)
    assert len(set(labels[2]) - {-1}) == 2
    assert np.array_equal(labels[2], G["lab_n24_p2"][-1]) and int(G["labk_n24_p2"][-1]) == 4


def test_no_merge_when_n_macrostates_is_the_number_of_kept_states():
    bf, labels, records, _ = _device("n24_nomerge")
    assert int(G["nmacro_n24_nomerge"]) == 22 and labels == {} and list(bf) == [21]
    bf2, labels2 = B.bace(G["C_n24_nomerge"], 1000)
    assert labels2 == {} and list(bf2) == [21] and bf2[21] == bf[21]


def test_one_sided_pairs_are_listed_from_their_side_only():
    c = G["pc_asym16"].astype(np.float64)
    one_sided = (c > 1) & ~(c.T > 1)
    assert one_sided.any() and int(G["p_asym16"]) == 0
    _, _, _, dmats = _device("asym16", 1)
    # the initial matrix holds the pairs s < d with c[s, d] > 1 and no others
    assert np.array_equal(dmats[0] != 0, np.triu(c > 1, 1))
    assert (np.triu(one_sided, 1) & (dmats[0] != 0)).any()
    assert (np.tril(one_sided, -1).T & (dmats[0] == 0)).any()


def test_the_whole_matrix_after_the_first_steps():
    """n = 70: the initial matrix and the one after each of the first three merges
    equal the restatement's -- zeros exactly (the pair lists), the rest to rtol
    1e-6 (the arithmetic)"""
    want = _restated("n70")
    _, _, records, dmats = _device("n70", 4)
    assert dmats.shape == (4, 70, 70)
    for step in range(4):
        ref = want["dmats"][step]
        print("step", step, "entries", int((ref != 0).sum()), "largest relative difference",
              np.abs(dmats[step][ref != 0] / ref[ref != 0] - 1).max())
        assert np.array_equal(dmats[step] == 0, ref == 0), step
        np.testing.assert_allclose(dmats[step], ref, rtol=RTOL)
        assert (records["x"][step], records["y"][step]) == want["records"][step][:2]


@pytest.mark.parametrize("name", ["prune3", "n24_p2", "n300_sparse"])
def test_prune_factors_on_the_device(name):
    C = G["C_" + name]
    gold = G["pd_" + name]
    assert np.abs(gold - nb.LOG3).min() > 1e-4 * nb.LOG3      # none near the threshold
    want = nb.prune_factors(C)
    np.testing.assert_allclose(want, gold, rtol=RTOL)
    got = B._prune_factors(np.ascontiguousarray(C, dtype=np.float64))
    print(name, "largest relative difference", np.abs(got / want - 1).max())
    assert got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=RTOL)
    pruned, labels, kept = B.baysean_prune(C)
    assert np.array_equal(kept, G["pk_" + name])
    assert np.array_equal(labels, G["pl_" + name])
    assert np.array_equal(pruned, G["pc_" + name])


def test_prune_at_another_factor():
    pruned, labels, kept = B.baysean_prune(G["C_prune3"], factor=1.3)
    assert np.abs(G["pd_prune3"] - 1.3).min() > 1e-4 * 1.3
    assert np.array_equal(pruned, G["pc_prune3f13"]) and pruned[1, 1] == 227
    assert np.array_equal(labels, G["pl_prune3f13"]) and list(kept) == [1]


@pytest.mark.parametrize("kind", [scipy.sparse.csr_matrix, scipy.sparse.coo_matrix])
def test_sparse_input_is_the_dense_result(kind):
    C = G["C_n24_p2"]
    bf, labels, _, _ = _device("n24_p2")
    bf2, labels2 = B.bace(kind(C), 2, chunk_size=7, n_procs=3)
    assert sorted(bf2) == sorted(bf) and all(bf2[k] == bf[k] for k in bf)
    assert sorted(labels2) == sorted(labels)
    assert all(np.array_equal(labels2[k], labels[k]) for k in labels)
    pruned, plabels, kept = B.baysean_prune(kind(C))
    assert type(pruned) is kind
    assert np.array_equal(pruned.toarray(), G["pc_n24_p2"])
    assert np.array_equal(plabels, G["pl_n24_p2"]) and np.array_equal(kept, G["pk_n24_p2"])


def test_disconnected_counts_raise_at_the_macrostates_reached():
    """a block of four states and a fifth with self-counts only: the pseudo-counts
    that merges write into the counts add up to 4 / 5 between the two at the most,
    never more than 1, so at 2 macrostates no pair is left"""
    C = np.zeros((5, 5))
    C[:4, :4] = [[300, 40, 25, 12], [38, 280, 30, 9], [22, 35, 310, 14], [10, 8, 15, 90]]
    C[4, 4] = 500
    want = nb.bace_steps(C, 1)
    assert want["m"] == 5 and want["stopped"] == 3
    with pytest.raises(DataInvalid, match="at 2 macrostates"):
        B.bace(C, 1)
    bf, labels = B.bace(C, 2)
    assert sorted(labels) == [2, 3, 4] and bf[1] == np.float32(np.inf)
    assert np.array_equal(labels[2], want["labels"][2])
    assert np.array_equal(labels[2], [0, 0, 0, 0, 1])
