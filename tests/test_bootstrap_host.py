"""msm.bootstrap without a GPU: the draws and the numpy model (tests/_numpy_bootstrap.py)
against the real reference's recorded outputs (tests/golden/bootstrap_golden.npz,
written by tests/golden/make_bootstrap_golden.py), the resampling units of ``chunk_by``,
and the argument errors, which are all raised before the device is touched."""
import os

import numpy as np
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import _numpy_bootstrap as nb
from enspara_amd.exception import DataInvalid
from enspara_amd.msm import bootstrap as bs

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "bootstrap_golden.npz"))


@pytest.fixture
def np_rng_state():
    state = np.random.get_state()
    yield
    np.random.set_state(state)


def test_module_is_exported_like_bace():
    from enspara_amd import msm
    assert msm.bootstrap is bs


@pytest.mark.parametrize("fx", ["a", "b"])
def test_draws_are_the_references(golden, fx, np_rng_state):
    want = golden[fx + "_draws"]
    seed = int(golden[fx + "_seed"])
    np.random.seed(seed)
    got = bs.resample_indices(want.shape[1], want.shape[0])
    assert got.dtype == np.int64
    assert_array_equal(got, want)
    # an int seed and a RandomState draw from that generator the same way
    assert_array_equal(bs.resample_indices(want.shape[1], want.shape[0], seed), want)
    assert_array_equal(bs.resample_indices(want.shape[1], want.shape[0],
                                           np.random.RandomState(seed)), want)


def test_model_agrees_with_the_golden(golden):
    units = nb.units_of(golden["a_assigns"])
    for r, idx in enumerate(golden["a_draws"]):
        counts, probs, eq = nb.transpose(nb.counts_of(units, idx, 1, True, 4))
        assert_array_equal(counts, golden["a_tcounts"][r])
        assert_allclose(probs, golden["a_tprobs"][r], rtol=1e-14, atol=0)
        assert_allclose(eq, golden["a_eq_probs"][r], rtol=1e-14, atol=0)
    units = nb.units_of(golden["b_assigns"])
    for r, idx in enumerate(golden["b_draws"]):
        counts, probs = nb.normalize(nb.counts_of(units, idx, 1, True, 5))
        assert_array_equal(counts, golden["b_tcounts"][r])
        assert_allclose(probs, golden["b_tprobs"][r], rtol=1e-14, atol=0)
    assert_allclose(golden["a_tprobs"].mean(axis=0), golden["a_mean_table"], rtol=0.2)


def test_generic_bootstrap_is_a_plain_loop(golden, np_rng_state):
    data = golden["a_assigns"]
    np.random.seed(int(golden["a_seed"]))
    got = bs.bootstrap(lambda d, scale: scale * d, data, 100, n_procs=3, scale=2)
    assert len(got) == 100
    for g, idx in zip(got, golden["a_draws"]):
        assert_array_equal(g, 2 * data[idx])
    ragged = [np.array([0, 1]), np.array([2]), np.array([3, 4, 5])]
    got = bs.bootstrap(lambda d: [len(u) for u in d], ragged, 7, random_state=5)
    idx = bs.resample_indices(3, 7, 5)
    assert got == [[len(ragged[i]) for i in row] for row in idx]


def test_chunk_by_units_on_ragged_input():
    ragged = [np.arange(7), np.arange(3), np.zeros(0, dtype=int), np.arange(6), np.arange(1)]
    want = [[0, 1, 2], [3, 4, 5], [6], [0, 1, 2], [0, 1, 2], [3, 4, 5], [0]]
    model = nb.units_of(ragged, 3)
    assert [u.tolist() for u in model] == want
    flat, lengths = bs._units_of(ragged, 3)
    assert lengths.dtype == np.int64
    assert lengths.tolist() == [len(u) for u in want]
    assert flat.tolist() == [v for u in want for v in u]
    picked = bs._Units(flat, lengths).pick([6, 2, 0])
    assert [p.tolist() for p in picked] == [want[6], want[2], want[0]]
    # no chunk_by: the trajectories themselves, empty ones included
    flat, lengths = bs._units_of(ragged, None)
    assert lengths.tolist() == [7, 3, 0, 6, 1]
    for bad in (0, -2, 2.5, True):
        with pytest.raises(DataInvalid):
            bs._units_of(ragged, bad)


def test_argument_errors_come_before_the_device():
    a = np.zeros((3, 10), dtype=np.int32)
    with pytest.raises(DataInvalid):                # non-integer data
        bs.bootstrap(len, a.astype(np.float64), 2)
    with pytest.raises(DataInvalid):
        bs.bootstrap(len, [np.zeros(3, dtype=int), np.zeros(3)], 2)
    with pytest.raises(DataInvalid):
        bs.bootstrap_counts(a.astype(np.float32), 1, n_trials=2)
    with pytest.raises(DataInvalid):                # neither n_trials nor indices
        bs.bootstrap_counts(a, 1)
    with pytest.raises(DataInvalid):
        bs.MSMs(a, 1, "transpose")
    for bad in ([[0, 3]], [[-1, 0]]):               # indices out of range
        with pytest.raises(DataInvalid):
            bs.bootstrap_counts(a, 1, indices=np.array(bad))
    for bad in (np.zeros(3, dtype=int), np.zeros((2, 0), dtype=int), np.zeros((1, 2))):
        with pytest.raises(DataInvalid):
            bs.bootstrap_counts(a, 1, indices=bad)
    with pytest.raises(DataInvalid):                # n_trials contradicts indices
        bs.bootstrap_counts(a, 1, n_trials=3, indices=np.zeros((2, 3), dtype=int))
    with pytest.raises(DataInvalid):
        bs.resample_indices(0, 3)
    with pytest.raises(DataInvalid):
        bs.resample_indices(3, 2, random_state="seed")


def test_overflow_guard():
    """n_draws x (longest unit) could reach 2^31: a cell of the int32 table could too"""
    a = np.zeros((2, 1 << 16), dtype=np.int32)
    with pytest.raises(DataInvalid, match="2\\^31"):
        bs.bootstrap_counts(a, 1, indices=np.zeros((1, 1 << 15), dtype=np.int64))
    # one draw fewer stays below it, and is refused for another reason further on
    with pytest.raises(DataInvalid, match="(?i)lag"):
        bs.bootstrap_counts(a, 0, indices=np.zeros((1, (1 << 15) - 1), dtype=np.int64))
