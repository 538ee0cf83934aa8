"""enspara_amd.info_theory on the device (csrc/ek_mi.hip): joint counts on the int8
matrix cores and the mutual information computed from them.

No expected value comes from a device call.  Counts are array_equal to the numpy
restatement (tests/_numpy_mi.py: a float64 product of one-hot matrices, itself held
equal to the real reference by tests/test_mi_host.py) and to the reference's own
outputs in tests/golden/mi_golden.npz.  Mutual information is held to
    |mi_dev - mi_np|[i, j] <= (n_x n_y + 4) 2^-52 S[i, j],   S = sum |terms|
(_numpy_mi.mi_bound: the device's log may differ from glibc's by one ulp, nothing
else may differ); every such test prints the largest ratio it sees.

Shapes (Fx, n_x, Fy, n_y): (5, 3, 4, 4) 15 x 16 rows, one short of a tile and a tile
boundary inside a feature; (6, 3, 7, 5) ragged and different on each side, which no
swapped row / column or A / B map passes; (1, 2, 1, 2) from 1-D input; (17, 1, 3, 255)
single-state features and the state limit; (40, 3, 40, 3) X with itself, 120 rows:
every wave of a workgroup at work, the last tiles ragged.  Frames: 1, 63, 64, 65
around the padding, and the chunk length and its neighbours.  The data is
asymmetric: feature i leans towards state i % n and one column of Y is a noisy copy
of a column of X."""
import functools
import os
import warnings

import numpy as np
import pytest

import _numpy_mi as nm
from enspara_amd import info_theory, ra
from enspara_amd.exception import (DataInvalid, InsufficientResourceError,
                                   PerformanceWarning)
from enspara_amd.info_theory import MI_CHUNK, JointCounts

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "mi_golden.npz"))

SHAPES = {"15x16": (5, 3, 4, 4), "18x35": (6, 3, 7, 5), "1d": (1, 2, 1, 2),
          "n255": (17, 1, 3, 255), "self40": (40, 3, 40, 3)}
FRAMES = [1, 63, 64, 65, MI_CHUNK - 1, MI_CHUNK, MI_CHUNK + 1]
INT_TYPES = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64,
             np.uint64]


@functools.lru_cache(maxsize=None)
def _data(shape):
    """(X, Y) of MI_CHUNK + 1 frames; tests take prefixes.  Y is None for self40."""
    fx, nx, fy, ny = SHAPES[shape]
    rng = np.random.RandomState(sum(SHAPES[shape]))
    X = nm.biased_codes(rng, MI_CHUNK + 1, fx, nx)
    if shape == "self40":
        X = nm.noisy_copy(rng, X, X, 7, 1, nx)
        Y = None
    else:
        Y = nm.noisy_copy(rng, nm.biased_codes(rng, MI_CHUNK + 1, fy, ny), X,
                          fy - 1, fx // 2, ny)
        Y.setflags(write=False)
    X.setflags(write=False)
    return X, Y


def _prefix(shape, frames):
    X, Y = _data(shape)
    X = X[:frames]
    Y = None if Y is None else Y[:frames]
    if shape == "1d":
        X, Y = X[:, 0], Y[:, 0]
    return X, Y


def test_chunk_length_is_the_one_the_frames_assume():
    assert MI_CHUNK == 16384 and MI_CHUNK % 64 == 0


# ---- counts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_counts_equal_the_restatement(shape, frames):
    fx, nx, fy, ny = SHAPES[shape]
    X, Y = _prefix(shape, frames)
    if Y is None:
        jc = info_theory.joint_counts(X, n_x=nx)
    else:
        jc = info_theory.joint_counts(X, Y, nx, ny)
    assert jc.dtype == np.uint32 and jc.shape == (fx, fy, nx, ny)
    want = nm.joint_counts(X, Y, nx, ny)
    assert np.array_equal(jc, want)
    assert np.all(jc.sum(axis=(2, 3)) == frames)


def test_default_state_numbers_are_max_plus_one():
    X, Y = _prefix("18x35", 500)
    jc = info_theory.joint_counts(X, Y)
    assert jc.shape == (6, 7, X.max() + 1, Y.max() + 1)
    assert np.array_equal(jc, nm.joint_counts(X, Y))
    with pytest.warns(UserWarning, match="n_y unused"):
        jc = info_theory.joint_counts(X, n_x=3, n_y=5)
    assert np.array_equal(jc, nm.joint_counts(X, None, 3))


def test_binning_table():
    """the reference's test_joint_count_binning"""
    trj1 = np.array([1] * 3 + [2] * 6 + [1] * 6)
    trj2 = np.array([1] * 9 + [0] * 3 + [2] * 3)
    expected = np.array([[0, 0, 0], [3, 3, 3], [0, 6, 0]])[None, None, ...]
    assert np.array_equal(info_theory.joint_counts(trj1, trj2), expected)
    assert np.array_equal(info_theory.joint_counts(trj1, trj2, 3, 3), expected)


def test_a_cell_above_2_to_16():
    rng = np.random.RandomState(3)
    X = nm.biased_codes(rng, 70000, 3, 3)
    X[:, 0] = 1
    jc = info_theory.joint_counts(X, n_x=3)
    assert jc[0, 0, 1, 1] == 70000 > 2 ** 16
    assert np.array_equal(jc, nm.joint_counts(X, None, 3))


def test_counts_200000_x_64_x_3():
    rng = np.random.RandomState(4)
    X = nm.biased_codes(rng, 200000, 64, 3, np.int8)
    Y = nm.noisy_copy(rng, nm.biased_codes(rng, 200000, 64, 3, np.int8), X, 63, 5, 3)
    jc = info_theory.joint_counts(X, Y, 3, 3)
    assert jc.dtype == np.uint32
    assert np.array_equal(jc, nm.joint_counts(X, Y, 3, 3))


def test_every_integer_dtype_gives_the_same_counts():
    X, Y = _prefix("18x35", 1000)
    want = nm.joint_counts(X, Y, 3, 5)
    for dt in INT_TYPES:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            jc = info_theory.joint_counts(X.astype(dt), Y.astype(dt), 3, 5)
        assert np.array_equal(jc, want), dt
    # (not C-contiguous: a transposed view)
    jc = info_theory.joint_counts(np.asfortranarray(X), np.asfortranarray(Y), 3, 5)
    assert np.array_equal(jc, want)


def test_mixed_dtypes_warn():
    X, Y = _prefix("18x35", 200)
    with pytest.warns(PerformanceWarning, match="uptyped"):
        jc = info_theory.joint_counts(X.astype(np.int8), Y.astype(np.uint32), 3, 5)
    assert np.array_equal(jc, nm.joint_counts(X, Y, 3, 5))


def test_invalid_codes_raise():
    X, Y = _prefix("18x35", 200)
    bad = X.copy()
    bad[17, 2] = 3
    with pytest.raises(DataInvalid, match=r"\[0, 3\)"):
        info_theory.joint_counts(bad, Y, 3, 5)
    with pytest.raises(DataInvalid, match=r"\[0, 5\)"):
        info_theory.joint_counts(X, np.where(Y == 4, 5, Y), 3, 5)
    bad = X.copy()
    bad[0, 0] = -1
    with pytest.raises(DataInvalid, match=r"\[0, 3\)"):
        info_theory.joint_counts(bad, Y, 3, 5)
    with pytest.raises(DataInvalid, match="255"):
        info_theory.joint_counts(X, Y, 3, 256)
    with pytest.raises(DataInvalid, match="length"):
        info_theory.joint_counts(X, Y[:-1], 3, 5)


def test_three_ragged_trajectories_equal_their_concatenation_and_the_golden():
    X, Y = G["rag_X"], G["rag_Y"]
    ends = np.cumsum(G["rag_lengths"])
    with JointCounts(6, 7, 3, 5) as jc:
        for lo, hi in zip(np.r_[0, ends[:-1]], ends):
            jc.add(X[lo:hi], Y[lo:hi])
        assert jc.n_observations == len(X)
        got = jc.counts()
    assert got.dtype == np.uint32
    assert np.array_equal(got, nm.joint_counts(X, Y, 3, 5))
    assert np.array_equal(got, G["rag_jc"])
    assert np.array_equal(info_theory.joint_counts(G["self_X"], n_x=3), G["self_jc"])


def test_counts_too_large_for_the_device():
    with pytest.raises(InsufficientResourceError, match="MiB"):
        JointCounts(30000, 30000, 255, 255)


# ---- mutual information ----------------------------------------------------------------------
def _check_mi(tag, mi, jc, nx, ny, also=None):
    want, S = nm.mutual_information(jc)
    assert mi.dtype == np.float64 and mi.shape == want.shape
    bound = nm.mi_bound(nx, ny, S)
    err = np.abs(mi - want)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
    print("%s: largest |mi_dev - mi_np| / bound = %.3f; %d of %d entries equal bit for bit"
          % (tag, ratio, int((mi == want).sum()), mi.size))
    assert np.all(err <= bound)
    if also is not None:
        assert np.all(np.abs(mi - also) <= bound)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_mutual_information_within_the_derived_bound(shape):
    fx, nx, fy, ny = SHAPES[shape]
    X, Y = _prefix(shape, 5000)
    want_jc = nm.joint_counts(X, Y, nx, ny)
    with JointCounts(fx, fy, nx, ny) as d:
        d.add(X if X.ndim == 2 else X[:, None], None if Y is None else
              (Y if Y.ndim == 2 else Y[:, None]))
        mi = info_theory.mutual_information(d)
        assert np.array_equal(d.counts(), want_jc)
    _check_mi(shape, mi, want_jc, nx, ny)
    # uploaded counts, of another integer type: the same bits
    assert np.array_equal(info_theory.mutual_information(want_jc.astype(np.int64)), mi)


def test_mutual_information_against_the_reference():
    _check_mi("rag", info_theory.mutual_information(G["rag_jc"]), G["rag_jc"], 3, 5,
              also=G["rag_mi"])
    mi = info_theory.mutual_information(G["self_jc"])
    _check_mi("self", mi, G["self_jc"], 3, 3, also=G["self_mi"])
    # X against itself: symmetric to rounding only, nothing is mirrored
    _, S = nm.mutual_information(G["self_jc"])
    assert np.all(np.abs(mi - mi.T) <= 2 * nm.mi_bound(3, 3, S))


def test_empty_pairs_and_zero_cells():
    jc = np.zeros((2, 2, 3, 3), dtype=np.uint32)
    jc[0, 1] = [[5, 0, 0], [0, 0, 7], [0, 0, 0]]
    jc[1, 0] = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    mi = info_theory.mutual_information(jc)
    assert mi[0, 0] == 0 and mi[1, 1] == 0
    _check_mi("zeros", mi, jc, 3, 3)
    with pytest.raises(DataInvalid, match="2D"):
        info_theory.mutual_information(jc[0, 0])


def test_mi_matrix_against_the_reference():
    X, Y = G["rag_X"], G["rag_Y"]
    ends = np.cumsum(G["rag_lengths"])
    Xs = [X[lo:hi] for lo, hi in zip(np.r_[0, ends[:-1]], ends)]
    Ys = [Y[lo:hi] for lo, hi in zip(np.r_[0, ends[:-1]], ends)]
    mi = info_theory.mi_matrix(Xs, Ys, 3, 5, normalize=False)
    _check_mi("rag mi_matrix", mi, G["rag_jc"], 3, 5, also=G["rag_mimat"])
    assert np.array_equal(mi, info_theory.mutual_information(G["rag_jc"]))
    # normalised: the same matrix over log(3)
    sX = G["self_X"]
    mi = info_theory.mi_matrix([sX], [sX], 3, 3)
    raw = info_theory.mi_matrix([sX], [sX], [3] * 24, [3] * 24, normalize=False)
    assert np.array_equal(mi, raw / np.log(3))
    _, S = nm.mutual_information(G["self_jc"])
    # (the two quotients round once each: half an ulp of at most S / log 3 apiece)
    assert np.all(np.abs(mi - G["self_mimat"]) <=
                  (nm.mi_bound(3, 3, S) + 2 * nm.U * S) / np.log(3))


def test_mi_matrix_list_array_and_ragged_give_the_same_bits():
    rng = np.random.RandomState(8)
    data = nm.biased_codes(rng, 3 * 700, 5, 4).reshape(3, 700, 5)
    as_list = [t for t in data]
    as_ra = ra.RaggedArray(array=data.reshape(-1, 5), lengths=[700, 700, 700])
    a = info_theory.mi_matrix(as_list, as_list, 4, 4)
    b = info_theory.mi_matrix(data, data, 4, 4)
    c = info_theory.mi_matrix(as_ra, as_ra, [4] * 5, [4] * 5)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    # other lengths, the same frames: the same counts, so the same bits
    other = ra.RaggedArray(array=data.reshape(-1, 5), lengths=[1, 1036, 1063])
    assert np.array_equal(info_theory.mi_matrix(other, other, 4, 4), a)
    with pytest.raises(DataInvalid, match="same number of features"):
        info_theory.mi_matrix([data[0], data[1][:, :4]], [data[0], data[1][:, :4]], 4, 4)


def _zero_mi(rng):
    return rng.randint(1, 5, (3, 10000, 5)), [5] * 5


def test_statistical_cases_of_the_reference():
    """test_symmetrical_mi_zero / _nonzero / asymmetrical_mi_zero / _nonzero with
    their own tolerances"""
    rng = np.random.RandomState(0)
    a, n = _zero_mi(rng)
    mi = info_theory.mi_matrix(a, a, n, n)
    np.testing.assert_allclose(np.diag(mi), 0.86114, atol=0.1)
    mi[np.diag_indices_from(mi)] = 0
    np.testing.assert_allclose(mi, 0, atol=1e-3)

    b, _ = _zero_mi(rng)
    mi = info_theory.mi_matrix(a, b, n, n)
    np.testing.assert_allclose(mi, 0, atol=1e-3)

    c = a.copy()
    c[:, :, -2] = c[:, :, -1]
    for n_states in (n, 5):
        mi = info_theory.mi_matrix(c, c, n_states, n_states)
        np.testing.assert_almost_equal(mi[-1, -2], 0.86114, decimal=3)
        np.testing.assert_almost_equal(mi[-2, -1], 0.86114, decimal=3)
        mi[-1, -2] = mi[-2, -1] = 0
        np.testing.assert_almost_equal(np.diag(mi), 0.86114, decimal=2)
        mi[np.diag_indices_from(mi)] = 0
        np.testing.assert_allclose(mi, 0, atol=1e-3)

    d = a.copy()
    d[:, :, 0] = b[:, :, 3]
    mi = info_theory.mi_matrix(d, b, n, n)
    np.testing.assert_almost_equal(mi[0, 3], 0.86114, decimal=3)
    mi[0, 3] = 0
    np.testing.assert_allclose(mi, 0, atol=1e-2)


def test_mi_matrix_serial_is_the_composition():
    rng = np.random.RandomState(9)
    a = [nm.biased_codes(rng, 300, 3, 3), nm.biased_codes(rng, 211, 3, 3)]
    serial = info_theory.mi_matrix_serial(a, a, [3] * 3, [3] * 3, normalize=False)
    full = info_theory.mi_matrix(a, a, 3, 3, normalize=False)
    iu = np.triu_indices(3)
    assert np.array_equal(serial[iu], full[iu])
    assert np.array_equal(serial, serial.T)


# ---- the handle ----------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits():
    X, Y = _prefix("18x35", MI_CHUNK + 1)
    runs = []
    for _ in range(2):
        with JointCounts(6, 7, 3, 5) as d:
            d.add(X, Y)
            runs.append((d.counts(), d.mutual_information()))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert np.array_equal(runs[0][1], runs[1][1])


def test_handle_open_add_read_add_read_close():
    X, Y = _prefix("18x35", 3000)
    d = JointCounts(6, 7, 3, 5)
    assert np.array_equal(d.counts(), np.zeros((6, 7, 3, 5), dtype=np.uint32))
    assert np.array_equal(d.mutual_information(), np.zeros((6, 7)))
    d.add(X[:1000], Y[:1000])
    first = d.counts()
    assert np.array_equal(first, nm.joint_counts(X[:1000], Y[:1000], 3, 5))
    mi1 = d.mutual_information()
    d.add(X[1000:], Y[1000:])
    assert np.array_equal(d.counts(), nm.joint_counts(X, Y, 3, 5))
    mi2 = d.mutual_information()
    assert not np.array_equal(mi1, mi2)
    assert np.array_equal(mi2, info_theory.mutual_information(nm.joint_counts(X, Y, 3, 5)))
    with pytest.raises(DataInvalid, match="do not fit"):
        d.add(X[:, :5], Y)
    with pytest.raises(DataInvalid, match="do not fit"):
        d.add(X)
    assert np.all(d.last_timing() >= 0)
    d.close()
    d.close()


def test_add_after_load_counts_on_from_the_fullest_pair():
    jc = np.zeros((1, 2, 2, 2), dtype=np.uint64)
    jc[0, 0] = [[2 ** 32 - 10, 0], [0, 4]]
    jc[0, 1] = [[1, 2], [3, 4]]
    x = np.zeros((5, 1), dtype=np.int64)
    y = np.ones((5, 2), dtype=np.int64)
    with JointCounts(1, 2, 2, 2) as d:
        d.load(jc)
        assert d.n_observations == 2 ** 32 - 6
        d.add(x, y)
        assert d.n_observations == 2 ** 32 - 1
        want = jc.copy()
        want[0, :, 0, 1] += 5
        assert np.array_equal(d.counts(), want)
        # one more observation would wrap a cell
        with pytest.raises(DataInvalid, match="2\\^32"):
            d.add(x[:1], y[:1])
        assert np.array_equal(d.counts(), want)
    jc[0, 1, 1, 1] = 2 ** 32 - 5        # a pair's sum at 2^32 + 1
    with pytest.raises(DataInvalid, match="2\\^32"):
        info_theory.mutual_information(jc)
