"""enspara_amd.cards on the device (csrc/ek_cards.hip): transition statistics, disorder
codes and the four mutual-information matrices.

No expected value comes from a device call.  Statistics and disorder codes are
array_equal to the numpy restatement (tests/_numpy_cards.py, itself held equal to the
real reference by tests/test_cards_host.py) and to the reference's own outputs in
tests/golden/cards_golden.npz; the matrices are within _numpy_mi.mi_bound (plus the one
rounding of the normalisation) of the restatement's, on counts that are array_equal.

Frames 1, 2, 63, 64, 65 lie around the padding to 64, CH - 1, CH, CH + 1, 2 CH + 1 and
3 CH + 5 around the scan's chunk (CH = SCAN_CHUNK): one, two, three and four chunks, the
last ones nearly empty.  Features 1, 63, 64, 65, 257: around the pack kernel's tile and
more than one workgroup of the combine kernel.  The per-feature intervals cycle through
short spans only, long spans only, none, all and exactly 2, so both decisions fall on
either side of every chunk boundary."""
import functools
import os

import numpy as np
import pytest

import _numpy_cards as nc
from enspara_amd import cards
from enspara_amd.cards import disorder
from enspara_amd.cards.disorder import MAX_FRAMES, CardsStates
from enspara_amd.exception import DataInvalid, InsufficientResourceError

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "cards_golden.npz"))
CH = cards.SCAN_CHUNK
FRAMES = [1, 2, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 1, 3 * CH + 5]
FEATURES = [1, 63, 64, 65, 257]
INTERVALS = [(1, 3), (4, MAX_FRAMES), (1, 0), (1, MAX_FRAMES), (2, 2)]


@functools.lru_cache(maxsize=None)
def _data():
    """[3 CH + 5, 257] codes of 3 states; feature j switches at the rate RATES[j % 4]"""
    rng = np.random.RandomState(41)
    T, F = FRAMES[-1], FEATURES[-1]
    rate = np.array([0.02, 0.2, 0.5, 0.9])[np.arange(F) % 4]
    jump = np.where(rng.rand(T, F) < rate[None, :], rng.randint(1, 3, (T, F)), 0)
    X = (np.cumsum(jump, axis=0) % 3).astype(np.int8)
    X.setflags(write=False)
    return X


def _intervals(F):
    lo = np.array([INTERVALS[j % 5][0] for j in range(F)], dtype=np.int64)
    hi = np.array([INTERVALS[j % 5][1] for j in range(F)], dtype=np.int64)
    return lo, hi


def _golden_trajs():
    ends = np.cumsum(G["rag_lengths"])
    return [G["rag_X"][lo:hi] for lo, hi in zip(np.r_[0, ends[:-1]], ends)]


def test_chunk_length():
    assert CH == 2048 and CH % 1024 == 0


# ---- statistics and disorder codes -------------------------------------------------------------
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("F", FEATURES)
def test_stats_and_disorder_codes_equal_the_restatement(F, frames):
    X = _data()[:frames, :F]
    lo, hi = _intervals(F)
    with CardsStates(F, 3) as d:
        d.add(X.astype(np.uint8))
        st = d.stats()
        assert st.dtype == np.int64 and st.shape == (1, F, 4)
        assert np.array_equal(st[0], nc.stats(X))
        D = d.disorder(lo, hi).disorder_codes(0)
    assert D.dtype == np.uint8 and D.shape == X.shape
    want = nc.disorder_codes_from_interval(X, lo, hi)
    assert np.array_equal(D, want)
    if frames > 2 * CH and F >= 5:
        # both decisions on either side of the first chunk boundary, in some feature
        near = want[CH - 40:CH + 40]
        assert near[:40].any() and near[40:].any() and not near[:40].all() and not near[40:].all()


def _hand_built():
    T = 3 * CH + 5
    X = np.zeros((T, 8), dtype=np.uint8)
    X[CH + 8:, 1] = 1                               # exactly one transition, at CH + 7
    X[6:6 + 2 * CH + 100, 2] = 2                    # two, 2 CH + 100 apart, nothing between
    X[CH:CH + 4, 3] = 1                             # at CH - 1 (its pair straddles a chunk), CH + 3
    X[T - 9:T - 1, 4] = 1                           # at T - 10 and at T - 2
    X[:, 5] = np.arange(T) % 2                      # every frame
    X[CH:2 * CH, 6] = 2                             # at CH - 1 and 2 CH - 1: a whole chunk
    X[0, 7] = 1                                     # at frame 0 (a waiting time of 0) ...
    X[2 * CH + 1:, 7] = 2                           # ... and at 2 CH
    return X


def test_hand_built_columns():
    X = _hand_built()
    T = len(X)
    want = nc.stats(X)
    assert [list(nc.transition_times(X[:, j])) for j in (0, 1, 2, 3, 4, 6, 7)] == [
        [], [CH + 7], [5, 5 + 2 * CH + 100], [CH - 1, CH + 3], [T - 10, T - 2],
        [CH - 1, 2 * CH - 1], [0, 2 * CH]]
    assert want[5, 0] == T - 1
    with CardsStates(8, 3) as d:
        d.add(X)
        assert np.array_equal(d.stats()[0], want)
        for lo, hi in ((1, MAX_FRAMES), (1, 4), (5, MAX_FRAMES), (CH, 2 * CH), (1, 0)):
            lo, hi = np.full(8, lo, dtype=np.int64), np.full(8, hi, dtype=np.int64)
            D = d.disorder(lo, hi).disorder_codes(0)
            assert np.array_equal(D, nc.disorder_codes_from_interval(X, lo, hi)), (lo[0], hi[0])
        # all spans: column 2 is disordered across two whole chunks without a transition,
        # and nothing before a first or from a last transition on is
        D = d.disorder(np.ones(8, dtype=np.int64),
                       np.full(8, MAX_FRAMES, dtype=np.int64)).disorder_codes(0)
    assert D[5:5 + 2 * CH + 100, 2].all() and not D[:5, 2].any() and not D[5 + 2 * CH + 100:, 2].any()
    assert not D[:, 0].any() and not D[:, 1].any()
    assert D[CH - 1:CH + 3, 3].all() and D[:, 3].sum() == 4
    assert D[:T - 2, 5].all() and not D[T - 2:, 5].any()


def test_several_trajectories_keep_their_own_carries():
    X = _data()
    parts = [X[:CH + 1, :65], X[CH + 1:CH + 3, :65], X[CH + 3:, :65], X[:1, :65]]
    lo, hi = _intervals(65)
    with CardsStates(65, 3) as d:
        for p in parts:
            d.add(p.astype(np.uint8))
        st = d.stats()
        d.disorder(lo, hi)
        for i, p in enumerate(parts):
            assert np.array_equal(st[i], nc.stats(p))
            assert np.array_equal(d.disorder_codes(i),
                                  nc.disorder_codes_from_interval(p, lo, hi))


def test_statistics_and_assignment_against_the_reference():
    trajs = _golden_trajs()
    tt, mean_ord, mean_dis = disorder.transition_stats(trajs)
    assert np.array_equal(mean_ord, G["rag_mean_ord"])
    assert np.array_equal(mean_dis, G["rag_mean_dis"])
    flat = np.concatenate([np.concatenate(row) for row in tt])
    assert np.array_equal(flat, G["rag_tt"])
    assert np.array_equal([[len(c) for c in row] for row in tt], G["rag_tt_counts"])
    with CardsStates(12, 3) as d:
        for X in trajs:
            d.add(X.astype(np.uint8))
        times = np.stack(disorder.times_from_stats(d.stats()), axis=-1)
    assert np.array_equal(times, G["rag_times"])
    Ds, two = disorder.assign_order_disorder(trajs)
    assert two.dtype == np.int16 and np.array_equal(two, np.full(12, 2))
    assert all(D.dtype == np.int16 for D in Ds)
    assert np.array_equal(np.concatenate(Ds), G["rag_D"])
    assert [len(D) for D in Ds] == list(G["rag_lengths"])


# ---- matrices ------------------------------------------------------------------------------------
def _check_matrices(tag, got, want, bounds):
    for k, name in enumerate(("S-S", "D-D", "S-D", "D-S")):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape
        err = np.abs(got[k] - want[k])
        b = bounds[k]
        ratio = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0)))
        print("%s %s: largest |mi_dev - mi_np| / bound = %.3f; %d of %d entries equal bit for "
              "bit" % (tag, name, ratio, int((got[k] == want[k]).sum()), err.size))
        assert np.all(err <= b), name


def test_cards_matrices_on_the_golden_input():
    trajs = _golden_trajs()
    n = np.full(12, 3)
    want, bounds, Ds, jcs = nc.cards_matrices(trajs, n)
    got = cards.cards_matrices(trajs, n)
    assert len(got) == 4
    _check_matrices("golden", got, want, bounds)
    # the real reference's matrices (its D-D divided by a float32 log 2: _numpy_cards)
    ref = [G["rag_ss"], nc.dd_in_float64(G["rag_dd"]), G["rag_sd"], G["rag_ds"]]
    bounds[1] = bounds[1] + 2 * nc.nm.U * np.abs(ref[1])
    _check_matrices("reference", got, ref, bounds)
    # the codes and the counts behind them: exact
    with CardsStates(12, 3) as d:
        for X in trajs:
            d.add(X.astype(np.uint8))
        d.disorder(*disorder.disorder_interval(*d.mean_times()))
        for i, D in enumerate(Ds):
            assert np.array_equal(d.disorder_codes(i), D)
        raw = d.matrices()
        for k in range(4):
            jc = d.counts(k)
            assert jc.dtype == np.uint32 and np.array_equal(jc, jcs[k]), k
        assert np.array_equal(d.counts(3), d.counts(2).transpose(1, 0, 3, 2))
        assert np.all(d.last_timing() >= 0)
    assert np.array_equal(raw[0] / np.log(3), got[0])
    assert np.array_equal(raw[2] / np.log(2), got[2])


def test_state_numbers_per_feature_and_two_runs():
    X = _data()[:CH + 70, :7]
    X = np.where(np.arange(7)[None, :] < 3, X % 2, X)        # features 0 .. 2 have two states
    n = np.array([2, 2, 2, 3, 3, 3, 3])
    want, bounds, _, _ = nc.cards_matrices([X[:CH + 1], X[CH + 1:]], n)
    got = cards.cards_matrices([X[:CH + 1], X[CH + 1:]], n)
    _check_matrices("mixed", got, want, bounds)
    again = cards.cards_matrices([X[:CH + 1], X[CH + 1:]], n, n_procs=8)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


# ---- end to end ----------------------------------------------------------------------------------
def test_cards_end_to_end_from_coordinates():
    rng = np.random.RandomState(43)
    kind = np.array([0] * 4 + [1] * 4 + [2] * 8)
    bounds_, shifts = [nc.PHI, nc.PSI, nc.CHI], [0, 100, 0]
    trajs, states = [], []
    for frames in (CH + 1, 65):
        # busy and calm stretches, so that there is disorder to assign
        step = np.where((np.arange(frames) // 150) % 3 == 0, 70.0, 2.0)[:, None]
        xyz, quads, deg = nc.safe_trajectory(rng, frames, kind, bounds_, shifts, 15, step=step)
        trajs.append(xyz)
        states.append(nc.rotamer_states(deg, kind, bounds_, shifts, 15))
    dihedrals = {"phi": quads[:4], "psi": quads[4:8], "chi": quads[8:]}
    n = np.array([2] * 8 + [3] * 8)
    want, bounds, Ds, _ = nc.cards_matrices(states, n)
    assert 0.05 < np.concatenate(Ds).mean() < 0.95

    class Traj(object):
        def __init__(self, xyz):
            self.xyz = xyz

    got = cards.cards((Traj(x) for x in trajs), dihedrals, buffer_width=15, n_procs=2)
    assert len(got) == 5 and np.array_equal(got[4], quads)
    _check_matrices("end to end", got[:4], want, bounds)
    f = cards.RotamerFeaturizer(dihedrals).fit(trajs)
    assert np.array_equal(f.n_feature_states_, n) and np.array_equal(f.atom_indices_, quads)
    for a, b in zip(f.feature_trajectories_, states):
        assert a.dtype == np.int16 and np.array_equal(a, b)


# ---- the handle ----------------------------------------------------------------------------------
def test_counts_too_large_for_the_device():
    with pytest.raises(InsufficientResourceError, match="MiB"):
        CardsStates(30000, 255)


def test_handle_as_context_manager_and_double_close():
    X = _data()[:300, :5].astype(np.uint8)
    with CardsStates(5, 3) as d:
        d.add(X)
        assert d.lengths == [300]
        with pytest.raises(DataInvalid, match="does not fit"):
            d.add(X[:, :4])
    assert d._h is None
    d.close()
    d = CardsStates(5, 3)
    d.add(X)
    assert np.array_equal(d.stats()[0], nc.stats(X))
    d.close()
    d.close()
