"""enspara_amd.cards and enspara_amd.geometry.rotamer without a device: the numpy
restatement the GPU tests expect from (tests/_numpy_cards.py) against the real
reference's outputs (tests/golden/cards_golden.npz, made by
tests/golden/make_cards_golden.py), the interval rule against the reference's
likelihood-ratio expression, every validator (they raise before any device call: this
file runs where there is no device), the host helpers and `transitions`."""
import os

import numpy as np
import pytest

import _numpy_cards as nc
from enspara_amd import _lib, cards, ra
from enspara_amd.cards import disorder
from enspara_amd.exception import DataInvalid
from enspara_amd.geometry import rotamer

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "cards_golden.npz"))
WIDTHS = (0, 15, 15.5, 60)
BOUNDS = [nc.PHI, nc.PSI, nc.CHI]
SHIFTS = [0, 100, 0]


def _trajs():
    ends = np.cumsum(G["rag_lengths"])
    return [G["rag_X"][lo:hi] for lo, hi in zip(np.r_[0, ends[:-1]], ends)]


def _golden_tt():
    flat, counts = G["rag_tt"], G["rag_tt_counts"]
    ends = np.cumsum(counts.ravel()).reshape(counts.shape)
    return [[flat[ends[i, j] - counts[i, j]:ends[i, j]] for j in range(counts.shape[1])]
            for i in range(counts.shape[0])]


# ---- the restatement against the reference ------------------------------------------------
def test_restatement_statistics_equal_the_golden():
    trajs, tt = _trajs(), _golden_tt()
    mean_ord, mean_dis = nc.mean_times(trajs)
    assert np.array_equal(mean_ord, G["rag_mean_ord"])
    assert np.array_equal(mean_dis, G["rag_mean_dis"])
    for i, X in enumerate(trajs):
        st = nc.stats(X)
        for j in range(X.shape[1]):
            assert np.array_equal(nc.transition_times(X[:, j]), tt[i][j])
            assert nc.ord_disord_times(tt[i][j]) == tuple(G["rag_times"][i, j])
            want = (len(tt[i][j]), tt[i][j][0], tt[i][j][-1]) if len(tt[i][j]) else (0, -1, -1)
            assert tuple(st[j, :3]) == want
    # the golden holds all three cases
    assert (G["rag_tt_counts"].sum(axis=0) == 0).any()
    assert ((mean_ord < mean_dis) & (mean_dis > 0)).any()
    assert ((mean_ord > mean_dis) & (mean_dis > 0)).any()


def test_restatement_disorder_codes_equal_the_golden():
    trajs = _trajs()
    D = np.concatenate([nc.disorder_codes(X, G["rag_mean_ord"], G["rag_mean_dis"])
                        for X in trajs])
    assert np.array_equal(D, G["rag_D"])
    assert 0.05 < D.mean() < 0.95


def test_restatement_matrices_within_the_bound_of_the_golden():
    got, bounds, _, _ = nc.cards_matrices(_trajs(), np.full(12, 3))
    for k, key in enumerate(("rag_ss", "rag_dd", "rag_sd", "rag_ds")):
        want, b = G[key], bounds[k]
        if key == "rag_dd":
            want = nc.dd_in_float64(want)
            b = b + 2 * nc.nm.U * np.abs(want)
        assert np.all(np.abs(got[k] - want) <= b), key


@pytest.mark.parametrize("series", ["rot_angles", "rot_gates"])
def test_restatement_rotamer_states_equal_the_golden(series):
    A = G[series]
    want = G["rot_states" if series == "rot_angles" else "rot_gate_states"]
    for w, width in enumerate(WIDTHS):
        got = nc.rotamer_states(A, [0, 1, 2], BOUNDS, SHIFTS, width)
        assert np.array_equal(got.T, want[:, w]), width
    if series == "rot_gates":       # the psi column's shifted values sit on the gates too
        assert set(nc.shifted(A[:, 1], 100).tolist()) == set(np.float32(nc.ON_GATES).tolist())


# ---- the device's integers and intervals, on the host ----------------------------------------
def test_times_from_stats_are_the_reference_times():
    for i, X in enumerate(_trajs()):
        o, no, d, nd = disorder.times_from_stats(nc.stats(X))
        got = np.stack([o, no, d, nd], axis=1)
        assert np.array_equal(got, G["rag_times"][i])


def test_intervals_rebuild_the_golden_disorder_codes():
    lo, hi = disorder.disorder_interval(G["rag_mean_ord"], G["rag_mean_dis"])
    assert lo.dtype == np.int64 and hi.dtype == np.int64
    D = np.concatenate([nc.disorder_codes_from_interval(X, lo, hi) for X in _trajs()])
    assert np.array_equal(D, G["rag_D"])
    # a feature without transitions: an empty interval; one with ord < dis: a lower bound
    assert (hi < lo)[G["rag_tt_counts"].sum(axis=0) == 0].all()
    lower = (G["rag_mean_ord"] < G["rag_mean_dis"]) & (G["rag_mean_dis"] > 0)
    assert np.all(lo[lower] > 1) and np.all(hi[lower] == disorder.MAX_FRAMES)


def test_interval_rule_equals_the_reference_expression_for_every_span():
    rng = np.random.RandomState(5)
    o = np.concatenate([rng.uniform(0.5, 400, 150), rng.uniform(1, 30, 150),
                        [5.0, 1.0, 1e-3, 1e-300, 3.0, 1e5, 0.0, np.nan, 7.0, 2.5, 100.0,
                         1e9]])
    d = np.concatenate([rng.uniform(0.01, 30, 150), rng.uniform(1, 400, 150),
                        [5.0, 1.0, 1e-2, 1e-299, 1e-3, 0.3, 0.0, 2.0, np.nan, 0.999,
                         100.001, 1e6]])
    lo, hi = disorder.disorder_interval(o, d)
    spans = np.arange(1, 20001, dtype=np.int64)
    kinds = set()
    for k in range(len(o)):
        want = nc.likelihood(o[k], d[k], spans) >= 3.0
        got = (spans >= lo[k]) & (spans <= hi[k])
        assert np.array_equal(got, want), (o[k], d[k], lo[k], hi[k])
        kinds.add((bool(want.any()), bool(want.all()), bool(o[k] < d[k])))
    assert len(kinds) == 6      # empty, full and proper intervals, ord above and below dis
    assert np.isinf(nc.likelihood(1e-3, 1e-2, spans)).any()    # an overflow to inf is among them
    e = o == d
    assert np.all(hi[e] < lo[e])


# ---- validators: DataInvalid before any device call ------------------------------------------
def test_rotamer_validators():
    a = np.array([10.0, 200.0, 300.0], dtype=np.float32)
    for width in (-1, 180, 400):
        with pytest.raises(DataInvalid, match="Buffer width"):
            rotamer.rotamers(a, nc.PHI, width)
    with pytest.raises(DataInvalid, match="Buffer width"):
        rotamer.rotamers(a, nc.CHI, 120)
    with pytest.raises(DataInvalid, match="start with 0"):
        rotamer.rotamers(a, [10, 180, 360])
    with pytest.raises(DataInvalid, match="end with 360"):
        rotamer.rotamers(a, [0, 180, 350])
    with pytest.raises(DataInvalid, match="increase"):
        rotamer.rotamers(a, [0, 200, 100, 360])
    with pytest.raises(DataInvalid, match="at most 8"):
        rotamer.rotamers(a, list(range(0, 361, 36)), 1)
    for bad in (360.0, -0.5, np.nan, np.inf):
        with pytest.raises(DataInvalid, match=r"\[0, 360\)"):
            rotamer.rotamers(np.array([10.0, bad], dtype=np.float32), nc.PHI)
    with pytest.raises(DataInvalid, match="frames"):
        rotamer.rotamers(np.zeros((2, 2, 2), dtype=np.float32), nc.PHI)
    with pytest.raises(DataInvalid, match="kinds must lie"):
        rotamer.rotamer_states(a[:, None], [1], [nc.PHI], [0])


def test_coordinate_validators():
    xyz = np.random.RandomState(0).rand(5, 6, 3).astype(np.float32)
    q = np.array([[0, 1, 2, 3]])
    bad = xyz.copy()
    bad[2, 1, 0] = np.nan
    with pytest.raises(DataInvalid, match="finite"):
        rotamer.dihedral_angles(bad, q)
    with pytest.raises(DataInvalid, match=r"\[0, 6\)"):
        rotamer.dihedral_angles(xyz, [[0, 1, 2, 6]])
    with pytest.raises(DataInvalid, match=r"\[0, 6\)"):
        rotamer.phi_rotamers(xyz, [[-1, 1, 2, 3]])
    with pytest.raises(DataInvalid, match=r"\[n, 4\]"):
        rotamer.dihedral_angles(xyz, [[0, 1, 2]])
    with pytest.raises(DataInvalid, match="atoms, 3"):
        rotamer.dihedral_angles(xyz[:, :, :2], q)
    with pytest.raises(DataInvalid, match="`dihedrals` is required"):
        cards.cards([xyz])
    with pytest.raises(DataInvalid, match="'phi', 'psi', 'chi'"):
        cards.cards([xyz], {"omega": q})
    with pytest.raises(DataInvalid, match="`dihedrals` is required"):
        rotamer.all_rotamers(xyz, None)

    class Traj(object):
        pass
    t = Traj()
    t.xyz = bad
    with pytest.raises(DataInvalid, match="finite"):      # (an object with .xyz is read)
        cards.cards([t], {"phi": q})


def test_state_code_validators():
    X = np.zeros((10, 3), dtype=np.int64)
    with pytest.raises(DataInvalid, match=r"\[0, n\)"):
        cards.cards_matrices([np.where(X == 0, 3, 0)], [3, 3, 3])
    with pytest.raises(DataInvalid, match=r"\[0, n\)"):
        cards.cards_matrices([X - 1], [3, 3, 3])
    per_feature = X.copy()
    per_feature[4, 0] = 2       # feature 0 has two states, feature 2 three
    with pytest.raises(DataInvalid, match=r"\[0, n\)"):
        cards.cards_matrices([per_feature], [2, 2, 3])
    with pytest.raises(DataInvalid, match="differs between trajectories"):
        cards.cards_matrices([X, X[:, :2]], [3, 3, 3])
    with pytest.raises(DataInvalid, match="does not fit"):
        cards.cards_matrices([X], [3, 3])
    with pytest.raises(DataInvalid, match="state indices"):
        cards.cards_matrices([X.astype(np.float64)], [3, 3, 3])
    with pytest.raises(DataInvalid, match="1 to 255"):
        cards.cards_matrices([X], [3, 3, 256])
    with pytest.raises(DataInvalid, match="No trajectories"):
        cards.cards_matrices([], [3])
    with pytest.raises(DataInvalid, match="frames"):
        cards.cards_matrices([X[:0]], [3, 3, 3])
    with pytest.raises(DataInvalid, match="differs between trajectories"):
        disorder.assign_order_disorder([X, X[:, :1]])
    with pytest.raises(DataInvalid, match="differs between trajectories"):
        disorder.transition_stats([X, X[:, :1]])

    class Long(object):     # 2^26 frames without the memory: only what the check reads
        ndim, shape, dtype, size = 2, (2 ** 26, 1), np.dtype(np.int8), 2 ** 26

        def __len__(self):
            return 2 ** 26

    import enspara_amd.cards.disorder as mod
    real = mod.np.asarray
    try:
        mod.np.asarray = lambda t, *a, **k: t if isinstance(t, Long) else real(t, *a, **k)
        with pytest.raises(DataInvalid, match="2\\^26"):
            cards.cards_matrices([Long()], [3])
    finally:
        mod.np.asarray = real


# ---- host helpers -----------------------------------------------------------------------------
def test_gates_and_buffered_transitions():
    assert rotamer.get_gates(0, nc.CHI, 15) == (345, 135)
    assert rotamer.get_gates(1, nc.CHI, 15) == (105, 255)
    assert rotamer.get_gates(2, nc.CHI, 15.5) == (224.5, 15.5)
    # inside the gates: stays; on a gate: stays (closed); outside: leaves
    for angle, out in ((120, False), (105, False), (255, False), (104.9, True), (256, True)):
        assert rotamer.is_buffered_transition(1, angle, nc.CHI, 15) is out
    # wrap-around: basin 0 of [0, 120) leaves on upper <= a <= lower
    for angle, out in ((0, False), (134.9, False), (135, True), (345, True), (345.1, False)):
        assert rotamer.is_buffered_transition(0, angle, nc.CHI, 15) is out
    # equal gates never transition
    assert rotamer.is_buffered_transition(0, 90.0, [0, 180, 360], 90) is False
    for k, hb in enumerate(BOUNDS):
        for s in range(len(hb) - 1):
            lo, up = nc.gates(hb, 15.5)
            assert rotamer.get_gates(s, hb, 15.5) == (lo[s], up[s])
    assert rotamer._rotamers is rotamer.rotamers


def test_ord_disord_times_and_disorder_traj():
    # the reference's own test table (float "times")
    tt = np.array([0.0, 0.5, 0.5, 1.0, 1.0, 0.5])
    assert disorder.traj_ord_disord_times(tt) == (1.25, 0.5, 0.1, 0.5)
    assert disorder.traj_ord_disord_times(np.array([], dtype=np.int64)) == (0.0, 0.0, 0.0, 0.0)
    assert disorder.traj_ord_disord_times(np.array([7])) == (28.0, 7, 0.0, 0.0)
    golden_tt = _golden_tt()
    for i in (0, 4):
        for j in range(12):
            got = disorder.traj_ord_disord_times(golden_tt[i][j])
            assert tuple(float(x) for x in got) == tuple(G["rag_times"][i, j])
    ends = np.cumsum(G["rag_lengths"])
    for j in (3, 11):
        got = disorder.create_disorder_traj(golden_tt[4][j].astype(np.int64), 1500,
                                            G["rag_mean_ord"][j], G["rag_mean_dis"][j])
        assert got.dtype == np.float64
        assert np.array_equal(got, G["rag_D"][ends[3]:ends[4], j])
    assert not disorder.create_disorder_traj(np.array([5]), 10, 3.0, 1.0).any()


def test_aggregate_mean_times():
    times = np.array([[1.0, 0.0], [3.0, 4.0], [0.0, 8.0]])
    got = disorder.aggregate_mean_times(times, None, np.array([10, 30, 60]))
    wt = np.array([10, 30, 60]) / 100
    assert np.array_equal(got, [(times[:, 0] * wt).sum(), (times[:, 1] * wt).sum()])
    o, no, d, nd = (G["rag_times"][:, :, k] for k in range(4))
    assert np.array_equal(disorder.aggregate_mean_times(o, no, G["rag_lengths"]),
                          G["rag_mean_ord"])
    assert np.array_equal(disorder.aggregate_mean_times(d, nd, G["rag_lengths"]),
                          G["rag_mean_dis"])


# ---- transitions: the reference's three tables ------------------------------------------------
def test_transition_times():
    states = np.array([0, 0, 1, 1, 1, 2, 3, 3])
    assert np.array_equal(disorder.transitions(states), [1, 4, 5])


def test_transition_times_multidim():
    states = np.array([[0, 0, 1, 1, 1, 2, 3, 3],
                       [0, 0, 1, 1, 1, 2, 2, 2]])
    tt = disorder.transitions(states)
    assert np.array_equal(tt[0], [1, 4, 5]) and np.array_equal(tt[1], [1, 4])


def test_transition_times_ragged():
    states = ra.RaggedArray([[0, 0, 1, 1, 1, 2, 3, 3], [0, 0, 1, 1, 1]])
    tt = disorder.transitions(states)
    assert np.array_equal(tt[0], [1, 4, 5]) and np.array_equal(tt[1], [1])
    # a last row without a transition keeps its (empty) row
    tt = disorder.transitions(np.array([[0, 1, 1], [2, 2, 2]]))
    assert len(tt) == 2 and np.array_equal(tt[0], [0]) and len(tt[1]) == 0


# ---- the package ---------------------------------------------------------------------------------
def test_scan_chunk_is_the_library_s():
    L = _lib.load()
    assert cards.SCAN_CHUNK == L.ek_cards_scan_chunk() == 2048
    assert cards.SCAN_CHUNK % 1024 == 0


def test_featurizer_attributes():
    q = {"phi": np.array([[0, 1, 2, 3]]), "chi": np.array([[1, 2, 3, 4], [2, 3, 4, 5]])}
    f = cards.RotamerFeaturizer(q, buffer_width=10, n_procs=4)
    assert f.buffer_width == 10 and f.n_procs == 4
    quads, kind, n = rotamer.check_dihedrals(q)
    assert np.array_equal(quads, [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5]])
    assert list(kind) == [0, 2, 2] and list(n) == [2, 3, 3] and n.dtype == np.int16
