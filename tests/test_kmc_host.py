"""Host-side checks of the kinetic Monte Carlo contract: the plain model of
tests/_numpy_kmc.py against Philox's known answers, numpy's Generator.choice and the real
reference's recorded outputs (tests/golden/kmc_golden.npz, made by make_kmc_golden.py);
the numpy helpers of enspara_amd.geometry.dyes_from_expt_dist against the reference; the
validation errors, which need no device."""
import os

import numpy as np
import pytest
import scipy.sparse
import scipy.stats

import _numpy_kmc as nk
from enspara_amd import _lib, ra
from enspara_amd.exception import DataInvalid
from enspara_amd.geometry import dyes_from_expt_dist as dyes
from enspara_amd.msm import synthetic_data as sd

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "kmc_golden.npz"))


def _split(flat, lengths):
    ends = np.cumsum(lengths)
    return [flat[e - k:e] for e, k in zip(ends, lengths)]


def _hex(words):
    return " ".join("%08x" % w for w in words)


def test_philox_known_answers():
    assert _hex(nk.philox4x32([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(nk.philox4x32([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)) == \
        "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(nk.philox4x32([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344],
                              [0xA4093822, 0x299F31D0])) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"
    # vectorised over counters: the same words
    many = nk.philox4x32([[0, 0, 0, 0], [0xFFFFFFFF] * 4], [[0, 0], [0xFFFFFFFF] * 2])
    assert _hex(many[0]).startswith("6627e8d5") and _hex(many[1]).startswith("408f276d")


def test_doubles_stay_below_one():
    assert nk.to_double(0xFFFFFFFF, 0xFFFFFFFF) == 1 - 2.0 ** -53
    assert nk.to_double(0, 0) == 0.0
    assert nk.to_double(31, 63) == 0.0          # the bits shifted out
    assert nk.to_double(32, 0) == 2.0 ** -27 and nk.to_double(0, 64) == 2.0 ** -53
    u = nk.PhiloxUniforms(99)(nk.TRANS, np.arange(50)[:, None], np.arange(2000)[None, :])
    assert u.shape == (50, 2000) and u.min() >= 0 and u.max() < 1
    assert abs(u.mean() - 0.5) < 0.005
    # an even index and the next odd one share a call; streams and chains do not collide
    g = nk.PhiloxUniforms(99)
    w = nk.philox4x32([3, 0, 7, (nk.BIN << 28) | 1], g.key).astype(np.uint64)
    assert g(nk.BIN, 2 ** 32 + 7, 6) == nk.to_double(w[0], w[1])
    assert g(nk.BIN, 2 ** 32 + 7, 7) == nk.to_double(w[2], w[3])
    assert len({float(g(s, c, 0)) for s in range(5) for c in range(5)}) == 25


def test_step_is_numpys_choice():
    rng = np.random.RandomState(0)
    for trial in range(2000):
        n = rng.randint(1, 40)
        p = rng.dirichlet(np.ones(n))
        if n > 2:
            p[rng.rand(n) < 0.4] = 0.0
            if p.sum() == 0:
                p[rng.randint(n)] = 1.0
            p /= p.sum()
        u = np.random.default_rng(trial).random()
        want = np.random.default_rng(trial).choice(n, 1, p=p)[0]
        assert nk.step(p, u) == want
        cols = np.flatnonzero(p)                 # the nonzeros alone give the same state
        assert cols[np.searchsorted(nk.row_cdf(p[cols]), u, side="right")] == want
        assert nk.step_compressed(nk.compressed(p[None, :]), 0, u) == want


def test_compress_rows_has_numpys_bits():
    T = G["kmc_T"]
    for M in (T, scipy.sparse.csr_matrix(T), scipy.sparse.coo_matrix(T)):
        indptr, cols, cdf = sd.compress_rows(M)
        for i, row in enumerate(nk.compressed(T)):
            lo, hi = indptr[i], indptr[i + 1]
            assert np.array_equal(cols[lo:hi], row[0]) and np.array_equal(cdf[lo:hi], row[1])
            assert cdf[hi - 1] == 1.0
    T0 = T.copy()
    T0[3] = 0.0
    indptr, _, _ = sd.compress_rows(T0)
    assert indptr[4] == indptr[3]


def test_model_replays_the_reference_chain():
    for tag in ("dense", "sparse"):
        u = nk.RecordedUniforms({(nk.TRANS, 0): G["traj_u_" + tag]})
        T = G["kmc_T"] if tag == "dense" else scipy.sparse.csr_matrix(G["kmc_T"])
        got = nk.chains(T, [int(G["traj_start"])], 300, u)[0]
        assert np.array_equal(got, G["traj_" + tag])


def test_model_replays_the_reference_bursts():
    T, pops, R0 = G["kmc_T"], G["pops"], float(G["R0"])
    dd = _split(G["dd"], G["dd_lengths"])
    frames = _split(G["burst_frames"], G["burst_lengths"])
    trjs = _split(G["burst_trj"], G["burst_trj_lengths"])
    per_photon = {k: _split(G["burst_u_" + k], G["burst_lengths"])
                  for k in ("bin", "jitter", "coin")}
    trans = _split(G["burst_u_trans"], G["burst_trj_lengths"] - 1)
    for b, f in enumerate(frames):
        std = int(G["burst_std"][b]) or None
        u = nk.RecordedUniforms({
            (nk.INIT, b): [G["burst_u_init"][b]], (nk.TRANS, b): trans[b],
            (nk.BIN, b): per_photon["bin"][b], (nk.JITTER, b): per_photon["jitter"][b],
            (nk.COIN, b): per_photon["coin"][b]})
        val, dev, trj, _ = nk.burst(T, pops, dd, f, R0, std, u, chain=b)
        assert np.array_equal(trj, trjs[b]) and len(trj) == f.max() + 1
        assert val == G["burst_val"][b]
        if std is None:
            assert dev is None and np.isnan(G["burst_sd"][b])
        else:
            assert dev == G["burst_sd"][b]
    assert {int(s) for s in G["burst_std"]} == {0, 4, 7}
    # the efficiencies: the model's d^6 = (d d)(d d)(d d) against the reference's d ** 6,
    # five roundings against one, then the same sum and quotient: 2^-49 relative
    u2 = G["fe_u"]
    E = nk.fret_probs(dd, G["fe_states"], R0, nk.RecordedUniforms(
        {(nk.BIN, 0): u2[:, 0], (nk.JITTER, 0): u2[:, 1]}))
    assert np.all(np.abs(E - G["fe_E"]) <= 2.0 ** -49 * G["fe_E"])


def test_ensemble_model_against_the_reference():
    T, p0, obs = G["ens_T"], G["ens_p0"], G["ens_obs"]
    for tag, M in (("dense", T), ("sparse", scipy.sparse.csr_matrix(T))):
        p, every = nk.ensemble(M, p0, 30)
        want = G["ens_%s_all" % tag]
        bound = nk.ensemble_bound(T, p0, 30)
        assert every.shape == want.shape == (30, 5)
        assert np.array_equal(every, want) or np.all(np.abs(every - want).sum(axis=1) <= bound)
        assert np.abs(p - G["ens_%s_p" % tag]).sum() <= bound[-1]
        _, o = nk.ensemble(M, p0, 30, obs)
        o_want = G["ens_%s_obs" % tag]
        assert np.array_equal(o, o_want) or \
            np.all(np.abs(o - o_want) <= nk.observable_bound(T, p0, 30, obs))
    assert np.all(np.diff(nk.ensemble_bound(T, p0, 30)) > 0)


def test_numpy_helpers_are_the_references():
    assert np.array_equal(dyes.FRET_efficiency(G["fe_dists"], float(G["fe_r0"]),
                                               offset=float(G["fe_offset"])), G["fe_out"])
    probs = _split(G["md_probs"], G["md_lengths"])
    edges = _split(G["md_edges"], G["md_lengths"] + 1)
    for e in (ra.RaggedArray(edges), edges):
        made = dyes.make_distribution(ra.RaggedArray(probs), e)
        assert np.array_equal(made._data, G["md_out"])
        assert np.array_equal(made.lengths, G["md_out_lengths"])
    times = _split(G["cp_times"], G["cp_lengths"])
    conv = dyes.convert_photon_times(times, float(G["cp_lagtime"]), float(G["cp_slowing"]))
    assert conv.dtype == object and len(conv) == 3
    assert np.array_equal(np.concatenate(list(conv)), G["cp_out"])
    assert [list(c) for c in dyes.divide_chunks(list(range(5)), 2)] == [[0, 1], [2, 3], [4]]


def _dd(n):
    return [np.array([[1.0, 0.5], [2.0, 0.5]])] * n


def test_invalid_input_raises_without_a_device():
    T = G["kmc_T"]
    bad_T = []
    for change in ("negative", "nan", "sum", "shape"):
        M = T.copy()
        if change == "negative":
            M[1, 1], M[1, 2] = -0.1, M[1, 2] + M[1, 1] + 0.1
        elif change == "nan":
            M[0, 0] = np.nan
        elif change == "sum":
            M[2] *= 1 + 1e-7
        else:
            M = M[:, :5]
        bad_T.append(M)
    bad_T.append(scipy.sparse.csr_matrix(bad_T[2]))
    for M in bad_T:
        with pytest.raises(DataInvalid):
            sd.synthetic_trajectory(M, 0, 10, random_state=1)
        with pytest.raises(DataInvalid):
            sd.synthetic_trajectories(M, [0, 1], 10, random_state=1)
        with pytest.raises(DataInvalid):
            sd.sample_next(M, [0], [0.5])
        with pytest.raises(DataInvalid):
            sd.synthetic_ensemble(M, np.ones(6) / 6, 3)
        with pytest.raises(DataInvalid):
            dyes.sample_FRET_histograms(M, np.ones(6) / 6, _dd(6), [[0, 1]], 5.4)
    ok_sum = T.copy()
    ok_sum[2] *= 1 + 1e-9                       # within sqrt(eps): numpy takes it, so do we
    sd.compress_rows(ok_sum)
    for start in (-1, 6, [0, 6]):
        with pytest.raises(DataInvalid):
            sd.synthetic_trajectories(T, np.atleast_1d(start), 10, random_state=1)
    with pytest.raises(DataInvalid):
        sd.synthetic_trajectory(T, 6, 10)
    for n_steps in (0, -3, 2.5):
        with pytest.raises(DataInvalid):
            sd.synthetic_trajectory(T, 0, n_steps, random_state=1)
        with pytest.raises(DataInvalid):
            sd.synthetic_ensemble(T, np.ones(6) / 6, n_steps)
    with pytest.raises(DataInvalid):
        sd.synthetic_trajectory(T, 0, 10, random_state=-1)
    with pytest.raises(DataInvalid):
        sd.synthetic_ensemble(T, np.ones(5) / 5, 3)
    pops = G["pops"]
    for frames in ([[-1, 2]], [[0, 3, 2]], [[]], [[0, 1], [2.5]], []):
        with pytest.raises(DataInvalid):
            dyes.sample_FRET_histograms(T, pops, _dd(6), frames, 5.4, random_state=1)
    with pytest.raises(DataInvalid):
        dyes.sample_FRET_histograms(T, pops, _dd(5), [[0, 1]], 5.4, random_state=1)
    for p in (pops * 1.001, pops[:5], -pops):
        with pytest.raises(DataInvalid):
            dyes.sample_FRET_histograms(T, p, _dd(6), [[0, 1]], 5.4, random_state=1)
    with pytest.raises(DataInvalid):
        dyes.sample_FE_probs(_dd(3), [0, 3], 5.4, random_state=1)
    with pytest.raises(DataInvalid):
        dyes.sample_FE_probs([np.array([[1.0, 0.7], [2.0, 0.7]])] * 3, [0], 5.4, random_state=1)


def test_device_calls_fail_loudly_without_a_device():
    """no CPU fallback: with no HIP device every sampling call raises HipError (with one,
    the same calls simply run)"""
    T, pops = G["kmc_T"], G["pops"]
    calls = [
        lambda: sd.synthetic_trajectory(T, 0, 10, random_state=1),
        lambda: sd.synthetic_trajectories(scipy.sparse.csr_matrix(T), [0, 1], 10, random_state=1),
        lambda: sd.sample_next(T, [0, 1], [0.2, 0.9]),
        lambda: sd.synthetic_ensemble(T, pops, 4),
        lambda: dyes.sample_FE_probs(_dd(6), [0, 5], 5.4, random_state=1),
        lambda: dyes.sample_FRET_histograms(T, pops, _dd(6), [[0, 3]], 5.4, random_state=1),
    ]
    has_gpu = _lib.load().ek_device_count() > 0
    for call in calls:
        if has_gpu:
            call()
        else:
            with pytest.raises(_lib.HipError):
                call()
    assert sd.last_seed == 1
    sd._seed(None)
    assert isinstance(sd.last_seed, int) and 0 <= sd.last_seed < 2 ** 64


def _chi2(T, trajs):
    """Pearson chi^2 of the transition counts against T, and its degrees of freedom"""
    n = len(T)
    C = np.zeros((n, n))
    np.add.at(C, (trajs[:, :-1].ravel(), trajs[:, 1:].ravel()), 1)
    E = C.sum(axis=1)[:, None] * T
    live = T > 0
    assert not C[~live].any()
    stat = ((C - E)[live] ** 2 / E[live]).sum()
    dof = int(((T > 0).sum(axis=1) - 1)[C.sum(axis=1) > 0].sum())
    return stat, dof


def test_model_statistics():
    """one deterministic check of the model: the transition counts of one chain of 200 000
    steps and of 4096 chains of 50 steps on a 5-state T, each below the 1 - 10^-6 quantile
    of chi^2 at its degrees of freedom (seeds fixed, so this cannot flicker)"""
    T = G["ens_T"]
    assert T.shape == (5, 5)
    long = nk.chains(T, [0], 200000, nk.PhiloxUniforms(2024))
    stat, dof = _chi2(T, long)
    assert dof == (T > 0).sum() - 5
    assert stat < scipy.stats.chi2.ppf(1 - 1e-6, dof), (stat, dof)
    many = nk.chains(T, np.arange(4096) % 5, 50, nk.PhiloxUniforms(2025))
    stat, dof = _chi2(T, many)
    assert stat < scipy.stats.chi2.ppf(1 - 1e-6, dof), (stat, dof)
