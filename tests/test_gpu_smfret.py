"""enspara_amd.geometry.dyes_from_expt_dist on the device (the burst kernel of
csrc/ek_kmc.hip), through the public functions.

Expected values come from tests/_numpy_kmc.py, never from a device call.  Trajectories
and efficiencies per photon must be array_equal; FRET_val and FRET_std are then the
reference's numpy expressions on equal flags, so they must be equal too.

Shapes.  A burst is a lane; a workgroup is one wave of 64 bursts and writes trajectories in
tiles of 16 frames.  Bursts 1, 64, 65, 257; photons per burst cycle through 1, 2, 63, 64,
65; last frames cycle through 0, 1, 15, 16, 17, 300 and 3000, so one wave holds bursts of
very different lengths; frames repeat; some bursts have a photon at frame 0.  The per-state
histograms have 2, 1, 64, 65, 3 and 2 bins, some of probability zero."""
import functools

import numpy as np
import pytest

import _numpy_kmc as nk
from enspara_amd import ra
from enspara_amd.exception import DataInvalid
from enspara_amd.geometry import dyes_from_expt_dist as dyes
from enspara_amd.msm import synthetic_data as sd

pytestmark = pytest.mark.gpu

SEED = 0xF2E7000000000001
R0 = 5.4
N_BURSTS = 257
BINS = [2, 1, 64, 65, 3, 2]


@functools.lru_cache(maxsize=None)
def _system():
    rng = np.random.RandomState(21)
    T = nk.random_T(rng, 6, 4)
    pops = rng.dirichlet(np.ones(6))
    pops[4] = 0.0
    pops /= pops.sum()
    dd = []
    for s, bins in enumerate(BINS):
        centres = 2.0 + 0.25 * np.arange(bins) + 0.1 * s
        p = rng.dirichlet(np.ones(bins))
        if bins > 2:
            p[rng.rand(bins) < 0.3] = 0.0
            p[1] = 0.2
            p /= p.sum()
        dd.append(np.stack([centres, p], axis=1))
    frames = []
    for b in range(N_BURSTS):
        n_ph = [1, 2, 63, 64, 65][b % 5]
        last = [0, 1, 15, 16, 17, 300, 3000][b % 7]
        f = np.sort(rng.randint(0, last + 1, size=n_ph))
        if b % 3 == 0:
            f[0] = 0
        if n_ph > 2:
            f[1] = f[2]                 # a repeated frame
        frames.append(np.sort(f))
    return T, pops, ra.RaggedArray(dd), frames


@functools.lru_cache(maxsize=None)
def _model(n_photon_std):
    T, pops, dd, frames = _system()
    return nk.bursts(T, pops, dd, frames, R0, n_photon_std, nk.PhiloxUniforms(SEED))


def _same_FEs(got, want):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("n_bursts", [1, 64, 65, 257])
def test_bursts(n_bursts):
    T, pops, dd, frames = _system()
    for std in (None, 4, 7):
        FEs_want, trajs_want, _ = _model(std)
        FEs, trajs = dyes.sample_FRET_histograms(
            T, pops, dd, frames[:n_bursts], R0, n_procs=3, n_photon_std=std, random_state=SEED)
        _same_FEs(FEs, FEs_want[:n_bursts])
        assert len(trajs) == n_bursts
        for b in range(n_bursts):
            assert trajs[b].shape == (frames[b][-1] + 1,)
            assert np.array_equal(trajs[b], trajs_want[b]), b
        FEs_off, none = dyes.sample_FRET_histograms(
            T, pops, dd, frames[:n_bursts], R0, n_photon_std=std, random_state=SEED,
            return_trajectories=False)
        assert none is None
        _same_FEs(FEs_off, FEs_want[:n_bursts])
    assert np.isnan(_model(None)[0][:, 1]).all() and not np.isnan(_model(4)[0][:, 1]).any()


def test_bursts_cut_into_launches_and_calls(monkeypatch):
    T, pops, dd, frames = _system()
    FEs_want, trajs_want, _ = _model(4)
    with sd.Sampler(T) as s:
        for cap in (5, 16, 1000):
            for keep in (True, False):
                FEs, trajs = dyes.sample_FRET_histograms(
                    s, pops, dd, frames[:70], R0, n_photon_std=4, random_state=SEED,
                    return_trajectories=keep, step_cap=cap)
                _same_FEs(FEs, FEs_want[:70])
                if keep:
                    assert all(np.array_equal(a, b) for a, b in zip(trajs, trajs_want))
        # several device calls: few states, few photons a call
        monkeypatch.setattr(dyes, "_TRAJ_CELLS", 4000)
        FEs, trajs = dyes.sample_FRET_histograms(s, pops, dd, frames, R0, n_photon_std=4,
                                                 random_state=SEED)
        _same_FEs(FEs, FEs_want)
        assert all(np.array_equal(a, b) for a, b in zip(trajs, trajs_want))
        monkeypatch.setattr(dyes, "_PHOTONS", 100)
        FEs, _ = dyes.sample_FRET_histograms(s, pops, dd, frames, R0, n_photon_std=4,
                                             random_state=SEED, return_trajectories=False)
        _same_FEs(FEs, FEs_want)


def test_a_burst_is_a_chain_of_synthetic_trajectories():
    T, pops, dd, frames = _system()
    _, trajs = dyes.sample_FRET_histograms(T, pops, dd, frames[:65], R0, random_state=SEED)
    b = 6                                                       # last frame 3000
    chain = sd.synthetic_trajectories(T, [trajs[b][0]], len(trajs[b]), random_state=SEED,
                                      first_chain=b)[0]
    assert np.array_equal(chain, trajs[b])


def test_fret_probs_and_efficiency():
    T, pops, dd, frames = _system()
    rng = np.random.RandomState(5)
    states = rng.randint(0, 6, size=1000)
    for chain in (0, 3, 2 ** 40 + 5):
        want = nk.fret_probs(dd, states, R0, nk.PhiloxUniforms(SEED), chain=chain)
        got = dyes.sample_FE_probs(dd, states, R0, random_state=SEED, chain=chain)
        assert np.array_equal(got, want)
    assert np.all((got > 0) & (got < 1))
    # photon k of burst b draws what entry k of chain b draws
    _, trajs_want, flags = _model(None)
    b = 4
    E = dyes.sample_FE_probs(dd, trajs_want[b][frames[b]], R0, random_state=SEED, chain=b)
    coin = nk.PhiloxUniforms(SEED)(nk.COIN, b, np.arange(len(frames[b])))
    assert np.array_equal(coin <= E, flags[b])


def test_burst_on_an_empty_row():
    T = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    dd = [np.array([[1.0, 0.5], [2.0, 0.5]])] * 3
    with pytest.raises(DataInvalid, match="state 2"):
        dyes.sample_FRET_histograms(T, [1.0, 0, 0], dd, [[0, 5]], R0, random_state=SEED)
    FEs, trajs = dyes.sample_FRET_histograms(T, [1.0, 0, 0], dd, [[0, 2]], R0, random_state=SEED)
    assert np.array_equal(trajs[0], [0, 1, 2])
