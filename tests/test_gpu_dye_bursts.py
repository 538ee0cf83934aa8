"""The explicit-dye burst samplers on the device (csrc/ek_dye_bursts.hip on the burst loop of
csrc/ek_kmc_burst.h), through the public functions and so through the C ABI.

Expected values come from tests/_numpy_dye_bursts.py, never from a device call, with one
exception: k2, r and the FE behind a kappa-squared photon are compared bit for bit with
``explicit_r0_calc.pair_table`` of the state's conformations, which
tests/test_gpu_dye_lifetimes.py already holds to the exact values within derived bounds.

Shapes: those of tests/test_gpu_smfret.py (its six-state T, populations and frames: bursts 1,
64, 65, 257 bracket the wave a workgroup is, last frames from 0 to 3000 bracket the tile of 16
frames, frames repeat) plus a seventh, dyeless state of population 0 that nothing enters.
Photon events per state 1, 2, 63, 64, 65, 1000 among non-radiative ones; conformations per
state and side (1, 1), (2, 7), (7, 2), (64, 65), (65, 64), (5, 5).

The flags of the kappa-squared rule are an argument in three parts, as in
tests/test_gpu_dye_lifetimes.py: (a) the largest gap between the device's FE and the model's,
(b) every photon's |coin - FE| in the model, (c) gap < margin / 2 for every photon, asserted,
none left out; then both sides decide every coin alike."""
import functools
import gc
import os

import numpy as np
import pytest

import _numpy_dye_bursts as nb
import _numpy_dye_lifetimes as nd
import test_dye_bursts_host as th
import test_gpu_lifetime as tl
import test_gpu_smfret as ts
from _lifetime_cases import Case, bits
from enspara_amd import _lib
from enspara_amd.exception import DataInvalid
from enspara_amd.geometry import dye_lifetimes as dl
from enspara_amd.geometry import dyes_from_expt_dist as dyes
from enspara_amd.geometry import explicit_r0_calc as r0c
from enspara_amd.msm import synthetic_data as sd

pytestmark = pytest.mark.gpu

G = th.G
SEED = ts.SEED
PARAMS = (2.5e15, 0.92, 4.1)
COUNTS = [1, 2, 63, 64, 65, 1000]
CONFS = [(1, 1), (2, 7), (7, 2), (64, 65), (65, 64), (5, 5)]
C6 = 0.02108 ** 6 * PARAMS[1] * PARAMS[0] / 1.333 ** 4
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _system():
    """(T [7, 7], populations, frames, events, donor and acceptor conformations, dd)"""
    T6, pops6, dd6, frames = ts._system()
    T = np.zeros((7, 7))
    T[:6, :6] = T6
    pops = np.concatenate([pops6, [0.0]])
    rng = np.random.RandomState(31)
    events = []
    for m in COUNTS:
        total = m + (0 if m == 1 else rng.randint(1, 5 + m // 2))
        codes = np.ones(total, dtype=np.int8)
        codes[rng.choice(total, size=m, replace=False)] = rng.choice([0, 2], size=m)
        events.append((np.round(rng.exponential(3.0, size=total), 4), codes))
    events.append(([], []))
    dc = [nd.random_coords(rng, i, (0, 0, 0)) for i, _ in CONFS] + [[]]
    ac = [nd.random_coords(rng, j, (4.5, 1.0, 0)) for _, j in CONFS] + [[]]
    dd = list(dd6) + [np.array([[1.0, 0.5], [2.0, 0.5]])]
    return T, pops, frames, events, dc, ac, dd


@functools.lru_cache(maxsize=None)
def _chains():
    T, pops, frames = _system()[:3]
    return nb.burst_chains(T, pops, frames, nb.PhiloxUniforms(SEED))


@functools.lru_cache(maxsize=None)
def _life_model():
    T, pops, frames, events = _system()[:4]
    return nb.lifetime_bursts(T, pops, nb.event_table(events), frames, nb.PhiloxUniforms(SEED),
                              trajs=_chains())


@functools.lru_cache(maxsize=None)
def _k2_model():
    T, pops, frames, _, dc, ac, _ = _system()
    return nb.k2_bursts(T, pops, dc, ac, frames, C6, nb.PhiloxUniforms(SEED), trajs=_chains())


def _same_rows(got, want, dtype, n=None):
    n = len(got) if n is None else n
    assert len(got) == n and got._data.dtype == dtype
    for b in range(n):
        assert np.asarray(got[b]).tobytes() == np.asarray(want[b], dtype=dtype).tobytes(), b


def _same_trajs(got, want, n):
    assert len(got) == n
    for b in range(n):
        assert got[b].dtype == np.int32 and np.array_equal(got[b], want[b]), b


# ---- lifetime bursts -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_bursts", [1, 64, 65, 257])
def test_lifetime_bursts(n_bursts):
    T, pops, frames, events = _system()[:4]
    flags, lifes, states, trajs = _life_model()
    assert list(nb.event_table(events)[3]) == COUNTS + [0] and not T[:, 6].any()
    got = dl.sample_lifetime_bursts(T, pops, events, frames[:n_bursts], random_state=SEED,
                                    return_trajectories=True)
    assert len(got) == 4
    _same_rows(got[0], flags, np.uint8, n_bursts)
    _same_rows(got[1], lifes, np.float64, n_bursts)
    _same_rows(got[2], states, np.int32, n_bursts)
    _same_trajs(got[3], trajs, n_bursts)
    off = dl.sample_lifetime_bursts(T, pops, dl.event_table(events), frames[:n_bursts],
                                    random_state=SEED)
    assert len(off) == 3 and bits(off) == bits(got[:3])
    assert dl.last_seed == SEED and dl.burst_timing().shape == (3,)


def test_cut_into_launches_and_calls(monkeypatch):
    T, pops, frames, events, dc, ac, _ = _system()
    with sd.Sampler(T) as s:
        want_l = dl.sample_lifetime_bursts(s, pops, events, frames, random_state=SEED,
                                           return_trajectories=True)
        want_k = r0c.sample_k2_bursts(s, pops, dc, ac, frames, PARAMS, random_state=SEED,
                                      return_trajectories=True, return_conformations=True)
        _same_rows(want_l[1], _life_model()[1], np.float64)
        _same_rows(want_k[4], _k2_model()[4], np.int32)
        for cap in (5, 16, 1000):
            for keep in (True, False):
                got = dl.sample_lifetime_bursts(s, pops, events, frames[:70], random_state=SEED,
                                                return_trajectories=keep, step_cap=cap)
                for a, b in zip(got[:3], want_l):
                    assert bits(list(a)) == bits(list(b)[:70])
                if keep:
                    _same_trajs(got[3], want_l[3], 70)
                got = r0c.sample_k2_bursts(s, pops, dc, ac, frames[:70], PARAMS, random_state=SEED,
                                           return_trajectories=keep, return_conformations=True,
                                           step_cap=cap)
                for a, b in zip(got[:6], want_k):
                    assert bits(list(a)) == bits(list(b)[:70])
        # several device calls: few states, then few photons a call
        monkeypatch.setattr(dl, "_TRAJ_CELLS", 4000)
        assert bits(dl.sample_lifetime_bursts(s, pops, events, frames, random_state=SEED,
                                              return_trajectories=True)) == bits(want_l)
        assert bits(r0c.sample_k2_bursts(s, pops, dc, ac, frames, PARAMS, random_state=SEED,
                                         return_trajectories=True,
                                         return_conformations=True)) == bits(want_k)
        monkeypatch.setattr(dl, "_PHOTONS", 100)
        assert bits(dl.sample_lifetime_bursts(s, pops, events, frames,
                                              random_state=SEED)) == bits(want_l[:3])
        assert bits(r0c.sample_k2_bursts(s, pops, dc, ac, frames, PARAMS, random_state=SEED,
                                         return_conformations=True)) == bits(want_k[:6])


def test_one_chain_whichever_rule():
    T, pops, frames, events, dc, ac, dd = _system()
    n = 65
    with sd.Sampler(T) as s:
        a = dl.sample_lifetime_bursts(s, pops, events, frames[:n], random_state=SEED,
                                      return_trajectories=True)[3]
        _, b, _, _ = r0c.simulate_burst_k2(frames[:n], s, pops, dc, ac, PARAMS, random_state=SEED)
        _, c = dyes.sample_FRET_histograms(s, pops, dd, frames[:n], ts.R0, random_state=SEED)
        for k in range(n):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
        for k in (0, 5, 6, 13, 64):                      # last frames 0, 300, 3000, 3000, 1
            chain = sd.synthetic_trajectories(s, [a[k][0]], len(a[k]), random_state=SEED,
                                              first_chain=k)[0]
            assert np.array_equal(chain, a[k]), k
    _same_trajs(a, _chains(), n)


# ---- per-entry calls -------------------------------------------------------------------------------
def test_per_entry_calls_equal_the_bursts():
    T, pops, frames, events, dc, ac, _ = _system()
    flags, lifes, states, _ = _life_model()
    kflags, k2, r, _, di, ai, _, kstates, _ = _k2_model()
    life, out = [e[0] for e in events], [e[1] for e in events]
    names = [dl.outcome_names(o) if len(o) else [] for o in out]
    for b in (0, 3, 4, 64, 256):
        ph, lt = dl._sample_lifetimes_guarenteed_photon(states[b], life, out, rng_seed=SEED,
                                                        chain=b)
        assert ph.dtype == np.uint8 and np.array_equal(ph, flags[b])
        assert lt.tobytes() == lifes[b].tobytes()
        one = dl.sample_lifetimes_guarenteed_photon(frames[b], T, pops, life, names,
                                                    rng_seed=SEED, chain=b)
        assert np.array_equal(one[0], flags[b]) and one[1].tobytes() == lifes[b].tobytes()
        assert one[2].dtype == np.int32 and np.array_equal(one[2], states[b])
        gk2, gr, gd, ga = r0c.sample_dye_coords(dc, ac, kstates[b], random_state=SEED, chain=b,
                                                return_conformations=True)
        assert np.array_equal(gd, di[b]) and np.array_equal(ga, ai[b])
        plain = r0c.sample_dye_coords(dc, ac, kstates[b], random_state=SEED, chain=b)
        assert bits(plain) == bits((gk2, gr))
        assert np.all(np.abs(gk2 - k2[b]) <= 2 * nd.K2_ABS)
        assert np.all(np.abs(gr - r[b]) <= 2 * nd.R_REL * r[b])


def test_pick_events():
    events = _system()[3]
    table = nb.event_table(events)
    uni = nb.PhiloxUniforms(SEED)
    states = np.random.RandomState(3).randint(0, 6, size=3000)
    u = uni(nb.EVENT, 7, np.arange(len(states)))
    want = nb.lifetime_photons(table, states, uni, chain=7)[2]
    got = dl.pick_events(events, states, u)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(dl.pick_events(dl.event_table(events), states.reshape(30, 100),
                                         u.reshape(30, 100)), want.reshape(30, 100))
    for m in (1, 3, 64, 1000):
        ub = th.boundary_doubles(m)
        one = [(np.zeros(m), np.zeros(m, dtype=np.int8))]
        got = dl.pick_events(one, np.zeros(len(ub), dtype=np.int64), ub)
        assert np.array_equal(got, nb.pick(ub, m)) and got.max() == m - 1 and got.min() == 0


# ---- kappa-squared bursts --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tables():
    """the device's pair table of every state's conformations: (k2, r, FE) [nd, na] each"""
    _, _, _, _, dc, ac, _ = _system()
    return [r0c.pair_table(dc[s], ac[s], PARAMS) for s in range(6)]


@pytest.mark.parametrize("n_bursts", [1, 64, 65, 257])
def test_k2_bursts(n_bursts):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    T, pops, frames, _, dc, ac, _ = _system()
    mflags, mk2, mr, mFE, mi, mj, margin, mstates, trajs = _k2_model()
    photons, k2s, rs, states, drows, arows, got_trajs = r0c.sample_k2_bursts(
        T, pops, dc, ac, frames[:n_bursts], PARAMS, random_state=SEED, return_trajectories=True,
        return_conformations=True)
    # (a) the chain and the rows
    _same_rows(states, mstates, np.int32, n_bursts)
    _same_rows(drows, mi, np.int32, n_bursts)
    _same_rows(arows, mj, np.int32, n_bursts)
    _same_trajs(got_trajs, trajs, n_bursts)
    tables = _tables()
    coin = nb.PhiloxUniforms(SEED)
    K = nb._K(C6)
    gap, tightest = 0.0, np.inf
    ratios = {"k2": 0.0, "r": 0.0, "FE": 0.0}
    for b in range(n_bursts):
        s, i, j = mstates[b], mi[b], mj[b]
        # (b) bit for bit the pair table's
        tk2 = np.array([tables[x][0][y, z] for x, y, z in zip(s, i, j)])
        tr = np.array([tables[x][1][y, z] for x, y, z in zip(s, i, j)])
        tFE = np.array([tables[x][2][y, z] for x, y, z in zip(s, i, j)])
        assert np.asarray(k2s[b]).tobytes() == tk2.tobytes(), b
        assert np.asarray(rs[b]).tobytes() == tr.tobytes(), b
        c = coin(nb.COIN, b, np.arange(len(s)))
        assert np.array_equal(np.asarray(photons[b]), (c <= tFE).astype(np.uint8)), b
        # (c) against the model
        d = np.array([dc[x][y] for x, y in zip(s, i)])
        a = np.array([ac[x][z] for x, z in zip(s, j)])
        xk2, xr, xFE, _ = nd.pair_exact(d, a, K)
        ratios["k2"] = max(ratios["k2"], float((np.abs(tk2 - xk2) / nd.K2_ABS).max()))
        ratios["r"] = max(ratios["r"], float((np.abs(tr - xr) / (nd.R_REL * xr)).max()))
        ratios["FE"] = max(ratios["FE"],
                           float((np.abs(tFE - xFE) / nd.fe_bound(xk2, xr, K)).max()))
        gap = max(gap, float(np.abs(tFE - mFE[b]).max()))
        tightest = min(tightest, float(margin[b].min()))
        assert np.all(np.abs(tFE - mFE[b]).max() < margin[b] / 2), b
        assert np.array_equal(np.asarray(photons[b]), mflags[b].astype(np.uint8)), b
    print("%d bursts: largest |FE - FE_model| %.3g, smallest |coin - FE| %.3g; largest ratio to "
          "the bound: %s" % (n_bursts, gap, tightest,
                             ", ".join("%s %.3g" % kv for kv in ratios.items())))
    assert all(v <= 1 for v in ratios.values())
    assert gap < tightest / 2
    # the reference's return values
    FEs, tr2, k2b, rb = r0c.simulate_burst_k2(frames[:n_bursts], T, pops, dc, ac, PARAMS,
                                              random_state=SEED, n_procs=4)
    assert np.array_equal(FEs, [np.mean(f) for f in mflags[:n_bursts]])
    assert bits((k2b, rb)) == bits((k2s, rs))
    _same_trajs(tr2, trajs, n_bursts)
    none = r0c.simulate_burst_k2(frames[:n_bursts], T, pops, dc, ac, PARAMS, random_state=SEED,
                                 return_trajectories=False)
    assert none[1] is None and bits((none[0], none[2], none[3])) == bits((FEs, k2b, rb))


# ---- the host steps that end on the device -----------------------------------------------------------
def test_remake_and_remove_dyeless_equal_the_reference():
    lifetimes = [np.ones(k) for k in G["rm_lengths"]]
    tprobs, eqs = dl.remake_prot_MSM_from_lifetimes(lifetimes, G["rm_counts"],
                                                    prot_eqs=G["rm_eqs_in"])
    bad = np.flatnonzero(G["rm_lengths"] == 0)
    assert np.array_equal(tprobs, G["rm_tprobs"]) and len(bad) == 2
    assert np.all(eqs[bad] == 0.0)
    np.testing.assert_allclose(eqs, np.where(G["rm_lengths"] == 0, 0.0, G["rm_eqs"]), rtol=0,
                               atol=1e-10)
    c1 = [np.ones((k, 9)) for k in G["rd_len1"]]
    c2 = [np.ones((k, 9)) for k in G["rd_len2"]]
    eqs, tprobs, o1, o2 = r0c.remove_dyeless_msm_states(c1, c2, G["rd_eqs_in"], G["rd_counts"])
    bad = np.flatnonzero((G["rd_len1"] == 0) | (G["rd_len2"] == 0))
    assert np.array_equal(tprobs, G["rd_tprobs"]) and np.all(eqs[bad] == 0.0)
    keep = np.ones(len(eqs), dtype=bool)
    keep[bad] = False
    np.testing.assert_allclose(eqs[keep], G["rd_eqs"][keep], rtol=0, atol=1e-10)
    assert [len(x) for x in o1] == list(G["rd_out_len1"])
    assert [len(x) for x in o2] == list(G["rd_out_len2"])
    assert all(not o1[i].any() and not o2[i].any() and o1[i].shape == (1, 9) for i in bad)
    assert len(c1[2]) == 0                          # the caller's lists are left alone


def test_run_mc():
    T, pops, frames, events = _system()[:4]
    rng = np.random.RandomState(8)
    counts = rng.randint(1, 30, size=(7, 7))
    FEs, d_l, a_l, photons, states = dl.run_mc(events, counts, frames[:65], random_state=SEED)
    tprobs, eqs = dl.remake_prot_MSM_from_lifetimes([e[0] for e in events], counts)
    assert eqs[6] == 0.0 and not tprobs[:, 6].any() and not tprobs[6].any()
    flags, lifes, mstates, _ = nb.lifetime_bursts(tprobs, eqs, nb.event_table(events),
                                                  frames[:65], nb.PhiloxUniforms(SEED))
    _same_rows(photons, flags, np.uint8)
    _same_rows(states, mstates, np.int32)
    assert np.array_equal(FEs, [np.sum(f) / len(f) for f in flags])
    for b in range(65):
        assert np.array_equal(d_l[b], lifes[b][flags[b] == 0])
        assert np.array_equal(a_l[b], lifes[b][flags[b] == 1])


# ---- raises --------------------------------------------------------------------------------------------
T3 = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
EV3 = [([1.0], [0]), ([1.0, 2.0], [1, 1]), ([], [])]
ONE = np.array([[0.0, 0, 0, 0, 0, 0, 1.0, 0, 0]])
FAR = ONE + [3.0, 0, 0, 3.0, 1.0, 0, 0, 1.0, 0]
C3D, C3A = [ONE, ONE, ONE], [FAR, [], FAR]


def _raise_only_non_radiative():
    dl.sample_lifetime_bursts(T3, [1.0, 0, 0], EV3, [[0, 1]], random_state=SEED)


def _raise_dyeless():
    dl.sample_lifetime_bursts(T3, [0, 0, 1.0], EV3, [[0]], random_state=SEED,
                              return_trajectories=True)


def _raise_no_conformation():
    r0c.simulate_burst_k2([[0, 1]], T3, [1.0, 0, 0], C3D, C3A, PARAMS, random_state=SEED)


def _raise_empty_row_lifetimes():
    dl.sample_lifetime_bursts(T3, [1.0, 0, 0], [EV3[0]] * 3, [[0, 5]], random_state=SEED)


def _raise_empty_row_k2():
    r0c.simulate_burst_k2([[0, 5]], T3, [1.0, 0, 0], C3D, [FAR] * 3, PARAMS, random_state=SEED)


RAISES = [_raise_only_non_radiative, _raise_dyeless, _raise_no_conformation,
          _raise_empty_row_lifetimes, _raise_empty_row_k2]


def test_raises():
    with pytest.raises(DataInvalid, match="state 1, which has only non-radiative"):
        _raise_only_non_radiative()
    with pytest.raises(DataInvalid, match="state 2, which has no event at all"):
        _raise_dyeless()
    with pytest.raises(DataInvalid, match="state 1, which has no acceptor conformation"):
        _raise_no_conformation()
    with pytest.raises(DataInvalid, match="state 1"):
        dl._sample_lifetimes_guarenteed_photon([0, 1], [e[0] for e in EV3], [e[1] for e in EV3],
                                               rng_seed=SEED)
    with pytest.raises(DataInvalid, match="state 1"):
        r0c.sample_dye_coords(C3D, C3A, [0, 2, 1], random_state=SEED)
    with pytest.raises(DataInvalid, match="state 1"):
        dl.pick_events(EV3, [0, 1], [0.5, 0.5])
    # the empty-row case of tests/test_gpu_smfret.py, for both rules
    for call in (_raise_empty_row_lifetimes, _raise_empty_row_k2):
        with pytest.raises(DataInvalid, match="state 2"):
            call()
    out = dl.sample_lifetime_bursts(T3, [1.0, 0, 0], [EV3[0]] * 3, [[0, 2]], random_state=SEED,
                                    return_trajectories=True)
    assert np.array_equal(out[3][0], [0, 1, 2]) and np.array_equal(out[2][0], [0, 2])
    _, trajs, _, _ = r0c.simulate_burst_k2([[0, 2]], T3, [1.0, 0, 0], C3D, [FAR] * 3, PARAMS,
                                           random_state=SEED)
    assert np.array_equal(trajs[0], [0, 1, 2])


# ---- resources --------------------------------------------------------------------------
def _small():
    T, pops, frames, events, dc, ac, _ = _system()
    return T, pops, frames[:20], events, dc, ac


def _two_calls(fn):
    """fn under bounds that cut its 20 bursts into two device calls"""
    keep = dl._PHOTONS
    dl._PHOTONS = 400
    try:
        return fn()
    finally:
        dl._PHOTONS = keep


def _life_bursts():
    T, pops, frames, events, _, _ = _small()
    return dl.sample_lifetime_bursts(T, pops, events, frames, random_state=SEED,
                                     return_trajectories=True, step_cap=100)


def _k2_bursts():
    T, pops, frames, _, dc, ac = _small()
    return r0c.simulate_burst_k2(frames, T, pops, dc, ac, PARAMS, random_state=SEED,
                                 return_conformations=True, step_cap=100)


def _events():
    events = _system()[3]
    return [e[0] for e in events], [e[1] for e in events]


CASES = [
    Case("sample_lifetime_bursts, two calls", fn=lambda: _two_calls(_life_bursts)),
    Case("simulate_burst_k2, two calls", fn=lambda: _two_calls(_k2_bursts)),
    Case("sample_lifetime_bursts", fn=_life_bursts),
    Case("simulate_burst_k2", fn=_k2_bursts),
    Case("sample_lifetimes_guarenteed_photon", fn=lambda: dl.sample_lifetimes_guarenteed_photon(
        _small()[2][3], _small()[0], _small()[1], *_events(), rng_seed=SEED, chain=3)),
    Case("_sample_lifetimes_guarenteed_photon", fn=lambda: dl._sample_lifetimes_guarenteed_photon(
        [0, 1, 5, 3], *_events(), rng_seed=SEED)),
    Case("pick_events", fn=lambda: dl.pick_events(_system()[3], [0, 5, 2], [0.1, 0.9, 0.5])),
    Case("sample_dye_coords", fn=lambda: r0c.sample_dye_coords(
        _small()[4], _small()[5], [0, 1, 5, 3], random_state=SEED, return_conformations=True)),
    Case("run_mc", fn=lambda: dl.run_mc(_system()[3], np.arange(1, 50).reshape(7, 7),
                                        _small()[2], random_state=SEED)),
]
MAX_ALLOCS = 80         # two calls: twice the loop's 9 and a rule's up to 9; a handle (3)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_balance(case):
    n_ph = sum(len(f) for f in _small()[2])
    assert 400 < n_ph < 800                         # two calls under _two_calls' bound
    tl.test_balance(case)


@pytest.mark.parametrize("call", RAISES, ids=[c.__name__ for c in RAISES])
def test_raise_paths_balance(call):
    tl.test_raise_paths_balance(call.__name__, call, DataInvalid)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_injected_allocation_failure(case):
    """tests/test_gpu_lifetime.py's injection, with room for the two calls' allocations"""
    want = bits(case.run())
    base = tl.baseline()
    t0 = tl.total()
    assert bits(case.run()) == want
    n_allocs = tl.total() - t0
    assert tl.live() == base
    print("%s: %d device allocations" % (case.name, n_allocs))
    assert 0 < n_allocs <= MAX_ALLOCS
    for k in range(n_allocs):
        assert _lib.fail_alloc_at(k) == -1
        try:
            with pytest.raises(tl.FAILED):
                case.run()
        finally:
            pending = _lib.fail_alloc_at(-1)
        assert pending == -1, "allocation %d: the arm is still set" % k
        assert tl.live() == base, "allocation %d" % k
    gc.collect()
    assert bits(case.run()) == want and tl.live() == base
