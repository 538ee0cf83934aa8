"""enspara_amd.geometry.dye_lifetimes and explicit_r0_calc.pair_table on the device
(csrc/ek_dye_pair.hip), through the public functions and so through the C ABI.

No expected value comes from a device call.  The pair table is held to the np.longdouble
model within the bounds derived in tests/_numpy_dye_lifetimes.py, and prints
the largest ratio to them.  Steps, outcomes and trajectories must be ``==`` the float64
model's.  That is an argument in three parts: (a) the largest gap between the device's table
and the model's decay CDFs, (b) every chain's smallest distance between a decay draw and a
CDF value in the model, (c) gap < margin / 2 for every chain of the fixed seeds, which is a
condition on the inputs and is asserted, no chain left out; then both sides decide every
draw alike.  Hops and initial states search the host's own CDF bits and need no argument.

Shapes.  The excitation kernel has workgroups of 256 lanes and waves of 64, the list of live
excitations is compacted per wave: samples 1, 63, 64, 65, 130 bracket the wave, and with three
problems the workgroup; step caps 1, 3, 64 cut the pairs of doubles of a Philox call at
both phases and force hundreds of launches and compactions; the default is one launch."""
import functools
import gc
import os

import numpy as np
import pytest

import _numpy_dye_lifetimes as nd
import test_gpu_lifetime as tl
from _lifetime_cases import Case, bits
from enspara_amd import _lib
from enspara_amd.exception import DataInvalid
from enspara_amd.geometry import dye_lifetimes as dl
from enspara_amd.geometry import explicit_r0_calc as r0c

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "dye_lifetimes_golden.npz"))
PARAMS = tuple(G["dye_params"])
LAG = float(G["lagtime"])
SEED = 0x5EED0123456789AB
U = 2.0 ** -53
P32 = 1 << 32


# ---- problems: (d_coords, d_T, d_eqs, a_coords, a_T, a_eqs, lag) -------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    return tuple(G["mc_" + k] for k in ("d_coords", "d_T", "d_eqs", "a_coords", "a_T",
                                        "a_eqs")) + (LAG,)


@functools.lru_cache(maxsize=None)
def _long():
    """33 x 17, far apart, lag 0.02 ns: a mean of about 200 steps"""
    rng = np.random.RandomState(11)
    dT, de = nd.random_msm(rng, 33, 5)
    aT, ae = nd.random_msm(rng, 17, 4)
    return (nd.random_coords(rng, 33, (0, 0, 0)), dT, de,
            nd.random_coords(rng, 17, (9.0, 1.0, 0.5)), aT, ae, 0.02)


@functools.lru_cache(maxsize=None)
def _clashing():
    """12 x 9 with clashing states: empty rows, nothing enters them, eq prob 0"""
    rng = np.random.RandomState(12)
    dT, de = nd.random_msm(rng, 12, 4, empty=(0, 5, 11))
    aT, ae = nd.random_msm(rng, 9, 3, empty=(3,))
    return (nd.random_coords(rng, 12, (0, 0, 0)), dT, de,
            nd.random_coords(rng, 9, (5.0, 0, 0)), aT, ae, LAG)


@functools.lru_cache(maxsize=None)
def _close():
    """the golden's 3 x 2 pair less than 1 nm apart: the renormalised branch"""
    rng = np.random.RandomState(13)
    dT, de = nd.random_msm(rng, 3, 3)
    aT, ae = nd.random_msm(rng, 2, 2)
    return G["cl_d_coords"], dT, de, G["cl_a_coords"], aT, ae, LAG


def _problem(q):
    return dl.problem(q[0], q[1], q[2], q[3], q[4], q[5], PARAMS, q[6])


def _K(q):
    return nd.consts(PARAMS, q[6])


@functools.lru_cache(maxsize=None)
def _model(name, n, first_chain=0, seed=SEED):
    q = PROBLEMS[name]()
    return nd.resolve(q[0], q[1], q[2], q[3], q[4], q[5], _K(q), n, nd.PhiloxUniforms(seed),
                      first_chain=first_chain)


PROBLEMS = {"golden": _golden, "long": _long, "clashing": _clashing, "close": _close}


@functools.lru_cache(maxsize=None)
def _gap(name):
    """(a): the device's table against the float64 model's, largest CDF and FE gaps"""
    q = PROBLEMS[name]()
    with dl.DyePair(_problem(q)) as pair:
        _, _, FE, cdf = pair.pair_table(0)
    _, _, mFE, mcdf = nd.table(q[0], q[3], _K(q))
    return float(np.abs(cdf - mcdf).max()), float(np.abs(FE - mFE).max())


def _assert_decided(name, margins):
    """(c): every chain's margin is more than twice the table's gap"""
    gap = _gap(name)[0]
    print("%s: table gap %.3g, smallest margin %.3g over %d chains"
          % (name, gap, margins.min(), len(margins)))
    assert np.all(gap < margins / 2)


def _assert_equal(got, want, n=None):
    steps, codes, dtr, atr = got
    n = len(steps) if n is None else n
    assert steps.dtype == np.int64 and codes.dtype == np.int8
    assert np.array_equal(steps, want[0][:n]) and np.array_equal(codes, want[1][:n])
    assert len(dtr) == len(atr) == n
    for j in range(n):
        assert np.array_equal(dtr[j], want[2][j]) and np.array_equal(atr[j], want[3][j])


# ---- the pair table --------------------------------------------------------------------------
@pytest.mark.parametrize("nd_,na_", [(1, 1), (7, 5), (63, 65), (129, 257)])
def test_pair_table_within_the_derived_bounds(nd_, na_):
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    rng = np.random.RandomState(nd_ * 1000 + na_)
    dc = nd.random_coords(rng, nd_, (0, 0, 0))
    ac = nd.random_coords(rng, na_, (4.0, 1.0, 0))
    ac[0, 0:3] = dc[0, 0:3] + [0.5, 0.3, -0.2]      # a close pair: the renormalised branch
    ac[0, 3:6] = dc[0, 3:6] + [0.4, 0.3, -0.1]
    if nd_ > 1:                                      # perpendicular dipoles: k2 = 0 exactly
        dc[-1, 3:9] = [0, 0, 0, 0.3, 0, 0]
        ac[-1, 3:9] = [0, 0, 2.0, 0, 0.2, 0]
    K = nd.consts(PARAMS, LAG)
    k2, r, FE, cdf = r0c.pair_table(dc, ac, PARAMS, LAG)
    assert k2.shape == r.shape == FE.shape == (nd_, na_) and cdf.shape == (nd_, na_, 3)
    xk2, xr, xFE, xcdf = nd.table(dc, ac, K, dtype=np.longdouble)
    assert cdf[0, 0, 2] == 1.0 and float(xcdf[0, 0, 2]) == 1.0
    if nd_ > 1:
        assert xk2[-1, -1] == 0 and k2[-1, -1] <= nd.K2_ABS and FE[-1, -1] <= 8 * U
    ratios = {
        "k2": np.abs(k2 - xk2) / nd.K2_ABS,
        "r": np.abs(r - xr) / (nd.R_REL * xr),
        "FE": np.abs(FE - xFE) / nd.fe_bound(xk2, xr, K),
        "cdf": np.abs(cdf - xcdf) / nd.cdf_bound(xr, K)[..., None],
    }
    print("largest ratio to the bound, %d x %d: %s" % (
        nd_, na_, ", ".join("%s %.3g" % (k, float(v.max())) for k, v in ratios.items())))
    for k, v in ratios.items():
        assert np.all(v <= 1), k
    assert np.all(np.diff(cdf, axis=2) >= 0) and np.all(cdf <= 1) and np.all(cdf >= 0)
    # without a lag time: the same geometry, no CDF
    assert bits(r0c.pair_table(dc, ac, PARAMS)) == bits((k2, r, FE))


# ---- integer results -------------------------------------------------------------------------
def test_golden_pair_300_chains():
    want = _model("golden", 300)
    _assert_decided("golden", want[4])
    assert 5 < want[0].mean() < 15
    q = _golden()
    got = dl.resolve_excitations(q[1], q[4], q[2], q[5], q[0], q[3], PARAMS, q[6],
                                 n_samples=300, random_state=SEED)
    _assert_equal(got, want)
    assert dl.last_seed == SEED and dl.last_timing().shape == (3,)


@pytest.mark.parametrize("cap", [1, 3, 64, None])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_long_pair_every_cut(n, cap):
    want = _model("long", 130)
    _assert_decided("long", want[4])
    assert 120 < want[0].mean() < 320
    with dl.DyePair(_problem(_long())) as pair:
        got = pair.resolve(n, random_state=SEED, return_trajectories=True, step_cap=cap)
        plain = pair.resolve(n, random_state=SEED, step_cap=cap)
    _assert_equal((got[0][0], got[1][0], got[2], got[3]), want, n=n)
    assert bits(plain) == bits(got[:2])


def test_first_chain_splits():
    want = _model("long", 130)
    with dl.DyePair(_problem(_long())) as pair:
        a = pair.resolve(50, random_state=SEED, return_trajectories=True)
        b = pair.resolve(80, random_state=SEED, first_chain=50, return_trajectories=True)
    steps = np.concatenate([a[0][0], b[0][0]])
    codes = np.concatenate([a[1][0], b[1][0]])
    _assert_equal((steps, codes, list(a[2]) + list(b[2]), list(a[3]) + list(b[3])), want)


def test_batch_of_three_problems():
    names, n = ["golden", "clashing", "close"], 70
    problems = [_problem(PROBLEMS[k]()) for k in names]
    with dl.DyePair(problems) as pair:
        got = pair.resolve(n, random_state=SEED, return_trajectories=True, step_cap=2)
        again = pair.resolve(n, random_state=SEED, return_trajectories=True)
    assert bits(got) == bits(again)                 # one seed, byte for byte
    assert got[0].shape == got[1].shape == (3, n) and len(got[2]) == 3 * n
    with dl.DyePair(problems, chunk_bytes=1) as pair:          # a device call per problem
        assert len(pair._chunks(n)) == 3
        assert bits(pair.resolve(n, random_state=SEED, return_trajectories=True)) == bits(got)
    for p, name in enumerate(names):
        want = _model(name, n, first_chain=p * P32)
        _assert_decided(name, want[4])
        rows = slice(p * n, (p + 1) * n)
        _assert_equal((got[0][p], got[1][p], list(got[2])[rows], list(got[3])[rows]), want)
        with dl.DyePair(problems[p]) as one:
            alone = one.resolve(n, random_state=SEED, first_chain=p * P32,
                                return_trajectories=True)
        _assert_equal((alone[0][0], alone[1][0], alone[2], alone[3]), want)
    # the clashing states are never visited; the close pair never stays excited on a
    # renormalised pair of states
    q = _clashing()
    visited = np.concatenate(list(got[2])[n:2 * n])
    assert not np.isin(visited, np.flatnonzero(q[2] == 0)).any()
    assert G["cl_raised"].any() and got[0][2].min() == 1


def test_trajectory_buffer_is_cut_into_groups():
    """more states than the trajectory buffer of a side holds (2^24): two groups of samples,
    equal to two calls that fit one group each"""
    n = 100000
    with dl.DyePair(_problem(_long())) as pair:
        whole = pair.resolve(n, random_state=SEED, return_trajectories=True)
        assert int((whole[0] + 1).sum()) > 1 << 24
        half = [pair.resolve(n // 2, random_state=SEED, first_chain=k * (n // 2),
                             return_trajectories=True) for k in range(2)]
    assert max(int((h[0] + 1).sum()) for h in half) < 1 << 24
    assert np.array_equal(whole[0][0], np.concatenate([h[0][0] for h in half]))
    assert np.array_equal(whole[1][0], np.concatenate([h[1][0] for h in half]))
    for k, traj in ((2, whole[2]), (3, whole[3])):
        flat = np.concatenate([np.asarray(h[k]._data) for h in half])
        assert np.array_equal(np.asarray(traj._data), flat)
    assert np.array_equal(np.asarray(whole[2]._data)[:200],
                          np.concatenate(_model("long", 130)[2])[:200])


# ---- static and isotropic ----------------------------------------------------------------------
def test_static_and_isotropic():
    q, n = _golden(), 500
    K = _K(q)
    d_eqs = G["st_d_eqs"]
    uni = nd.PhiloxUniforms(SEED)
    acc, ds, as_, margin = nd.static(q[0], d_eqs, q[3], q[5], K, n, uni, first_chain=7)
    fe_gap = _gap("golden")[1]
    print("static: FE gap %.3g, smallest |coin - FE| %.3g" % (fe_gap, margin.min()))
    assert np.all(fe_gap < margin / 2)
    prob = dl.problem(q[0], q[1], d_eqs, q[3], q[4], q[5], PARAMS, q[6])
    with dl.DyePair(prob) as pair:
        codes, gd, ga = pair.static(n, random_state=SEED, first_chain=7, return_states=True)
        iso = pair.isotropic(n, random_state=SEED, first_chain=7)[0]
        # the static treatment of chain c sees the initial states of the Monte Carlo of chain c
        mc = pair.resolve(n, random_state=SEED, first_chain=7, return_trajectories=True)
    assert codes.dtype == np.int8 and np.array_equal(codes[0], acc * 2)
    assert np.array_equal(gd[0], ds) and np.array_equal(ga[0], as_) and not np.any(gd[0] == 2)
    assert np.array_equal([t[0] for t in mc[2]], ds) and np.array_equal([t[0] for t in mc[3]], as_)
    assert bits(dl.explicit_static_dyes(d_eqs, q[5], q[0], q[3], PARAMS, n_samples=n,
                                        random_state=SEED, first_chain=7)) == bits(codes[0])
    macc, mk2, mFE, meqs, mavg, mmargin = nd.isotropic(q[0], d_eqs, q[3], q[5], K, n, uni,
                                                       first_chain=7)
    transfers, k2s, FEs, eqs, avg = iso
    assert np.array_equal(eqs, meqs) and np.array_equal(eqs, G["iso_eqs"])
    assert np.all(np.abs(k2s - mk2) <= 2 * nd.K2_ABS) and np.all(np.abs(FEs - mFE) <= fe_gap)
    assert abs(avg - mavg) <= fe_gap + 4 * U and np.all(fe_gap + 4 * U < mmargin / 2)
    assert np.array_equal(transfers, macc * 2)
    full = dl.fully_averaged_explicit_dyes(d_eqs, q[5], q[0], q[3], PARAMS, n_samples=n,
                                           random_state=SEED, first_chain=7)
    assert bits(full[1:]) == bits(list(iso[:4])) and not full[0].any()


def test_calc_lifetimes():
    q, n = _clashing(), 40
    rng = np.random.RandomState(5)
    d_counts, a_counts = rng.randint(1, 30, size=(12, 12)), rng.randint(1, 30, size=(9, 9))
    d_keep, a_keep = np.array([1, 2, 3, 4, 6, 7, 8, 9, 10]), np.array([0, 1, 2, 4, 5, 6, 7, 8])
    args = (q[0], d_counts, d_keep, q[3], a_counts, a_keep, PARAMS, LAG)
    lifetimes, outcomes = dl.calc_lifetimes(*args, n_samples=n, random_state=SEED)
    d_tp, d_eq, _ = dl.make_dye_msm(d_counts, d_keep)
    a_tp, a_eq, _ = dl.make_dye_msm(a_counts, a_keep)
    assert d_eq[[0, 5, 11]].sum() == 0 and not d_tp[[0, 5, 11]].any() and abs(d_eq.sum() - 1) < 1e-9
    want = nd.resolve(q[0], d_tp, d_eq, q[3], a_tp, a_eq, nd.consts(PARAMS, LAG), n,
                      nd.PhiloxUniforms(SEED))
    with dl.DyePair(dl.problem(q[0], d_tp, d_eq, q[3], a_tp, a_eq, PARAMS, LAG)) as pair:
        gap = float(np.abs(pair.pair_table(0)[3] - nd.table(q[0], q[3], nd.consts(PARAMS, LAG))[3])
                    .max())
    assert np.all(gap < want[4] / 2)
    assert np.array_equal(lifetimes, want[0].astype(float) * LAG)
    assert list(outcomes) == [nd.OUTCOMES[c] for c in want[1]]
    unlabelled = (q[0], d_counts, [], q[3], a_counts, a_keep)
    many = dl.calc_lifetimes_many([args[:6], unlabelled, args[:6]], PARAMS, LAG, n_samples=n,
                                  random_state=SEED)
    assert bits(many[0]) == bits((lifetimes, outcomes)) and many[1] == ([], [])
    third = nd.resolve(q[0], d_tp, d_eq, q[3], a_tp, a_eq, nd.consts(PARAMS, LAG), n,
                       nd.PhiloxUniforms(SEED), first_chain=2 * P32)
    assert np.all(gap < third[4] / 2)
    assert np.array_equal(many[2][0], third[0].astype(float) * LAG)
    for treatment in ("static", "isotropic"):
        lt, oc = dl.calc_lifetimes(*args, n_samples=n, dye_treatment=treatment, random_state=SEED)
        assert not lt.any() and set(oc) <= {"radiative", "energy_transfer"}


# ---- raises ------------------------------------------------------------------------------------
def _empty_row_problem():
    q = _clashing()
    eqs = np.zeros(12)
    eqs[5] = 1.0                    # every donor starts on a clashing state
    return dl.problem(q[0], q[1], eqs, q[3], q[4], q[5], PARAMS, LAG)


def _never_decays():
    q = _golden()
    return dl.problem(q[0], q[1], q[2], q[3], q[4], q[5], PARAMS, 1e-7)


def _raise_empty_row():
    with dl.DyePair(_empty_row_problem()) as pair:
        pair.resolve(10, random_state=SEED, return_trajectories=True)


def _raise_max_steps():
    with dl.DyePair(_never_decays()) as pair:
        pair.resolve(10, random_state=SEED, max_steps=50, step_cap=16)


def test_raises():
    with pytest.raises(DataInvalid, match="donor of problem 0 stood on state 5"):
        _raise_empty_row()
    with pytest.raises(DataInvalid, match=r"Sample 0 of problem 0 \(chain 0\) is still excited "
                                          "after 50 steps"):
        _raise_max_steps()
    with dl.DyePair([_problem(_golden()), _never_decays()]) as pair:
        with pytest.raises(DataInvalid, match=r"Sample 0 of problem 1 \(chain %d\)" % P32):
            pair.resolve(3, random_state=SEED, max_steps=50)


# ---- resources --------------------------------------------------------------------
def _three():
    return [_problem(PROBLEMS[k]()) for k in ("golden", "clashing", "close")]


def _open_two_chunks():
    ps = _three()
    return dl.DyePair(ps, chunk_bytes=ps[0].bytes + ps[1].bytes + 2 * 32 * 20)


def _use(pair):
    return (pair.resolve(20, random_state=SEED, return_trajectories=True, step_cap=4),
            pair.static(20, random_state=SEED, return_states=True),
            pair.isotropic(20, random_state=SEED), pair.pair_table(len(pair.problems) - 1))


def _use_two_chunks(pair):
    """(every chunk: a handle, the first pass with compactions, the replay)"""
    return pair.resolve(20, random_state=SEED, return_trajectories=True, step_cap=4)


def _q():
    q = _golden()
    return (q[1], q[4], q[2], q[5], q[0], q[3], PARAMS, q[6])


CASES = [
    Case("DyePair, two chunks", open=_open_two_chunks, use=_use_two_chunks),
    Case("DyePair, resident", open=lambda: dl.DyePair(_problem(_golden())), use=_use),
    Case("resolve_excitations", fn=lambda: dl.resolve_excitations(*_q(), n_samples=20,
                                                                  random_state=SEED)),
    Case("explicit_static_dyes", fn=lambda: dl.explicit_static_dyes(
        _q()[2], _q()[3], _q()[4], _q()[5], PARAMS, n_samples=20, random_state=SEED)),
    Case("fully_averaged_explicit_dyes", fn=lambda: dl.fully_averaged_explicit_dyes(
        _q()[2], _q()[3], _q()[4], _q()[5], PARAMS, n_samples=20, random_state=SEED)),
    Case("pair_table", fn=lambda: r0c.pair_table(_q()[4], _q()[5], PARAMS, LAG)),
]
MAX_ALLOCS = 80         # two chunks: twice a handle (13), a first pass (11), a replay (7)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_balance(case):
    assert len(_open_two_chunks()._chunks(20)) == 2
    tl.test_balance(case)


@pytest.mark.parametrize("call", [_raise_empty_row, _raise_max_steps],
                         ids=["empty row", "max_steps"])
def test_raise_paths_balance(call):
    tl.test_raise_paths_balance(call.__name__, call, DataInvalid)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_injected_allocation_failure(case):
    """tests/test_gpu_lifetime.py's injection, with room for the two chunks' allocations"""
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
