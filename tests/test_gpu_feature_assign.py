"""ek_feat_assign_nearest (csrc/ek_feat_assign.hip: every sample against a
table of centers in one launch) against the ORACLE's scan
(oracle/features.py::assign_to_nearest_center, pinned to the reference's
compiled module by test_features.py) -- never against another device form,
except for the bulk of the large case, which the per-center device loop
covers.  Exact throughout: labels equal, float64 distances equal as values with
the same sign of zero, the same dtypes.  No tolerance anywhere."""
import os
import re

import numpy as np
import pytest

from oracle import features as of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = {"euclidean": of.euclidean, "manhattan": of.manhattan,
          "hamming": of.hamming}
MID = {"euclidean": 0, "manhattan": 1, "hamming": 2}
TC = int(re.search(r"#define\s+FA_TC\s+(\d+)", open(os.path.join(
    ROOT, "enspara_amd", "csrc", "ek_feat_assign.hip")).read()).group(1))

FS = (1, 31, 32, 33, 129, 2047, 2049, 4100)
NS = (1, 255, 256, 257, 1000)
KS = (1, TC - 1, TC, TC + 1, 255, 256, 257, 1030, 0)


def _device(name):
    from enspara_amd.geometry import libdist
    return libdist.hamming if name == "hamming" else name


def _same(got, want):
    """equal values (NaN where NaN), equal dtypes, the same sign of zero"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got, want)
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(np.signbit(got[ok]), np.signbit(want[ok]))


def _check(name, X, C, forms=("util", "resident", "bound")):
    """util's entry, the module function, a bound matrix"""
    from enspara_amd.cluster import util
    from enspara_amd.geometry import libdist
    wa, wd = of.assign_to_nearest_center(X, C, ORACLE[name])
    assert wa.dtype == np.int64 and wd.dtype == np.float64
    what = (name, X.dtype, X.shape, np.shape(C))
    if "util" in forms and len(C):
        a, d = util.assign_to_nearest_center(X, C, _device(name))
        _same(a, wa), _same(d, wd)
    if "resident" in forms:
        a, d = libdist.assign_nearest_resident(X, MID[name], C)
        _same(a, wa), _same(d, wd)
    if "bound" in forms:
        a, d = getattr(libdist, name).bind(X).assign_nearest(C)
        _same(a, wa), _same(d, wd)
    return wa, wd, what


def _ints(rng, dt, shape):
    info = np.iinfo(dt)
    lo, hi = max(int(info.min), -2 ** 26), min(int(info.max), 2 ** 26)
    return rng.randint(lo, hi, size=shape, dtype=np.int64).astype(dt)


def _shapes():
    """(F, n, K): every F with every K of the first center tiles, every K with
    the feature counts up to 129, every n throughout; two whole-table cases at
    the largest F"""
    out = []
    small_k = (1, TC - 1, TC, TC + 1, 0)
    for i, F in enumerate(FS):
        for off in (0, 2):
            out.append((F, NS[(i + off) % 5], small_k[(i + off) % 5]))
    for i, K in enumerate(KS):
        for off in (0, 2):
            out.append((FS[(i + off) % 5], NS[(i + 2 * off + 1) % 5], K))
    return out


def test_grid():
    """n, K and F across every tile and slice: 256 samples, TC centers, the
    staged feature slice, more features than any chunk; float32 and float64 in
    their own arithmetic, the integer types through float64, hamming on the
    integers at the extremes of each type.  Every dtype takes the whole list of
    shapes rotated by its position."""
    rng = np.random.RandomState(131)
    float_dts = (np.float32, np.float64, np.int8, np.int16, np.int32, np.int64)
    ham_dts = (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32,
               np.int64, np.uint64)
    shapes = _shapes()
    assert {s[0] for s in shapes} == set(FS) and {s[1] for s in shapes} == set(NS)
    assert {s[2] for s in shapes} == set(KS)
    for k, dt in enumerate(float_dts):
        for q, (F, n, K) in enumerate(shapes):
            n = NS[(NS.index(n) + k) % 5]
            if np.issubdtype(dt, np.floating):
                X = rng.normal(size=(n, F)).astype(dt)
                C = rng.normal(size=(K, F)).astype(dt)
            else:
                X = _ints(rng, dt, (n, F))
                C = _ints(rng, dt, (K, F))
            if K:
                C[:, ::2] = X[rng.randint(n), ::2]       # half the features on a sample
                C[K // 2] = X[n // 2]                   # one center ON a sample
            forms = (("util", "resident", "bound") if q % 4 == 0 else ("util",)
                     if K else ("resident",))
            for name in ("euclidean", "manhattan"):
                _, wd, _ = _check(name, X, C, forms)
                if K:
                    assert wd[n // 2] == 0.0
                else:
                    assert np.isposinf(wd).all()
    # whole tables at the largest feature counts (several slices, several tiles)
    for dt in (np.float32, np.float64):
        for F, n, K in ((2049, 257, 257), (4100, 255, 1030)):
            X = rng.normal(size=(n, F)).astype(dt)
            C = rng.normal(size=(K, F)).astype(dt)
            C[K - 1] = X[0]
            for name in ("euclidean", "manhattan"):
                wa, wd, _ = _check(name, X, C, ("util",))
                assert wa[0] == K - 1 and wd[0] == 0.0
    for k, dt in enumerate(ham_dts):
        info = np.iinfo(dt)
        vals = np.array([info.min, info.max, 1], dtype=dt)
        for q, (F, n, K) in enumerate(shapes):
            n = NS[(NS.index(n) + k) % 5]
            X = vals[rng.randint(0, 3, size=(n, F))]
            C = vals[rng.randint(0, 3, size=(K, F))]
            if K:
                C[K // 2] = X[n // 2]
            _, wd, _ = _check("hamming", X, C, ("util",) if K else ("resident",))
            if K:
                assert wd[n // 2] == 0.0


def test_ties_lowest_index_wins():
    """duplicated centers and small-integer data: many centers at the same
    distance, across center tiles and (few samples, many centers) across the
    parts the centers are split into"""
    rng = np.random.RandomState(132)
    for dt, names in ((np.float32, ("euclidean", "manhattan")),
                      (np.float64, ("euclidean", "manhattan")),
                      (np.int64, ("euclidean", "manhattan", "hamming"))):
        for n, K, F in ((700, 5 * TC + 3, 6), (40, 1030, 4), (3000, 300, 9)):
            X = rng.randint(0, 3, size=(n, F)).astype(dt)
            base = X[rng.randint(0, n, size=K // 3 + 1)]
            C = np.concatenate([base, base, base])[:K]    # every center 2-3 times
            C = C[np.r_[rng.permutation(K // 2), np.arange(K // 2, K)]]
            for name in names:
                wa, wd, _ = _check(name, X, C, ("util", "bound"))
                assert (wd == 0).sum() >= min(n, len(base)) // 2
                # the oracle's label is the first minimum: no earlier center as near
                first = {}
                for i, c in enumerate(map(bytes, C)):
                    first.setdefault(c, i)
                assert all(first[bytes(C[a])] == a for a in wa)


def test_value_edges():
    """NaN and +-inf in samples and in centers; rows whose every distance is
    NaN keep label 0 / +inf; float32 cancellation at 1e4, overflowing squares,
    subnormals, signed zeros"""
    rng = np.random.RandomState(133)
    for dt in (np.float32, np.float64):
        X = rng.normal(size=(1500, 5)).astype(dt)
        X[rng.rand(1500, 5) < 0.03] = np.inf
        X[rng.rand(1500, 5) < 0.03] = -np.inf
        X[rng.rand(1500, 5) < 0.02] = np.nan
        X[11] = np.nan
        C = X[rng.randint(0, 1500, size=70)].copy()
        C[0] = np.nan                                    # a center that is never taken
        C[5] = rng.normal(size=5)
        for name in ("euclidean", "manhattan"):
            wa, wd, _ = _check(name, X, C)
            assert wa[11] == 0 and np.isposinf(wd[11])
            assert not np.isnan(wd).any() and (wa[np.isfinite(wd)] != 0).all()
        # every center NaN: label 0 / +inf everywhere
        wa, wd, _ = _check("euclidean", X, np.full((TC + 1, 5), np.nan, dtype=dt))
        assert (wa == 0).all() and np.isposinf(wd).all()
    fam = [(1e4 + 1e-3 * rng.normal(size=(3000, 8))).astype(np.float32)]
    big = rng.normal(size=(2000, 4)) * np.where(rng.rand(2000, 1) < 0.5, 3e19, 1.0)
    fam.append(big.astype(np.float32))
    for dt, tiny, sq in ((np.float32, 1e-40, 1e-20), (np.float64, 1e-310, 1e-160)):
        v = rng.normal(size=(2500, 6))
        fam.append((v * np.where(rng.rand(2500, 1) < 0.3, 1.0, np.where(
            rng.rand(2500, 6) < 0.5, tiny, sq))).astype(dt))
        vals = np.array([-0.0, 0.0, 1.0, -1.0], dtype=dt)
        fam.append(vals[rng.randint(0, 4, size=(2000, 6))])
    v = (2 ** 26 - rng.randint(0, 4, size=(2000, 5))) * rng.choice([-1, 1], size=(2000, 5))
    fam.append(v.astype(np.int64))
    for X in fam:
        C = X[rng.randint(0, len(X), size=2 * TC + 5)]
        for name in ("euclidean", "manhattan"):
            _check(name, X, C, ("util",))
    wa, wd, _ = _check("euclidean", fam[1], fam[1][:40], ("resident",))
    assert np.isposinf(wd).any()


def test_no_per_center_call(monkeypatch):
    """with the one-point-against-all entry made to raise, the scan and
    predict() still run: nothing calls the metric once per center"""
    from enspara_amd.cluster import util
    from enspara_amd.cluster.kcenters import KCenters
    from enspara_amd.geometry import libdist
    rng = np.random.RandomState(134)
    X = rng.normal(size=(5000, 12)).astype(np.float32)
    Y = rng.normal(size=(3000, 12)).astype(np.float32)

    def boom(*a, **kw):
        raise AssertionError("one launch and read-back per center")
    monkeypatch.setattr(libdist._Resident, "distance", boom)
    C = X[:77]
    a, d = util.assign_to_nearest_center(X, C, "euclidean")
    wa, wd = of.assign_to_nearest_center(X, C, of.euclidean)
    _same(a, wa), _same(d, wd)
    est = KCenters("euclidean", n_clusters=40).fit(X)
    pred = est.predict(Y)
    assert len(est.centers_) == 40
    wa, wd = of.assign_to_nearest_center(Y, np.array(est.centers_), of.euclidean)
    _same(pred.assignments, wa), _same(pred.distances, wd)


def test_warm_start_kcenters(monkeypatch):
    """kcenters(init_centers=...) takes the scan and equals the same call
    around the oracle's callable"""
    from enspara_amd.cluster.kcenters import kcenters
    from enspara_amd.geometry import libdist
    calls = []
    real = libdist.assign_nearest_resident

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(libdist, "assign_nearest_resident", counted)
    rng = np.random.RandomState(135)
    for dt, name in ((np.float32, "euclidean"), (np.float64, "manhattan"),
                     (np.int32, "euclidean")):
        X = (rng.normal(size=(4000, 7)) * 3).astype(dt)
        C = [X[5].copy(), X[2000].copy(), X[5].copy(), (X[5] + 100).astype(dt),
             X[3999].copy()]
        before = len(calls)
        got = kcenters(X, name, n_clusters=20, init_centers=C)
        assert len(calls) == before + 1, "the warm start did not take the scan"
        want = kcenters(X, ORACLE[name], n_clusters=20, init_centers=C)
        assert len(calls) == before + 1
        assert list(got.center_indices) == list(want.center_indices)
        _same(got.assignments, want.assignments)
        _same(got.distances, want.distances)


def test_sharded_store_state_continues():
    """one device shard: FeatureStore.assign_nearest leaves the oracle's state
    on the device, and ek_feat_kcenters_step runs that follow give what the
    single-handle run from the same state gives"""
    import torch
    from enspara_amd.geometry import libdist
    rng = np.random.RandomState(136)
    X = rng.normal(size=(6000, 9)).astype(np.float32)
    C = X[[7, 4000, 7, 5999]]
    wa, wd = of.assign_to_nearest_center(X, C, of.euclidean)
    stream = torch.cuda.Stream()
    with libdist.FeatureStore.from_array(X, 0, stream=stream.cuda_stream) as st:
        d, a = st.assign_nearest(0, C)
        _same(d, wd), _same(a, wa.astype(np.int32))
        d2, a2 = st.download_state()
        _same(d2, wd), _same(a2, wa.astype(np.int32))
        with torch.cuda.stream(stream):
            rec = torch.zeros(st.record_bytes, dtype=torch.uint8, device="cuda")
            st.reset_history()
            st.local_candidate(rec.data_ptr())
            for label in range(4, 16):
                st.kcenters_step(0, rec.data_ptr(), 1, label, 0.0, rec.data_ptr())
            idx, _, n_done = st.history(4, 12)
        sd, sa = st.download_state()
    assert n_done == 16
    centers, rd, ra_, _ = libdist.kcenters_resident(X, 0, 4, 12, 0.0, wd,
                                                    wa.astype(np.int32))
    assert list(idx) == list(centers)
    _same(sd, rd), _same(sa, ra_)
    # an empty center table: label 0 / +inf
    with libdist.FeatureStore.from_array(X[:300], 1) as st:
        d, a = st.assign_nearest(1, np.zeros((0, 9), dtype=np.float32))
        assert (a == 0).all() and np.isposinf(d).all()


def _loop(bound):
    """the per-center device loop: a callable without ``device_metric_id``"""
    return lambda A, y: bound(A, y)


@pytest.mark.parametrize("dt,name", [(np.float32, "euclidean"),
                                     (np.float64, "manhattan")])
def test_large(dt, name):
    """200 000 x 64 against 1000 centers: the oracle on 5000 random rows plus
    the first and the last tile, the per-center device loop on all rows"""
    from enspara_amd.cluster import util
    from enspara_amd.geometry import libdist
    rng = np.random.RandomState(137)
    n, F, K = 200003, 64, 1000
    X = rng.normal(size=(n, F)).astype(dt)
    C = X[rng.choice(n, size=K, replace=False)].copy()
    C[K // 2:] += (rng.normal(size=(K - K // 2, F)) * 0.1).astype(dt)
    a, d = util.assign_to_nearest_center(X, C, name)
    rows = np.unique(np.r_[rng.choice(n, size=5000, replace=False), np.arange(256),
                           np.arange(n - n % 256, n)])
    wa, wd = of.assign_to_nearest_center(X[rows], C, ORACLE[name])
    _same(a[rows], wa), _same(d[rows], wd)
    la, ld = util.assign_to_nearest_center(
        X, C, _loop(getattr(libdist, name).bind(X)))
    _same(a, la), _same(d, ld)
    assert (d == 0).sum() >= K // 2
