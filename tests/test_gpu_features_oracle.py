"""The feature-space kernels (csrc/ek_features.hip: libdist.euclidean /
manhattan / hamming; ek_feat_kcenters.hip: the resident k-centers loop;
ek_feat_pam.hip: the resident PAM sweep)
against the ORACLE (oracle/features.py, pinned to the reference's compiled
module by test_features.py::test_oracle_matches_reference_libdist) -- never
against another device form -- at the forms the library takes on real data:
feature counts across every staging chunk, partial tiles, every input dtype,
the value edges of IEEE arithmetic, a matrix loaded in more than one chunk
whose arg-max runs over thousands of block maxima and whose PAM sweep takes
windows by size, more than 256 medoids (the tiled nearest search in several
chunks), windows of every width, and the resident loops one feature past
the target's staging chunk.  Exact throughout: float64 distances and
labels equal, the same centers and medoids, the same dtypes, the random stream
left in the same place."""
import numpy as np
import pytest

from oracle import features as of

pytestmark = pytest.mark.gpu

ORACLE = {"euclidean": of.euclidean, "manhattan": of.manhattan,
          "hamming": of.hamming}


def _device(name):
    """what a caller passes for the metric: the string for euclidean /
    manhattan, the library's callable for hamming (no string names it)"""
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


def _check_distance(name, X, y, forms=("call", "bind", "out", "bind_out")):
    """the unbound call, a bound matrix, out= on both"""
    from enspara_amd.geometry import libdist
    f = getattr(libdist, name)
    want = ORACLE[name](X, y)
    assert want.dtype == np.float64
    if "call" in forms:
        _same(f(X, y), want)
    if "bind" in forms:
        _same(f.bind(X)(X, y), want)
    if "out" in forms:
        out = np.full(len(X), -7.0)
        assert f(X, y, out=out) is out
        _same(out, want)
    if "bind_out" in forms:
        out = np.full(len(X), -7.0)
        assert f.bind(X)(X, y, out=out) is out
        _same(out, want)
    return want


@pytest.fixture
def resident_calls(monkeypatch):
    """counts the k-centers runs that took the device-resident loop"""
    from enspara_amd.geometry import libdist
    calls = []
    real = libdist.kcenters_resident

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(libdist, "kcenters_resident", counted)
    return calls


def _check_kcenters(name, X, resident_calls, **kw):
    """the resident loop against the reference-shaped host loop around the
    oracle's callable"""
    from enspara_amd.cluster.kcenters import kcenters
    before = len(resident_calls)
    got = kcenters(X, _device(name), **kw)
    assert len(resident_calls) == before + 1, "the resident loop did not run"
    want = kcenters(X, ORACLE[name], **kw)
    assert len(resident_calls) == before + 1
    assert list(got.center_indices) == list(want.center_indices), (name, X.dtype)
    _same(got.assignments, want.assignments)
    _same(got.distances, want.distances)
    return want


def _sweeps(X, name, inds, a, d, props, seed, n_sweeps, monkeypatch):
    """n_sweeps PAM sweeps on the device (dev=1) and in the reference-shaped
    host loop around the oracle's callable (dev=0, its nearest-center search
    in the oracle's vectorised form); checks everything the sweep returns"""
    from enspara_amd.cluster import kmedoids as km
    from enspara_amd.cluster import util
    assert km._feature_sweep_applies(X, util._get_distance_method(_device(name)), d,
                                     props, a)
    out = {}
    for dev in (1, 0):
        rs = np.random.RandomState(seed)
        ii, dd, aa = list(inds), d.copy(), a.copy()
        with monkeypatch.context() as mp:
            mp.setattr(km, "PAM_FEATURE_DEVICE", 1)
            if not dev:
                mp.setattr(util, "assign_to_nearest_center",
                           of.assign_to_nearest_center)
            for _ in range(n_sweeps):
                ii, dd, aa, ctrs = km._kmedoids_pam_update(
                    X, _device(name) if dev else ORACLE[name], ii, aa, dd,
                    proposals=props, random_state=rs)
        out[dev] = (list(ii), dd, aa, ctrs, rs.randint(1 << 30, size=3))
    assert out[1][0] == out[0][0], (name, X.shape, X.dtype, props is not None)
    _same(out[1][1], out[0][1])
    _same(out[1][2], out[0][2])
    assert len(out[1][3]) == len(out[0][3])
    for x, y in zip(out[1][3], out[0][3]):
        _same(x, y)
    _same(out[1][4], out[0][4])
    return out[0]


# ---- (a) one point against all: every feature count, sample count, dtype --------
FS = (1, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049, 4100)
NS = (1, 255, 256, 257, 1000)


def _ints(rng, dt, shape):
    info = np.iinfo(dt)
    lo, hi = max(int(info.min), -2 ** 26), min(int(info.max), 2 ** 26)
    return rng.randint(lo, hi, size=shape, dtype=np.int64).astype(dt)


def test_one_vs_all_grid():
    """FT_CHUNK (32) of the loader, FY_CHUNK (2048) of the target's staging,
    partial and whole tiles of 256 samples; float32 and float64 in their own
    arithmetic, int8 ... int64 through the float64 path, hamming on int8 ...
    uint64 (the extremes of each type: uint64 above 2**63 wraps on its way to
    the device's int64, equality survives).  Every F with two n per dtype."""
    rng = np.random.RandomState(31)
    float_dts = (np.float32, np.float64, np.int8, np.int16, np.int32, np.int64)
    ham_dts = (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32,
               np.int64, np.uint64)
    for k, dt in enumerate(float_dts):
        for i, F in enumerate(FS):
            for off in (0, 2):
                n = NS[(i + k + off) % len(NS)]
                if np.issubdtype(dt, np.floating):
                    X = rng.normal(size=(n, F)).astype(dt)
                    y = rng.normal(size=F).astype(dt)
                else:
                    X = _ints(rng, dt, (n, F))
                    y = _ints(rng, dt, F)
                y[::2] = X[rng.randint(n), ::2]      # half the features on a sample
                for name in ("euclidean", "manhattan"):
                    _check_distance(name, X, y)
    for k, dt in enumerate(ham_dts):
        info = np.iinfo(dt)
        vals = np.array([info.min, info.max, 1], dtype=dt)
        for i, F in enumerate(FS):
            for off in (0, 2):
                n = NS[(i + k + off) % len(NS)]
                X = vals[rng.randint(0, 3, size=(n, F))]
                y = X[rng.randint(n)].copy()
                y[rng.rand(F) < 0.3] = vals[2]
                d = _check_distance("hamming", X, y)
                assert d.min() < 1.0 or n == 1


# ---- (b) value edges ----------------------------------------------------------
def _families(rng):
    """(label, X, metrics): every family also through resident k-centers"""
    fam = []
    # float32 cancellation: 1e4 with noise of an ulp or so; the float32
    # difference is what the reference computes
    fam.append(("cancel32", (1e4 + 1e-3 * rng.normal(size=(3000, 8))).astype(np.float32),
                ("euclidean", "manhattan")))
    # subnormals: values (float32 below 1.2e-38, float64 below 2.2e-308), squares
    # (float32 1e-20, float64 1e-160), alone and mixed with normal samples
    for dt, tiny, sq in ((np.float32, 1e-40, 1e-20), (np.float64, 1e-310, 1e-160)):
        v = rng.normal(size=(2500, 6))
        fam.append(("subnormal", (v * tiny).astype(dt), ("euclidean", "manhattan")))
        fam.append(("subnormal_sq", (v * sq).astype(dt), ("euclidean", "manhattan")))
        m = (v * np.where(rng.rand(2500, 1) < 0.3, 1.0,
                          np.where(rng.rand(2500, 6) < 0.5, tiny, sq))).astype(dt)
        fam.append(("subnormal_mixed", m, ("euclidean", "manhattan")))
    # float32 squares that overflow to inf (and sums that do): distances +inf,
    # np.argmax takes the first +inf, a sample at +inf from every center keeps -1
    big = rng.normal(size=(2000, 4)) * np.where(rng.rand(2000, 1) < 0.5, 3e19, 1.0)
    fam.append(("overflow32", big.astype(np.float32), ("euclidean", "manhattan")))
    # +-inf in the data, no NaN: the resident path; inf - inf = NaN distances,
    # which the strict < never takes
    for dt in (np.float32, np.float64):
        v = rng.normal(size=(2000, 5))
        v[rng.rand(2000, 5) < 0.03] = np.inf
        v[rng.rand(2000, 5) < 0.03] = -np.inf
        fam.append(("inf", v.astype(dt), ("euclidean", "manhattan")))
    # -0.0 against 0.0
    for dt in (np.float32, np.float64):
        vals = np.array([-0.0, 0.0, 1.0, -1.0], dtype=dt)
        fam.append(("signed_zero", vals[rng.randint(0, 4, size=(2000, 6))],
                    ("euclidean", "manhattan")))
    # integers near the 2**26 bound of libdist._working_dtype, both signs
    v = (2 ** 26 - rng.randint(0, 4, size=(2000, 5))) * rng.choice([-1, 1], size=(2000, 5))
    fam.append(("int26", v.astype(np.int64), ("euclidean", "manhattan", "hamming")))
    return fam


def test_value_edges_one_vs_all():
    rng = np.random.RandomState(41)
    for label, X, names in _families(rng):
        for t in (0, len(X) // 2 + 1, len(X) - 1):
            for name in names:
                d = _check_distance(name, X, X[t])
                if label == "overflow32" and name == "euclidean":
                    assert np.isposinf(d).any()
                if label == "inf":
                    assert not np.isnan(X).any()
        if label == "inf":
            assert np.isnan(of.euclidean(X, X[np.isinf(X).any(axis=1)][0])).any()
        if label == "subnormal_sq" and X.dtype == np.float32:
            assert (of.euclidean(X, X[0])[1:] > 0).all()


def test_value_edges_resident_kcenters(resident_calls):
    rng = np.random.RandomState(43)
    for label, X, names in _families(rng):
        if label == "cancel32":
            Xc = X
        for name in names:
            r = _check_kcenters(name, X, resident_calls, n_clusters=30)
            if label == "overflow32" and name == "euclidean":
                assert np.isposinf(r.distances).any()
                assert (r.assignments == -1).any()
    # a cut-off among the cancelled float32 values
    _check_kcenters("euclidean", Xc, resident_calls, n_clusters=np.inf,
                    dist_cutoff=2.5e-3)


# ---- (c) one matrix of 134 MB ----------------------------------------------------
N_BIG = 2100003
F_BIG = 16
FAR = (5, 2000000)          # two identical outliers, 7812 blocks of 256 apart
NEXT = (1500000, 2050000)   # and the next pair, both beyond the first 1024 blocks


def _big_matrix(dt):
    rng = np.random.RandomState(51)
    X = rng.randint(0, 6, size=(N_BIG, F_BIG)).astype(dt)
    for i in FAR:
        X[i] = 40
    for i in NEXT:
        X[i] = 30
    return X


def test_large_matrix(resident_calls, monkeypatch):
    """float32 2 100 003 x 16 in small integers (ties in distance everywhere):
    the loader stages 128 MB per chunk (two chunks), the k-centers arg-max runs
    over 8204 block maxima (the 1024-stride loop of feat_pick_kernel) and ties
    between blocks thousands apart (the second tie beyond the first 1024), the PAM sweep takes windows by size (>= 64 MB,
    no override).  float64: three loader chunks."""
    monkeypatch.delenv("EK_FEAT_PAM_WINDOWS", raising=False)
    monkeypatch.delenv("EK_FEAT_PAM_SYNC", raising=False)
    X = _big_matrix(np.float32)
    assert X.nbytes > 128 << 20 and X.nbytes >= 64 << 20
    assert (N_BIG + 255) // 256 > 8 * 1024
    for t in (0, FAR[0], N_BIG - 1000):
        _check_distance("euclidean", X, X[t])
        _check_distance("manhattan", X, X[t], forms=("bind",))
    r = _check_kcenters("euclidean", X, resident_calls, n_clusters=25)
    assert r.center_indices[:3] == [0, FAR[0], NEXT[0]]     # the first of each tie
    _check_kcenters("euclidean", X, resident_calls, n_clusters=np.inf,
                    dist_cutoff=12.2)                  # (stops at the ninth center)
    inds = [int(i) for i in r.center_indices]
    got = _sweeps(X, "euclidean", inds, r.assignments.copy(), r.distances.copy(),
                  None, 4, 1, monkeypatch)
    assert got[0] != inds                               # proposals were accepted
    del X
    X = _big_matrix(np.float64)
    for t in (0, N_BIG - 1000):
        _check_distance("euclidean", X, X[t], forms=("call", "bind_out"))
    _check_kcenters("euclidean", X, resident_calls, n_clusters=12)


# ---- (d) more than 256 medoids ----------------------------------------------------
def _start(X, name, K):
    from enspara_amd.cluster.kcenters import kcenters
    r = kcenters(X, _device(name), n_clusters=K)
    return [int(i) for i in r.center_indices], r.assignments, r.distances


def test_pam_beyond_256_medoids(monkeypatch):
    """The tiled nearest search in KC = ceil(K / 256) chunks, merged by the
    last workgroup of each batch (lowest medoid index among equal distances).
    Drawn and explicit proposals, two sweeps; small integer values give ties in
    every sweep.  With explicit proposals, medoid slot 3 and a slot in the next
    chunk sit on identical coordinates (proposed where they are, so both stay):
    the lower label must win every tie between them."""
    rng = np.random.RandomState(61)
    cases = [
        (rng.randint(0, 5, size=(12000, 9)).astype(np.float32), 513,
         ("euclidean", "manhattan")),
        (rng.normal(size=(6000, 130)), 300, ("euclidean", "manhattan")),
        (rng.randint(0, 3, size=(8000, 9)).astype(np.int64), 257,
         ("euclidean", "manhattan", "hamming")),
        (rng.randint(0, 3, size=(6000, 130)).astype(np.int64), 300, ("hamming",)),
        (rng.normal(size=(7000, 9)).astype(np.float32), 300, ("euclidean",)),
    ]
    moved = 0
    for X, K, names in cases:
        for name in names:
            inds, a, d = _start(X, name, K)
            got = _sweeps(X, name, inds, a, d, None, 4, 2, monkeypatch)
            moved += got[0] != inds
            # explicit proposals, slot `hi` on the coordinates of slot 3
            hi = 260 if K > 260 else 256
            Xp = X.copy()
            free = np.setdiff1d(np.arange(len(X)), inds)
            q = int(free[rng.randint(len(free))])
            Xp[q] = Xp[inds[3]]
            med = list(inds)
            med[hi] = q
            a0, d0 = of.assign_to_nearest_center(Xp, [Xp[i] for i in med], ORACLE[name])
            assert not (a0 == hi).any() and (d0 == 0).sum() >= K
            props = [int(v) for v in rng.randint(0, len(X), size=K)]
            props[3], props[hi] = med[3], med[hi]
            got = _sweeps(Xp, name, med, a0, d0, props, 4, 2, monkeypatch)
            moved += got[0] != med
            assert got[0][3] == med[3] and got[0][hi] == q
            assert not (got[2] == hi).any()
    assert moved >= 12


# ---- (e) windows of every width ------------------------------------------------------
def test_pam_windows_every_width(monkeypatch):
    """Windows of FEAT_WIN = 32 proposals; the last window of K = 35, 71, 108,
    128 holds 3, 7, 12, 32 slots, which selects feat_multi_distance_kernel<W>
    with W = 4, 8, 16, 32; F = 33 and 65 cross its FEAT_MD_CH (32) slices."""
    monkeypatch.setenv("EK_FEAT_PAM_WINDOWS", "1")
    rng = np.random.RandomState(71)
    moved = 0
    for K, F, dt in ((35, 33, np.float32), (71, 65, np.float64), (108, 33, np.float64),
                     (128, 65, np.float32), (35, 65, np.float64), (71, 33, np.float32),
                     (108, 65, np.float32), (128, 33, np.float64)):
        X = rng.normal(size=(3000, F)).astype(dt)
        if K in (71, 108):
            X = np.round(X)                          # ties
        for name in ("euclidean", "manhattan"):
            inds, a, d = _start(X, name, K)
            props = [int(v) for v in rng.randint(0, len(X), size=K)]
            got = _sweeps(X, name, inds, a, d, props, 4, 2, monkeypatch)
            moved += got[0] != inds
            got = _sweeps(X, name, inds, a, d, None, 4, 1, monkeypatch)
            moved += got[0] != inds
    assert moved >= 24


# ---- (f) the resident loops across FY_CHUNK -------------------------------------------
# feat_step_kernel (resident k-centers) and feat_dist_classify_kernel (the sweep's
# plain path) stage the center / the proposal through feat_one_vs_all in pieces of
# FY_CHUNK = 2048 features: one feature past it, a last tile of 300 - 256 samples.
ACROSS = (("euclidean", np.float32), ("manhattan", np.float64), ("hamming", np.uint16))


def _across_matrix(name, dt):
    rng = np.random.RandomState(81)
    if name == "hamming":
        return rng.randint(0, 3, size=(300, 2049)).astype(dt)
    return rng.normal(size=(300, 2049)).astype(dt)


@pytest.mark.parametrize("name,dt", ACROSS)
def test_resident_kcenters_across_fy_chunk(name, dt, resident_calls):
    _check_kcenters(name, _across_matrix(name, dt), resident_calls, n_clusters=5)


@pytest.mark.parametrize("name,dt", ACROSS)
def test_pam_sweep_across_fy_chunk(name, dt, monkeypatch):
    """5 medoids, drawn and explicit proposals: 2.4 MB or less of samples, so every
    proposal takes its own pass over them (no window)."""
    monkeypatch.delenv("EK_FEAT_PAM_WINDOWS", raising=False)
    monkeypatch.delenv("EK_FEAT_PAM_SYNC", raising=False)
    X = _across_matrix(name, dt)
    assert X.nbytes < 64 << 20
    inds, a, d = _start(X, name, 5)
    _sweeps(X, name, inds, a, d, None, 4, 2, monkeypatch)
    _sweeps(X, name, inds, a, d, [7, 299, 256, 100, 255], 4, 1, monkeypatch)
