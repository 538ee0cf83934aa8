"""The nearest-center scan for libdist metrics (ek_feat_assign_nearest), the
parts that need no device: which inputs of util.assign_to_nearest_center take
the one-launch form (libdist.assign_nearest_resident, here a recorder that
answers from the oracle), the ABI, reassign_features' batching, and the sharded
warm start with shard objects that have no ``assign_nearest``."""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import features as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ORACLE = {0: of.euclidean, 1: of.manhattan, 2: of.hamming}


@pytest.fixture
def recorder(monkeypatch):
    """libdist.assign_nearest_resident replaced by the oracle; the calls"""
    from enspara_amd.geometry import libdist
    calls = []

    def fake(X, metric_id, centers, device=0):
        calls.append((np.asarray(X).shape, int(metric_id), len(centers)))
        return of.assign_to_nearest_center(np.asarray(X), np.asarray(centers),
                                           ORACLE[int(metric_id)])
    # (no raising=False: the attribute must exist)
    monkeypatch.setattr(libdist, "assign_nearest_resident", fake)
    return calls


def test_dispatch_takes_the_device_form(recorder):
    from enspara_amd.cluster import util
    from enspara_amd.geometry import libdist
    rng = np.random.RandomState(1)
    for dt in (np.float32, np.float64, np.int16, np.uint8, np.int64):
        X = (rng.normal(size=(300, 7)) * 5).astype(dt)
        C = X[[3, 50, 3, 299]]
        for metric, mid in (("euclidean", 0), ("manhattan", 1), ("cityblock", 1),
                            (libdist.euclidean, 0), (libdist.manhattan, 1)):
            before = len(recorder)
            a, d = util.assign_to_nearest_center(X, C, metric)
            assert recorder[before:] == [((300, 7), mid, 4)], (dt, metric)
            wa, wd = of.assign_to_nearest_center(X, C, ORACLE[mid])
            assert a.dtype == np.int64 and d.dtype == np.float64
            np.testing.assert_array_equal(a, wa)
            np.testing.assert_array_equal(d, wd)
            assert not (a == 2).any()           # the duplicate never wins
        # a list of rows qualifies as well
        before = len(recorder)
        util.assign_to_nearest_center(X, [c for c in C], "euclidean")
        assert len(recorder) == before + 1
    Xi = rng.randint(0, 3, size=(100, 6))
    before = len(recorder)
    util.assign_to_nearest_center(Xi, Xi[:5], libdist.hamming)
    assert recorder[before:] == [((100, 6), 2, 5)]


def test_dispatch_keeps_the_loop(recorder, monkeypatch):
    """a plain callable, float16, an empty X, a list instead of an array: the
    per-center loop as before"""
    from enspara_amd.cluster import util
    from enspara_amd.geometry import libdist
    rng = np.random.RandomState(2)
    X = rng.normal(size=(50, 4))
    C = X[:3]
    # the loop would need a device for the libdist metrics: stand-ins that count
    loop_calls = []

    def per_center(metric_id):
        def f(A, y, out=None):
            loop_calls.append(metric_id)
            return ORACLE[metric_id](np.asarray(A, dtype=np.float64)
                                     if np.asarray(A).dtype == np.float16
                                     else np.asarray(A), np.asarray(y))
        f.device_metric_id = metric_id
        return f
    a, d = util.assign_to_nearest_center(X, C, of.euclidean)     # plain callable
    np.testing.assert_array_equal(a, of.assign_to_nearest_center(X, C, of.euclidean)[0])
    assert recorder == []
    for Xq, Cq in ((X.astype(np.float16), C.astype(np.float16)),
                   (X[:0], C),
                   ([list(r) for r in X], C)):
        n = len(loop_calls)
        a, d = util.assign_to_nearest_center(Xq, Cq, per_center(0))
        assert recorder == [], type(Xq)
        assert len(loop_calls) == n + 3
        assert len(a) == len(Xq) and a.dtype == np.int64 and d.dtype == np.float64
    assert loop_calls, "the loop never ran"
    # NaN needs no gate: the oracle (and the kernel) never take one
    Xn = X.copy()
    Xn[7] = np.nan
    a, d = util.assign_to_nearest_center(Xn, C, "euclidean")
    assert len(recorder) == 1
    assert a[7] == 0 and np.isposinf(d[7])


def test_header_and_library_carry_the_symbol():
    from enspara_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "enspara_hip.h")).read()
    assert re.search(r"\bint\s+ek_feat_assign_nearest\s*\(\s*ek_feat\s*\*", hdr)
    assert "ek_feat_assign_nearest" in _lib.SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH],
                         capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT ek_feat_assign_nearest\b", out)


def test_reassign_features_batches(recorder):
    from enspara_amd import ra
    from enspara_amd.cluster.reassign import reassign_features
    rng = np.random.RandomState(3)
    C = rng.normal(size=(9, 5)).astype(np.float32)
    lens = [40, 1, 0, 77, 13, 60]
    arrays = [rng.normal(size=(n, 5)).astype(np.float32) for n in lens]
    want_a, want_d = of.assign_to_nearest_center(np.concatenate(arrays), C,
                                                 of.manhattan)
    # uneven lengths, three batches (one of them a callable) -> RaggedArrays
    targets = list(arrays)
    targets[3] = lambda: arrays[3]
    a, d = reassign_features(targets, C, "manhattan", batch_size=80)
    assert [c[0][0] for c in recorder] == [41, 77, 73] and all(c[1] == 1 and c[2] == 9 for c in recorder)
    assert isinstance(a, ra.RaggedArray) and isinstance(d, ra.RaggedArray)
    assert [len(r) for r in a] == lens
    np.testing.assert_array_equal(np.concatenate(list(a)), want_a)
    np.testing.assert_array_equal(np.concatenate(list(d)), want_d)
    # one batch: one call on the concatenation
    del recorder[:]
    a1, d1 = reassign_features(arrays, C, "manhattan", batch_size=10 ** 6)
    assert recorder == [((sum(lens), 5), 1, 9)]
    np.testing.assert_array_equal(np.concatenate(list(a1)), want_a)
    np.testing.assert_array_equal(np.concatenate(list(d1)), want_d)
    # equal lengths -> ndarrays
    same = [rng.normal(size=(30, 5)) for _ in range(4)]
    a2, d2 = reassign_features(same, C, "euclidean", batch_size=70)
    wa, wd = of.assign_to_nearest_center(np.concatenate(same), C.astype(np.float64),
                                         of.euclidean)
    assert isinstance(a2, np.ndarray) and a2.shape == (4, 30) and a2.dtype == np.int64
    assert isinstance(d2, np.ndarray) and d2.dtype == np.float64
    np.testing.assert_array_equal(a2.ravel(), wa)
    np.testing.assert_array_equal(d2.ravel(), wd)
    from enspara_amd.exception import ImproperlyConfigured
    with pytest.raises(ImproperlyConfigured):
        reassign_features(arrays, C, "manhattan", batch_size=50)
    with pytest.raises(ImproperlyConfigured):
        reassign_features(arrays, C, of.manhattan, batch_size=500)


@pytest.fixture
def one_rank_group(tmp_path):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method="file://%s" % (tmp_path / "store"),
                            rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


def test_sharded_warm_start_without_assign_nearest(one_rank_group):
    """the host shard doubles have no ``assign_nearest``: the per-center loop
    around their ``distance`` still runs and gives the single-process result; a
    shard that has the method is asked once instead"""
    from _host_feature_shard import HostFeatureShard, make_host_shard
    from enspara_amd import sharded
    from enspara_amd.cluster.kcenters import kcenters
    assert not hasattr(HostFeatureShard, "assign_nearest")
    rng = np.random.RandomState(4)
    X = rng.normal(size=(700, 5)).astype(np.float32)
    init = [X[5].copy(), X[350].copy(), X[5].copy(), (X[5] + 100), X[600].copy()]
    want = kcenters(X, of.euclidean, n_clusters=14, init_centers=init)
    got = sharded.fit_features_sharded(X, 0, n_clusters=14, init_centers=init,
                                       make_shard=make_host_shard)
    assert [int(i) for _, i in got.center_indices] == \
        [int(i) for i in want.center_indices]
    np.testing.assert_array_equal(got.assignments, want.assignments)
    np.testing.assert_array_equal(got.distances, want.distances)

    asked = []

    class WithScan(HostFeatureShard):
        def assign_nearest(self, centers):
            asked.append(len(centers))
            a, d = of.assign_to_nearest_center(self.X, np.asarray(centers),
                                               of.euclidean)
            self.set_state(d, a.astype(np.int32))
            return d, a.astype(np.int32)

        def distance(self, y):
            raise AssertionError("the per-center loop ran")

    @contextlib.contextmanager
    def make(Xl, metric_id, offset):
        yield WithScan(Xl, metric_id, offset)
    got2 = sharded.fit_features_sharded(X, 0, n_clusters=14, init_centers=init,
                                        make_shard=make)
    assert asked == [5]
    np.testing.assert_array_equal(got2.assignments, want.assignments)
    np.testing.assert_array_equal(got2.distances, want.distances)
