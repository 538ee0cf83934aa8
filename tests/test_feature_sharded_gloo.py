"""mpi_mode for the feature metrics (enspara_amd/sharded.py
fit_features_sharded) at worlds 2 and 3 on CPU: backend gloo, numpy-backed
shards with the device's record layout (tests/_host_feature_shard.py).  What
is under test is the host logic: the agreement before the loop, the offsets,
the warm start's exchange, the driver loop's winner / stop rules and the
centers' rows.  Every comparison is exact; the want-side is the single-process
reference-shaped host loop (cluster/kcenters.py _kcenters_host) around the
ORACLE's metric, never the code under test.  The property is the one the
reference's own MPI tests assert on point clouds with a euclidean metric
(enspara/test/test_cluster.py:241-314)."""
import os
import socket
import sys
import tempfile
import time

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAWN_LIMIT = 240       # seconds: no rank may hang


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bounds(world):
    """uneven contiguous shards of the N samples; at world 3 the MIDDLE rank
    owns none"""
    return {2: [0, 517, N], 3: [0, 700, 700, N]}[world]


N = 1300
# name -> (metric id, dtype, n_features, n_clusters, cut-off, warm start)
CASES = {
    "count_euclidean_f32": (0, "float32", 5, 23, 0.0, False),
    "count_manhattan_f64": (1, "float64", 3, 17, 0.0, False),
    "count_hamming_i16": (2, "int16", 9, 12, 0.0, False),
    "cutoff_euclidean_f64": (0, "float64", 4, None, 1.1, False),
    "both_manhattan_f32": (1, "float32", 6, 40, 7.0, False),
    "warm_euclidean_f32": (0, "float32", 5, 15, 0.0, True),
    "warm_manhattan_i32": (1, "int32", 4, 14, 0.0, True),
}


def _data(name):
    mid, dtype, F, K, cutoff, warm = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    if np.issubdtype(np.dtype(dtype), np.integer):
        X = rng.randint(0, 4, size=(N, F)).astype(dtype)    # ties everywhere
    else:
        X = rng.normal(size=(N, F)).astype(dtype)
    init = None
    if warm:
        # x[5] twice: the second copy attracts nothing (strict <); a point far
        # outside the cloud attracts nothing either
        init = [X[5].copy(), X[N // 2].copy(), X[5].copy(),
                (X[5] + 100).astype(dtype), X[900].copy()]
    return X, init


def _oracle_metric(mid):
    from oracle import features as of
    f = {0: of.euclidean, 1: of.manhattan, 2: of.hamming}[mid]
    return lambda A, y: f(np.asarray(A), np.asarray(y))


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["OMP_NUM_THREADS"] = "2"
    from enspara_amd import sharded
    from _host_feature_shard import make_host_shard
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                            rank=rank, world_size=world)
    b = _bounds(world)
    out = {}
    for name, (mid, dtype, F, K, cutoff, warm) in CASES.items():
        X, init = _data(name)
        mine = X[b[rank]:b[rank + 1]]
        res = sharded.fit_features_sharded(
            mine, mid, n_clusters=K, dist_cutoff=cutoff, init_centers=init,
            make_shard=make_host_shard)
        out[name + "_ci"] = np.array(res.center_indices).reshape(-1, 2)
        out[name + "_a"] = res.assignments
        out[name + "_d"] = res.distances
        out[name + "_c"] = np.array(res.centers)
    np.savez(os.path.join(outdir, "r%d.npz" % rank), **out)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(fn, world, args):
    ctx = mp.spawn(fn, args=(world, _free_port()) + args, nprocs=world,
                   join=False)
    deadline = time.time() + SPAWN_LIMIT
    while not ctx.join(timeout=5):
        if time.time() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("a rank hung: %d s without all ranks returning"
                        % SPAWN_LIMIT)


_RESULTS = {}


def _results(world):
    if world not in _RESULTS:
        with tempfile.TemporaryDirectory() as d:
            _spawn(_worker, world, (d,))
            _RESULTS[world] = [dict(np.load(os.path.join(d, "r%d.npz" % r)))
                               for r in range(world)]
    return _RESULTS[world]


def _check(world, name):
    from enspara_amd.cluster.kcenters import kcenters
    mid, dtype, F, K, cutoff, warm = CASES[name]
    X, init = _data(name)
    want = kcenters(X, _oracle_metric(mid),
                    n_clusters=np.inf if K is None else K, dist_cutoff=cutoff,
                    init_centers=init)
    parts = _results(world)
    b = _bounds(world)
    for p in parts:                 # every rank reports the same centers
        got = [b[int(r)] + int(i) for r, i in p[name + "_ci"]]
        assert got == [int(i) for i in want.center_indices]
        for r, i in p[name + "_ci"]:
            assert 0 <= i < b[int(r) + 1] - b[int(r)]
        assert p[name + "_c"].dtype == X.dtype
        np.testing.assert_array_equal(p[name + "_c"], np.array(want.centers))
    np.testing.assert_array_equal(
        np.concatenate([p[name + "_a"] for p in parts]), want.assignments)
    np.testing.assert_array_equal(
        np.concatenate([p[name + "_d"] for p in parts]), want.distances)
    assert parts[0][name + "_d"].dtype == np.float64
    assert parts[0][name + "_a"].dtype == np.int64
    return want


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("count")])
def test_fixed_count(world, name):
    want = _check(world, name)
    assert len(want.center_indices) == CASES[name][3]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", ["cutoff_euclidean_f64", "both_manhattan_f32"])
def test_cutoff(world, name):
    want = _check(world, name)
    # stops on the cut-off, after more than a couple of centers and (where a
    # count is given too) before the count
    assert 2 < len(want.center_indices) < (CASES[name][3] or N)
    assert want.distances.max() <= CASES[name][4]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", [c for c in CASES if c.startswith("warm")])
def test_warm_start(world, name):
    want = _check(world, name)
    K = CASES[name][3]
    # five initial centers, two of which attract nothing: three occupied
    # labels, K - 3 new centers behind the caller's five rows
    assert len(want.center_indices) == K
    assert len(want.centers) == 5 + K - 3


def _error_worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from enspara_amd import sharded
    from _host_feature_shard import make_host_shard
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                            rank=rank, world_size=world)
    rng = np.random.RandomState(3 + rank)
    good = rng.normal(size=(40, 6))
    nan = good.copy()
    nan[7, 2] = np.nan
    odd = rank == world - 1
    trials = {
        "n_features": good[:, :5] if odd else good,
        "dtype": good.astype(np.float32) if odd else good,
        "nan": nan if odd else good,
        "half": good.astype(np.float16) if odd else good,
        "ndim": good[0] if odd else good,
        "fine": good,
    }
    seen = []
    for name, X in trials.items():
        try:
            sharded.fit_features_sharded(X, 0, n_clusters=3,
                                         make_shard=make_host_shard)
            seen.append(name + ":none")
        except Exception as e:
            seen.append(name + ":" + type(e).__name__)
    # hamming needs integers everywhere
    try:
        sharded.fit_features_sharded(
            good if odd else good.astype(np.int64), 2, n_clusters=3,
            make_shard=make_host_shard)
        seen.append("hamming:none")
    except Exception as e:
        seen.append("hamming:" + type(e).__name__)
    with open(os.path.join(outdir, "r%d.txt" % rank), "w") as f:
        f.write("\n".join(seen))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_raises(world):
    """one rank's samples disagree (n_features, dtype) or are unusable (NaN,
    float16, not 2-D; floats for hamming): EVERY rank raises the same error
    class and nobody is left waiting in a collective; the group then still
    works (the last fit succeeds everywhere)"""
    with tempfile.TemporaryDirectory() as d:
        _spawn(_error_worker, world, (d,))
        seen = [open(os.path.join(d, "r%d.txt" % r)).read().split("\n")
                for r in range(world)]
    want = ["n_features:ImproperlyConfigured", "dtype:ImproperlyConfigured",
            "nan:DataInvalid", "half:DataInvalid", "ndim:DataInvalid",
            "fine:none", "hamming:DataInvalid"]
    for s in seen:
        assert s == want


def test_estimator_needs_a_group_and_a_device_metric():
    """mpi_mode without a process group, with a callable metric or with the
    triangle inequality on a feature metric: ImproperlyConfigured, saying so
    (no host-loop fallback across ranks); KHybrid stays out of scope"""
    from enspara_amd.cluster import KCenters, KHybrid
    from enspara_amd.cluster.kcenters import kcenters
    from enspara_amd.exception import ImproperlyConfigured
    X = np.random.RandomState(0).normal(size=(50, 3))
    with pytest.raises(ImproperlyConfigured, match="process group"):
        KCenters("euclidean", n_clusters=3, mpi_mode=True).fit(X)
    with pytest.raises(ImproperlyConfigured, match="callable"):
        kcenters(X, _oracle_metric(0), n_clusters=3, mpi_mode=True)
    with pytest.raises(ImproperlyConfigured, match="triangle"):
        kcenters(X, "manhattan", n_clusters=3, mpi_mode=True,
                 use_triangle_inequality=True)
    with pytest.raises(ImproperlyConfigured, match="PAM"):
        KHybrid("euclidean", n_clusters=3, mpi_mode=True).fit(X)
