"""Sharded PAM sweeps for the feature metrics, host logic under gloo (no GPU).

The drivers of enspara_amd/sharded.py -- fit_features_sharded(n_iters=..),
kmedoids_features_sharded, pam_sweep_sharded over a feature shard's pam_*
methods -- run at worlds 2 and 3 over uneven shards (one of them empty) with a
numpy-backed shard (tests/_host_feature_pam_shard.py); every result is compared
exactly with tests/_feature_pam_mpi_want.py, the host restatement of the
reference's MPI sweep, which is itself pinned to oracle/cluster.py's
pam_update_numpy here."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
SPAWN_LIMIT = 300
N = 900


def _bounds(world):
    """uneven contiguous shards; at world 3 the MIDDLE rank owns none"""
    return {1: [0, N], 2: [0, 389, N], 3: [0, 500, 500, N]}[world]


# name -> (kind, metric id, dtype, n_features, K, sweeps, seed)
CASES = {
    "hy_euclidean_f32": ("hybrid", 0, "float32", 5, 12, 2, ("state", 7)),
    "hy_manhattan_f64": ("hybrid", 1, "float64", 3, 9, 2, ("int", 11)),
    "hy_hamming_i16": ("hybrid", 2, "int16", 8, 10, 2, ("state", 2)),
    "hy_init_euclidean_f32": ("hybrid_init", 0, "float32", 5, 12, 2, ("state", 8)),
    # one initial center attracts no sample: fewer medoids than labels come out of
    # the warm start, the labels after the gap shift (as in the single-process run)
    "hy_initgap_euclidean_f32": ("hybrid_init_gap", 0, "float32", 5, 10, 1, ("int", 2)),
    "km_cold_euclidean_f64": ("cold", 0, "float64", 4, 8, 2, ("int", 5)),
    "km_warm_manhattan_f32": ("warm", 1, "float32", 6, 11, 1, ("state", 3)),
    "km_props_euclidean_f32": ("props", 0, "float32", 5, 7, 1, None),
    # cost sums exact in float64: ANY sharding gives the single-process result
    "exact_manhattan_i32": ("hybrid", 1, "int32", 4, 8, 2, ("state", 4)),
    "exact_hamming_i8": ("hybrid", 2, "int8", 8, 9, 2, ("int", 6)),
}
EXACT = [c for c in CASES if c.startswith("exact")]


def _data(name):
    kind, mid, dtype, F, K, sweeps, seed = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    if np.issubdtype(np.dtype(dtype), np.integer):
        X = rng.randint(0, 4, size=(N, F)).astype(dtype)    # ties everywhere
    else:
        X = rng.normal(size=(N, F)).astype(dtype)
    return X


def _init(X, empty=False):
    """initial centers for the warm-started k-hybrid; ``empty``: x[5] twice --
    the second copy attracts nothing (strict <), its label stays empty"""
    rows = [X[5].copy(), X[N // 2].copy(), X[700].copy()]
    if empty:
        rows.insert(2, X[5].copy())
    return rows


def _seed(spec):
    if spec is None:
        return None
    return np.random.RandomState(spec[1]) if spec[0] == "state" else spec[1]


def _proposals(name):
    K = CASES[name][4]
    return [int(v) for v in
            np.random.RandomState(99).choice(N, size=K, replace=False)]


def _want(name, bounds):
    import _feature_pam_mpi_want as w
    kind, mid, dtype, F, K, sweeps, seed = CASES[name]
    X = _data(name)
    if kind == "hybrid":
        return w.khybrid_want(X, mid, K, sweeps, seed[1], bounds)
    if kind in ("hybrid_init", "hybrid_init_gap"):
        return w.khybrid_want(X, mid, K, sweeps, seed[1], bounds,
                              _init(X, empty=kind == "hybrid_init_gap"))
    if kind == "cold":
        med = w.cold_medoids(N, K, seed[1])
        a, d = w.start_nearest(X, mid, med)
    else:
        med, a, d = w.start_kcenters(X, mid, K)
    rs = np.random.RandomState(seed[1]) if seed else None
    for _ in range(sweeps):
        med, d, a = w.pam_update_mpi(
            X, mid, med, a, d, bounds, random_state=rs,
            proposals=_proposals(name) if kind == "props" else None)
    return med, d, a


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


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


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["OMP_NUM_THREADS"] = "2"
    from enspara_amd import sharded
    from _host_feature_pam_shard import make_host_pam_shard
    import _feature_pam_mpi_want as w
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                            rank=rank, world_size=world)
    b = _bounds(world)
    out = {}
    for name, (kind, mid, dtype, F, K, sweeps, seed) in CASES.items():
        X = _data(name)
        mine = X[b[rank]:b[rank + 1]]
        if kind.startswith("hybrid"):
            res = sharded.fit_features_sharded(
                mine, mid, n_clusters=K, n_iters=sweeps,
                init_centers=(_init(X, empty=kind == "hybrid_init_gap")
                              if kind != "hybrid" else None),
                random_state=_seed(seed), make_shard=make_host_pam_shard)
        elif kind == "cold":
            res = sharded.kmedoids_features_sharded(
                mine, mid, n_clusters=K, n_iters=sweeps,
                random_state=_seed(seed), make_shard=make_host_pam_shard)
        else:
            med, a, d = w.start_kcenters(X, mid, K)
            props = None
            if kind == "props":
                props = []
                for g in _proposals(name):
                    r = max(q for q in range(world) if b[q] <= g)
                    while b[r + 1] <= g:
                        r += 1
                    props.append((r, g - b[r]))
            res = sharded.kmedoids_features_sharded(
                mine, mid, n_iters=sweeps, assignments=a[b[rank]:b[rank + 1]],
                distances=d[b[rank]:b[rank + 1]], cluster_center_inds=med,
                proposals=props, random_state=_seed(seed),
                make_shard=make_host_pam_shard)
        out[name + "_ci"] = np.array(res.center_indices).reshape(-1, 2)
        out[name + "_a"] = res.assignments
        out[name + "_d"] = res.distances
        out[name + "_c"] = np.array(res.centers)
    np.savez(os.path.join(outdir, "r%d.npz" % rank), **out)
    dist.barrier()
    dist.destroy_process_group()


_RESULTS = {}


def _results(world):
    if world not in _RESULTS:
        with tempfile.TemporaryDirectory() as d:
            _spawn(_worker, world, (d,))
            _RESULTS[world] = [dict(np.load(os.path.join(d, "r%d.npz" % r)))
                               for r in range(world)]
    return _RESULTS[world]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", list(CASES))
def test_sharded_sweeps(world, name):
    """medoids, labels, float64 distances and the medoids' rows, exactly; the
    same medoid list on every rank"""
    b = _bounds(world)
    med, d, a = _want(name, b)
    X = _data(name)
    parts = _results(world)
    for p in parts:
        got = [b[int(r)] + int(i) for r, i in p[name + "_ci"]]
        assert got == med
        for r, i in p[name + "_ci"]:
            assert 0 <= i < b[int(r) + 1] - b[int(r)]
        assert p[name + "_c"].dtype == X.dtype
        np.testing.assert_array_equal(p[name + "_c"], X[med])
    np.testing.assert_array_equal(
        np.concatenate([p[name + "_a"] for p in parts]), a)
    np.testing.assert_array_equal(
        np.concatenate([p[name + "_d"] for p in parts]), d)
    assert parts[0][name + "_d"].dtype == np.float64
    assert parts[0][name + "_a"].dtype == np.int64
    if name in EXACT:
        # ... and the single-process sweep's
        m1, d1, a1 = _want(name, _bounds(1))
        assert med == m1
        np.testing.assert_array_equal(d, d1)
        np.testing.assert_array_equal(a, a1)


@pytest.mark.parametrize("name", EXACT)
def test_exact_inputs_do_not_depend_on_the_sharding(name):
    """the premise of the sharding-independence cases, on the want side"""
    ref = _want(name, _bounds(1))
    for world in (2, 3):
        got = _want(name, _bounds(world))
        assert got[0] == ref[0]
        np.testing.assert_array_equal(got[1], ref[1])
        np.testing.assert_array_equal(got[2], ref[2])


@pytest.mark.parametrize("name", ["hy_euclidean_f32", "hy_manhattan_f64",
                                  "hy_hamming_i16", "km_props_euclidean_f32"])
def test_want_helper_is_pam_update_numpy(name, monkeypatch):
    """with one shard the want side IS oracle/cluster.py's pam_update_numpy,
    run on feature rows with the oracle's metric.  (pam_update_numpy is written
    for frames: this pin swaps oracle.cluster's private _metric_on and
    assign_to_nearest_center for feature forms and hands it a qcp.Prepared
    made without __init__, of which it reads .xyz and .n only.  It holds while
    those names and that use stay; whoever renames them updates this test.)"""
    import _feature_pam_mpi_want as w
    from oracle import cluster as oc
    from oracle import features as of
    from oracle import qcp
    kind, mid, dtype, F, K, sweeps, seed = CASES[name]
    metric = w.METRICS[mid]
    X = _data(name)
    P = object.__new__(qcp.Prepared)
    P.xyz, P.n = X, len(X)
    monkeypatch.setattr(oc, "_metric_on", lambda P_: (lambda y: metric(P_.xyz, y)))
    monkeypatch.setattr(
        oc, "assign_to_nearest_center",
        lambda rows, ctrs: of.assign_to_nearest_center(rows, np.array(ctrs),
                                                       metric))
    med, a, d = w.start_kcenters(X, mid, K)
    props = _proposals(name) if kind == "props" else None
    rs1 = np.random.RandomState(5)
    rs2 = np.random.RandomState(5)
    got = (med, d, a)
    ref = (med, d, a)
    for _ in range(2):
        got = w.pam_update_mpi(X, mid, got[0], got[2], got[1], [0, N],
                               proposals=props, random_state=rs1)
        ref = oc.pam_update_numpy(P, ref[0], ref[2], ref[1], proposals=props,
                                  random_state=rs2)
        assert got[0] == [int(i) for i in ref[0]]
        np.testing.assert_array_equal(got[1], ref[1])
        np.testing.assert_array_equal(got[2], ref[2])
    assert got[0] != med            # (the sweeps did move medoids)


def _error_worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from enspara_amd import sharded
    from _host_feature_pam_shard import make_host_pam_shard
    import _feature_pam_mpi_want as w
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port,
                            rank=rank, world_size=world)
    b = _bounds(world)
    X = _data("hy_euclidean_f32")
    mine = X[b[rank]:b[rank + 1]]
    seen = []

    def attempt(name, f):
        try:
            f()
            seen.append(name + ":none")
        except Exception as e:
            seen.append(name + ":" + type(e).__name__)

    attempt("seed_int", lambda: sharded.fit_features_sharded(
        mine, 0, n_clusters=5, n_iters=1, random_state=10 + rank,
        make_shard=make_host_pam_shard))
    attempt("seed_state", lambda: sharded.kmedoids_features_sharded(
        mine, 0, n_clusters=5, n_iters=1,
        random_state=np.random.RandomState(rank),
        make_shard=make_host_pam_shard))
    attempt("seed_kind", lambda: sharded.fit_features_sharded(
        mine, 0, n_clusters=5, n_iters=1,
        random_state=None if rank else 3, make_shard=make_host_pam_shard))
    # a cluster without members: samples 0 and 100 are the same row, everything
    # is labelled 1 -- label 0's medoid sits at distance 0, and has no member
    Y = X.copy()
    Y[0] = Y[100]
    d = w.METRICS[0](Y, Y[100])
    a = np.ones(N, dtype=np.int64)
    attempt("memberless", lambda: sharded.kmedoids_features_sharded(
        Y[b[rank]:b[rank + 1]], 0, n_iters=1, assignments=a[b[rank]:b[rank + 1]],
        distances=d[b[rank]:b[rank + 1]], cluster_center_inds=[0, 100],
        random_state=1, make_shard=make_host_pam_shard))
    # medoids away from distance 0 on ONE rank's samples
    attempt("far_medoid", lambda: sharded.kmedoids_features_sharded(
        Y[b[rank]:b[rank + 1]], 0, n_iters=1, assignments=a[b[rank]:b[rank + 1]],
        distances=d[b[rank]:b[rank + 1]], cluster_center_inds=[0, 7],
        random_state=1, make_shard=make_host_pam_shard))
    attempt("some_of_three", lambda: sharded.kmedoids_features_sharded(
        mine, 0, n_iters=1, assignments=a[b[rank]:b[rank + 1]],
        make_shard=make_host_pam_shard))
    # a cold start with explicit proposals still draws its medoids from the seed
    attempt("seed_cold_props", lambda: sharded.kmedoids_features_sharded(
        mine, 0, n_clusters=3, n_iters=1, random_state=20 + rank,
        proposals=[(0, 1), (0, 2), (0, 3)], make_shard=make_host_pam_shard))
    # arguments that are wrong on ONE rank only
    odd = rank == world - 1
    attempt("some_of_three_one_rank", lambda: sharded.kmedoids_features_sharded(
        Y[b[rank]:b[rank + 1]], 0, n_iters=1, assignments=a[b[rank]:b[rank + 1]],
        distances=None if odd else d[b[rank]:b[rank + 1]],
        cluster_center_inds=[0, 100], random_state=1,
        make_shard=make_host_pam_shard))
    attempt("pairs_one_rank", lambda: sharded.kmedoids_features_sharded(
        Y[b[rank]:b[rank + 1]], 0, n_iters=1, assignments=a[b[rank]:b[rank + 1]],
        distances=d[b[rank]:b[rank + 1]],
        cluster_center_inds=[(0, 0), (0, 100)] if odd else [0, 100],
        random_state=1, make_shard=make_host_pam_shard))
    attempt("none_seed", lambda: sharded.fit_features_sharded(
        mine, 0, n_clusters=5, n_iters=1, random_state=None,
        make_shard=make_host_pam_shard))
    with open(os.path.join(outdir, "r%d.txt" % rank), "w") as f:
        f.write("\n".join(seen))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_raises(world):
    """ranks that disagree on the seed, a memberless cluster, a medoid away
    from its center on one rank: EVERY rank raises the same class, nobody is
    left in a collective, and the group still works afterwards (None as the
    seed everywhere: rank 0's draw for all)"""
    with tempfile.TemporaryDirectory() as d:
        _spawn(_error_worker, world, (d,))
        seen = [open(os.path.join(d, "r%d.txt" % r)).read().split("\n")
                for r in range(world)]
    want = ["seed_int:ImproperlyConfigured", "seed_state:ImproperlyConfigured",
            "seed_kind:ImproperlyConfigured", "memberless:ValueError",
            "far_medoid:DataInvalid", "some_of_three:ImproperlyConfigured",
            "seed_cold_props:ImproperlyConfigured",
            "some_of_three_one_rank:ImproperlyConfigured",
            "pairs_one_rank:ImproperlyConfigured",
            "none_seed:none"]
    for s in seen:
        assert s == want


def test_no_group_says_pam():
    from enspara_amd.cluster import KHybrid, KMedoids
    from enspara_amd.cluster.kmedoids import kmedoids
    from enspara_amd.exception import ImproperlyConfigured
    X = np.random.RandomState(0).normal(size=(50, 3))
    for f in (lambda: KHybrid("manhattan", n_clusters=3, mpi_mode=True).fit(X),
              lambda: KMedoids("euclidean", n_clusters=3, mpi_mode=True).fit(X)):
        with pytest.raises(ImproperlyConfigured, match="PAM sweep needs an "
                           "initialised torch.distributed process group"):
            f()
    with pytest.raises(ImproperlyConfigured, match="callable"):
        kmedoids(X, lambda A, y: np.zeros(len(A)), n_clusters=3, mpi_mode=True)
