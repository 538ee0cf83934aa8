"""k-centers with a feature metric over several shards on the device
(csrc/ek_feat_kcenters.hip feat_shard_step_kernel; enspara_amd/sharded.py
FeatureShard / fit_features_sharded).

First group: the C ABI in one process -- 1, 2, 3 and 8 shards as separate
ek_feat handles on the one GPU, the records concatenated on the device between
steps.  Second group: child processes on GPU 0 running the estimators with
mpi_mode=True (world 1 over nccl; 2 and 3 over gloo with stream-synchronising
wrappers, as tests/test_gpu_sharded.py::test_estimators_in_mpi_mode).

Every comparison is exact (centers, int labels, float64 distances).  The
want-side is the single-process reference-shaped host loop
(cluster/kcenters.py _kcenters_host) around the ORACLE's metric
(oracle/features.py), never the code under test; the existing single-handle
ek_feat_kcenters is compared as well."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EUCLIDEAN, MANHATTAN, HAMMING = 0, 1, 2


def _oracle_metric(mid):
    from oracle import features as of
    f = {0: of.euclidean, 1: of.manhattan, 2: of.hamming}[mid]
    return lambda A, y: f(np.asarray(A), np.asarray(y))


def _want(X, mid, K, cutoff=0.0):
    from enspara_amd.cluster.kcenters import kcenters
    return kcenters(X, _oracle_metric(mid), n_clusters=K, dist_cutoff=cutoff)


def _cuts(n, S, rng):
    """S contiguous shards of n samples: uneven, not on multiples of 256, and
    (from 3 shards on) one of them without samples"""
    if S == 1:
        return [0, n]
    inner = sorted(int(v) for v in rng.choice(np.arange(1, n), size=S - 1,
                                              replace=False))
    if S >= 3:
        inner[1] = inner[0]                 # shard 1 owns nothing
    return [0] + inner + [n]


def _run_shards(X, mid, cuts, K, cutoff=0.0):
    """K steps enqueued at once over len(cuts) - 1 handles -> (center global
    indices, their pre-update distances, distances, labels)"""
    import torch
    from enspara_amd.geometry.libdist import FeatureStore
    S = len(cuts) - 1
    ts = torch.cuda.Stream(device=0)
    stores = [FeatureStore.from_array(X[cuts[s]:cuts[s + 1]], mid, device=0,
                                      global_offset=cuts[s],
                                      stream=ts.cuda_stream) for s in range(S)]
    try:
        rb = stores[0].record_bytes
        assert rb % 16 == 0 and rb >= 16 + X.shape[1] * (
            4 if X.dtype == np.float32 and mid != HAMMING else 8)
        with torch.cuda.stream(ts):
            mine = [torch.empty(rb, dtype=torch.uint8, device="cuda")
                    for _ in range(S)]
            for st, m in zip(stores, mine):
                st.reset_state()
                st.local_candidate(m.data_ptr())
            for label in range(K):
                everyone = torch.cat(mine)  # on the device, in stream order
                for st, m in zip(stores, mine):
                    st.kcenters_step(mid, everyone.data_ptr(), S, label,
                                     cutoff, m.data_ptr())
        hist = [st.history(0, K) for st in stores]
        state = [st.download_state() for st in stores]
    finally:
        for st in stores:
            st.close()
    n_done = hist[0][2]
    for idx, cd, nd in hist:                # every shard: the same decisions
        assert nd == n_done
        np.testing.assert_array_equal(idx[:nd], hist[0][0][:nd])
        np.testing.assert_array_equal(cd[:nd], hist[0][1][:nd])
        assert np.all(idx[nd:] == -1)
    return (hist[0][0][:n_done], hist[0][1][:n_done],
            np.concatenate([d for d, _ in state]),
            np.concatenate([a for _, a in state]))


def _compare(X, mid, K, cutoff, want, shards=(1, 2, 3, 8), seed=0):
    from enspara_amd.geometry import libdist
    rng = np.random.RandomState(seed)
    n = len(X)
    # the existing single-handle loop
    ci, d1, a1, _ = libdist.kcenters_resident(
        X, mid, 0, K, cutoff, np.full(n, np.inf), np.full(n, -1, dtype=np.int64))
    assert [int(i) for i in ci] == [int(i) for i in want.center_indices]
    np.testing.assert_array_equal(d1, want.distances)
    np.testing.assert_array_equal(a1, want.assignments)
    for S in shards:
        cuts = _cuts(n, S, rng)
        idx, cd, d, a = _run_shards(X, mid, cuts, K, cutoff)
        assert [int(i) for i in idx] == [int(i) for i in want.center_indices], (S, cuts)
        np.testing.assert_array_equal(d, want.distances)
        np.testing.assert_array_equal(a.astype(np.int64), want.assignments)
        assert d.dtype == np.float64 and a.dtype == np.int32
        assert np.all(np.diff(cd) <= 0) and cd[0] == np.inf


CASES = [
    # metric, dtype, n, n_features, K
    (EUCLIDEAN, np.float32, 1037, 64, 20),
    (MANHATTAN, np.float32, 1300, 3, 25),
    (EUCLIDEAN, np.float64, 2500, 1, 15),
    (MANHATTAN, np.float64, 777, 64, 12),
    (MANHATTAN, np.float32, 600, 2049, 7),      # one feature past FY_CHUNK
    (EUCLIDEAN, np.float64, 520, 2049, 6),
    (EUCLIDEAN, np.float32, 500, 5000, 6),      # three chunks
    (HAMMING, np.int64, 1500, 12, 20),
    (HAMMING, np.int8, 900, 64, 15),
    (HAMMING, np.uint16, 300, 2049, 5),
]


def _make(mid, dtype, n, F, seed):
    rng = np.random.RandomState(seed)
    if mid == HAMMING:
        return rng.randint(0, 3, size=(n, F)).astype(dtype)
    return rng.normal(size=(n, F)).astype(dtype)


@pytest.mark.parametrize("mid,dtype,n,F,K", CASES)
def test_count_mode(mid, dtype, n, F, K):
    X = _make(mid, dtype, n, F, n + F)
    want = _want(X, mid, K)
    assert len(want.center_indices) == K
    _compare(X, mid, K, 0.0, want, seed=F)


@pytest.mark.parametrize("mid,dtype,n,F,K", [CASES[0], CASES[3], CASES[4],
                                             CASES[7]])
def test_cutoff_stops_mid_batch(mid, dtype, n, F, K):
    """the cut-off is distances.max() after about half of the K centers: the K
    steps are enqueued at once and the later ones must leave nothing behind"""
    X = _make(mid, dtype, n, F, n + F + 1)
    cutoff = float(_want(X, mid, K // 2).distances.max())
    want = _want(X, mid, K, cutoff)
    assert 0 < len(want.center_indices) < K
    _compare(X, mid, K, cutoff, want, seed=F + 1)


def test_ties_across_shard_boundaries():
    """small-integer-valued rows, each present many times in every shard: the
    maximum is tied between shards at every step and the lowest shard's first
    sample must win (np.argmax's first index over the concatenated data)"""
    rng = np.random.RandomState(11)
    for mid, dtype in ((EUCLIDEAN, np.float32), (MANHATTAN, np.float64),
                       (HAMMING, np.int64)):
        base = rng.randint(0, 3, size=(30, 7))
        X = base[rng.randint(0, 30, size=1111)].astype(dtype)
        want = _want(X, mid, 25)
        _compare(X, mid, 25, 0.0, want, seed=5)


def test_all_samples_identical_and_more_clusters_than_samples():
    X = np.full((700, 5), 1.5, dtype=np.float32)
    want = _want(X, EUCLIDEAN, 4)
    assert list(want.center_indices) == [0]         # max_dist is 0 after it
    _compare(X, EUCLIDEAN, 4, 0.0, want, seed=1)
    X = np.random.RandomState(2).normal(size=(37, 3))
    want = _want(X, MANHATTAN, 60)
    assert len(want.center_indices) == 37
    _compare(X, MANHATTAN, 60, 0.0, want, seed=2)


def test_driver_without_a_group():
    """sharded.kcenters_sharded over one FeatureShard, no process group: the
    count mode, the cut-off mode (progress every few steps) and a second call
    that continues the first"""
    import torch
    from enspara_amd import sharded
    from enspara_amd.geometry.libdist import FeatureStore
    X = _make(EUCLIDEAN, np.float32, 3001, 17, 8)
    cutoff = float(_want(X, EUCLIDEAN, 13).distances.max())
    for K, c in ((30, 0.0), (40, cutoff)):
        want = _want(X, EUCLIDEAN, K, c)
        ts = torch.cuda.Stream(device=0)
        with FeatureStore.from_array(X, EUCLIDEAN, device=0,
                                     stream=ts.cuda_stream) as st:
            sh = sharded.FeatureShard(st, EUCLIDEAN)
            with torch.cuda.stream(ts):
                sh.reset_state()
                idx, cd = sharded.kcenters_sharded(sh, 0, 5, c, check_every=4)
                idx2, _ = sharded.kcenters_sharded(sh, 5, K - 5, c,
                                                   check_every=4, fresh=False)
            d, a = sh.state()
        got = [int(i) for i in idx] + [int(i) for i in idx2]
        assert got == [int(i) for i in want.center_indices]
        np.testing.assert_array_equal(d, want.distances)
        np.testing.assert_array_equal(a.astype(np.int64), want.assignments)


def test_argument_errors():
    import ctypes as C
    from enspara_amd import _lib
    L = _lib.load()
    assert L.ek_feat_record_bytes(64, 0) == 16 + 256
    assert L.ek_feat_record_bytes(3, 0) == 32
    assert L.ek_feat_record_bytes(3, 2) == 48
    assert L.ek_feat_record_bytes(0, 0) == 0
    h = C.c_void_p()
    assert L.ek_feat_create_sharded(0, 10, 3, 0, -1, None, C.byref(h)) == _lib.EK_EARG
    assert L.ek_feat_kcenters_step(None, 0, None, 1, 0, 0.0, None) == _lib.EK_EARG
    assert L.ek_feat_create_sharded(0, 10, 3, 0, 0, None, C.byref(h)) == 0
    try:        # no samples loaded, no state: an error, not a launch
        assert L.ek_feat_local_candidate(h, C.c_void_p(16)) == _lib.EK_ESTATE
    finally:
        L.ek_feat_destroy(h)


# ---- the estimators' mpi_mode=True (every rank passes its own samples) ------------
_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
import torch.distributed as dist
rank, world, port, out, backend = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5], sys.argv[6]
torch.cuda.set_device(0)
if backend == "nccl":
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", port)
    dist.init_process_group("nccl", rank=rank, world_size=world,
                            device_id=torch.device("cuda", 0))
else:
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + port,
                            rank=rank, world_size=world)
    _agit, _ar = dist.all_gather_into_tensor, dist.all_reduce
    def agit(out_t, in_t, group=None):
        torch.cuda.current_stream().synchronize()
        o = torch.empty(out_t.shape, dtype=out_t.dtype)
        _agit(o, in_t.cpu(), group=group)
        out_t.copy_(o)
    def ar(t, op=dist.ReduceOp.SUM, group=None):
        torch.cuda.current_stream().synchronize()
        h = t.cpu()
        _ar(h, op=op, group=group)
        t.copy_(h)
    dist.all_gather_into_tensor, dist.all_reduce = agit, ar
from enspara_amd import sharded
from enspara_amd.cluster import KCenters
from enspara_amd.cluster.kcenters import kcenters, kcenters_mpi
from enspara_amd.geometry import libdist
n, K, radius = int(sys.argv[7]), int(sys.argv[8]), float(sys.argv[9])
rng = np.random.RandomState(13)
x = rng.normal(size=(n, 6)).astype(np.float32)
xi = rng.randint(0, 3, size=(n, 10)).astype(np.int16)
lo, cnt = sharded.shard_bounds(n, world, rank)
mine, mine_i = x[lo:lo + cnt], xi[lo:lo + cnt]
init = [x[5], x[n // 2], x[7], x[5]]
res = {
    "e": KCenters("euclidean", n_clusters=K, mpi_mode=True).fit(mine).result_,
    "m": KCenters("manhattan", cluster_radius=radius, mpi_mode=True).fit(mine).result_,
    "b": KCenters("cityblock", n_clusters=K, cluster_radius=radius,
                  mpi_mode=True).fit(mine.astype(np.float64)).result_,
    "we": KCenters("euclidean", n_clusters=K, mpi_mode=True).fit(
        mine, init_centers=init).result_,
    "wm": KCenters("manhattan", n_clusters=K, mpi_mode=True).fit(
        mine, init_centers=init).result_,
    "h": kcenters(mine_i, libdist.hamming, n_clusters=K, mpi_mode=True),
    "f": kcenters_mpi(mine, libdist.euclidean, n_clusters=K),
}
o = {}
for key, r in res.items():
    o[key + "_ci"] = np.array(r.center_indices).reshape(-1, 2)
    o[key + "_a"], o[key + "_d"] = r.assignments, r.distances
    o[key + "_c"] = np.array(r.centers)
np.savez(out + ".%d.npz" % rank, **o)
dist.barrier()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("world,backend,n,K", [(1, "nccl", 3000, 20),
                                               (2, "gloo", 3000, 20),
                                               (3, "gloo", 500, 12)])
def test_estimators_in_mpi_mode_with_feature_metrics(tmp_path, world, backend,
                                                     n, K):
    # (3 ranks over 500 samples = 2 tiles: the last rank owns no samples)
    from enspara_amd import sharded
    from enspara_amd.cluster.kcenters import kcenters
    rng = np.random.RandomState(13)
    x = rng.normal(size=(n, 6)).astype(np.float32)
    xi = rng.randint(0, 3, size=(n, 10)).astype(np.int16)
    init = [x[5], x[n // 2], x[7], x[5]]
    radius = float(_want(x, MANHATTAN, K // 2).distances.max())
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    out = str(tmp_path / "r")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, str(r),
                               str(world), port, out, backend, str(n), str(K),
                               repr(radius)],
                              env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-4000:]
    parts = [np.load(out + ".%d.npz" % r) for r in range(world)]
    starts = [sharded.shard_bounds(n, world, r)[0] for r in range(world)]
    e, m = _oracle_metric(EUCLIDEAN), _oracle_metric(MANHATTAN)
    wants = {
        "e": kcenters(x, e, n_clusters=K),
        "m": kcenters(x, m, dist_cutoff=radius),
        "b": kcenters(x.astype(np.float64), m, n_clusters=K, dist_cutoff=radius),
        "we": kcenters(x, e, n_clusters=K, init_centers=init),
        "wm": kcenters(x, m, n_clusters=K, init_centers=init),
        "h": kcenters(xi, _oracle_metric(HAMMING), n_clusters=K),
        "f": kcenters(x, e, n_clusters=K),
    }
    assert len(wants["m"].center_indices) == K // 2
    assert len(wants["we"].centers) == 4 + K - 3    # the second x[5] attracts nothing
    for key, want in wants.items():
        for p in parts:             # (rank, local index) pairs, kcenters.py:375-376
            got = [starts[int(r)] + int(i) for r, i in p[key + "_ci"]]
            assert got == [int(i) for i in want.center_indices], key
            assert p[key + "_c"].dtype == np.array(want.centers).dtype, key
            np.testing.assert_array_equal(p[key + "_c"], np.array(want.centers))
        np.testing.assert_array_equal(
            np.concatenate([p[key + "_a"] for p in parts]), want.assignments)
        np.testing.assert_array_equal(
            np.concatenate([p[key + "_d"] for p in parts]), want.distances)
