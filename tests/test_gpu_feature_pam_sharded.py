"""Sharded PAM sweeps for the feature metrics on the device (gfx950).

(a) 1, 2, 3 and 8 ek_feat handles on one device, driven in-process through
enspara_amd.sharded.pam_sweep_sharded by a shard object that exchanges the
handles' tables and records as a process group would: medoids, labels and
float64 distances equal tests/_feature_pam_mpi_want.py (the host restatement of
the reference's MPI sweep, pinned to oracle/cluster.py in
tests/test_feature_pam_gloo.py) exactly, for every element kind, 1 to a few
thousand features, more than 256 medoids, ties across shard boundaries and an
empty shard.  (b) child processes at worlds 1 to 3 through KHybrid / KMedoids
with mpi_mode=True; at world 1 also against hybrid(mpi_mode=False), bit for
bit."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
pytestmark = pytest.mark.gpu
EUCLIDEAN, MANHATTAN, HAMMING = 0, 1, 2
from _feature_pam_handles import Handles as _Handles  # noqa: E402


def _cuts(n, S, rng):
    if S == 1:
        return [0, n]
    inner = sorted(int(v) for v in rng.choice(np.arange(1, n), size=S - 1,
                                              replace=False))
    if S >= 3:
        inner[1] = inner[0]                 # shard 1 owns nothing
    return [0] + inner + [n]


def _make(mid, dtype, n, F, seed):
    rng = np.random.RandomState(seed)
    if np.issubdtype(np.dtype(dtype), np.integer):
        return rng.randint(0, 3, size=(n, F)).astype(dtype)
    return rng.normal(size=(n, F)).astype(dtype)


def _sweeps_on_handles(X, mid, cuts, med, a, d, sweeps, seed, props):
    import torch
    from enspara_amd import sharded
    h = _Handles(X, mid, cuts)
    try:
        h.set_state(d, a)
        rs = np.random.RandomState(seed)
        with torch.cuda.stream(h.ts):
            for _ in range(sweeps):
                med = sharded.pam_sweep_sharded(h, med, proposals=props,
                                                random_state=rs)
        dd, aa = h.state()
    finally:
        h.close()
    return med, dd, aa, rs.randint(1 << 30), h.max_amb


def _compare(X, mid, K, sweeps=2, seed=3, shards=(1, 2, 3, 8), props=None):
    import _feature_pam_mpi_want as w
    med0, a0, d0 = w.start_kcenters(X, mid, K)
    rng = np.random.RandomState(seed)
    moved = False
    for S in shards:
        cuts = _cuts(len(X), S, rng)
        rs = np.random.RandomState(seed)
        wm, wd, wa = med0, d0, a0
        for _ in range(sweeps):
            wm, wd, wa = w.pam_update_mpi(X, mid, wm, wa, wd, cuts,
                                          proposals=props, random_state=rs)
        gm, gd, ga, after, max_amb = _sweeps_on_handles(
            X, mid, cuts, med0, a0, d0, sweeps, seed, props)
        assert gm == wm, (S, cuts)
        np.testing.assert_array_equal(gd, wd)
        np.testing.assert_array_equal(ga.astype(np.int64), wa)
        assert gd.dtype == np.float64 and ga.dtype == np.int32
        assert after == rs.randint(1 << 30)     # the same draws were consumed
        moved = moved or gm != med0
        assert max_amb > 0
    assert moved


CASES = [
    # metric, dtype, n, n_features, K
    (EUCLIDEAN, np.float32, 1037, 64, 20),
    (MANHATTAN, np.float32, 1300, 3, 25),
    (EUCLIDEAN, np.float64, 2500, 1, 15),
    (MANHATTAN, np.float64, 777, 64, 12),
    (MANHATTAN, np.float32, 600, 2049, 7),      # one feature past FY_CHUNK
    (EUCLIDEAN, np.float64, 520, 2049, 6),
    (EUCLIDEAN, np.float32, 500, 4100, 6),      # three chunks
    (HAMMING, np.int64, 1500, 12, 20),
    (HAMMING, np.int8, 900, 64, 15),
    (HAMMING, np.uint16, 300, 2049, 5),
    (EUCLIDEAN, np.float32, 9000, 8, 300),      # two chunks of 256 medoids
]


@pytest.mark.parametrize("mid,dtype,n,F,K", CASES)
def test_sweeps_over_handles(mid, dtype, n, F, K):
    _compare(_make(mid, dtype, n, F, 5), mid, K,
             shards=(1, 3) if K > 256 else (1, 2, 3, 8))


def test_ties_across_shard_boundaries_and_explicit_proposals():
    """small integers: equal distances everywhere, also between samples on
    different shards; manhattan on them sums exactly, so every sharding must
    give the one-shard result"""
    import _feature_pam_mpi_want as w
    X = _make(MANHATTAN, np.int32, 2000, 4, 1)
    _compare(X, MANHATTAN, 16)
    props = [int(v) for v in np.random.RandomState(2).choice(2000, 16, False)]
    _compare(X, MANHATTAN, 16, sweeps=1, props=props)
    med, a, d = w.start_kcenters(X, MANHATTAN, 16)
    one = w.pam_update_mpi(X, MANHATTAN, med, a, d, [0, 2000],
                           random_state=np.random.RandomState(3))
    got = _sweeps_on_handles(X, MANHATTAN, [0, 300, 300, 1111, 2000], med, a, d,
                             1, 3, None)
    assert got[0] == one[0]
    np.testing.assert_array_equal(got[1], one[1])


def test_protocol_errors():
    import torch
    from enspara_amd import _lib
    from enspara_amd.geometry.libdist import FeatureStore
    X = _make(EUCLIDEAN, np.float32, 300, 4, 0)
    with FeatureStore.from_array(X, 0, device=0) as st:
        buf = torch.zeros(64, dtype=torch.float32, device="cuda")
        with pytest.raises(_lib.HipError):      # no state yet
            st.pam_begin(0, buf.data_ptr(), 2)
        st.reset_state()
        with pytest.raises(_lib.HipError):      # no sweep begun
            st.pam_propose(0, buf.data_ptr(), 0, 1, buf.data_ptr())
        with pytest.raises(_lib.HipError):      # not this shard's sample
            st.pam_gather_rows([300], [0], buf.data_ptr())
        st.pam_begin(0, buf.data_ptr(), 2)
        with pytest.raises(_lib.HipError):      # cluster out of range
            st.pam_propose(2, buf.data_ptr(), 0, 1, buf.data_ptr())
        with pytest.raises(_lib.HipError):      # nothing proposed
            st.pam_commit(True)
        with pytest.raises(_lib.HipError):      # 33 clusters in a window
            st.pam_count_members_batch(0, 33)


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
from enspara_amd.cluster import KHybrid, KMedoids
from enspara_amd.cluster.hybrid import hybrid
from enspara_amd.cluster.kmedoids import kmedoids
from enspara_amd.geometry import libdist
n, K = int(sys.argv[7]), int(sys.argv[8])
rng = np.random.RandomState(13)
x = rng.normal(size=(n, 6)).astype(np.float32)
xi = rng.randint(0, 3, size=(n, 10)).astype(np.int16)
lo, cnt = sharded.shard_bounds(n, world, rank)
mine, mine_i = x[lo:lo + cnt], xi[lo:lo + cnt]
res = {
    "e": KHybrid("euclidean", n_clusters=K, kmedoids_updates=2, random_state=4,
                 mpi_mode=True).fit(mine).result_,
    "m": KHybrid("cityblock", n_clusters=K, kmedoids_updates=1, random_state=5,
                 mpi_mode=True).fit(mine.astype(np.float64)).result_,
    "h": hybrid(mine_i, libdist.hamming, n_iters=2, n_clusters=K,
                random_state=np.random.RandomState(6), mpi_mode=True),
    "k": kmedoids(mine, "euclidean", n_clusters=K, n_iters=2, random_state=7,
                  mpi_mode=True),
}
km = KMedoids("manhattan", n_clusters=K, n_iters=1, mpi_mode=True)
a0 = np.load(out + ".warm.npz")
res["w"] = km.fit(mine, assignments=a0["a"][lo:lo + cnt],
                  distances=a0["d"][lo:lo + cnt],
                  cluster_center_inds=[int(v) for v in a0["med"]]).result_
res["wk"] = kmedoids(mine, "manhattan", n_iters=1, assignments=a0["a"][lo:lo + cnt],
                     distances=a0["d"][lo:lo + cnt],
                     cluster_center_inds=[int(v) for v in a0["med"]],
                     random_state=8, mpi_mode=True)
init = [x[5], x[n // 2], x[7]]
res["i"] = KHybrid("euclidean", n_clusters=K, kmedoids_updates=1, random_state=9,
                   mpi_mode=True).fit(mine, init_centers=init).result_
if world == 1:
    res["s"] = hybrid(x, "euclidean", n_iters=2, n_clusters=K,
                      random_state=np.random.RandomState(4), mpi_mode=False)
o = {}
for key, r in res.items():
    ci = np.array(r.center_indices)
    o[key + "_ci"] = ci.reshape(-1, 2) if key != "s" else ci
    o[key + "_a"], o[key + "_d"] = r.assignments, r.distances
    o[key + "_c"] = np.array(r.centers)
np.savez(out + ".%d.npz" % rank, **o)
dist.barrier()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("world,backend,n,K", [(1, "nccl", 3000, 20),
                                               (2, "gloo", 3000, 20),
                                               (3, "gloo", 500, 12)])
def test_estimators_in_mpi_mode(tmp_path, world, backend, n, K):
    # (3 ranks over 500 samples = 2 tiles: the last rank owns no samples)
    import _feature_pam_mpi_want as w
    from enspara_amd import sharded
    rng = np.random.RandomState(13)
    x = rng.normal(size=(n, 6)).astype(np.float32)
    xi = rng.randint(0, 3, size=(n, 10)).astype(np.int16)
    starts = [sharded.shard_bounds(n, world, r)[0] for r in range(world)] + [n]
    wmed, wa, wd = w.start_kcenters(x, MANHATTAN, K)
    out = str(tmp_path / "r")
    np.savez(out + ".warm.npz", a=wa, d=wd, med=np.array(wmed))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    procs = [subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, str(r),
                               str(world), port, out, backend, str(n), str(K)],
                              env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    logs = [p.communicate(timeout=600)[0] for p in procs]
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-4000:]
    parts = [np.load(out + ".%d.npz" % r) for r in range(world)]
    cold = w.cold_medoids(n, K, 7)
    ca, cd = w.start_nearest(x, EUCLIDEAN, cold)
    rs = np.random.RandomState(7)
    k = (cold, cd, ca)
    for _ in range(2):
        k = w.pam_update_mpi(x, EUCLIDEAN, k[0], k[2], k[1], starts,
                             random_state=rs)
    wants = {
        "e": (x, w.khybrid_want(x, EUCLIDEAN, K, 2, 4, starts)),
        "m": (x.astype(np.float64),
              w.khybrid_want(x.astype(np.float64), MANHATTAN, K, 1, 5, starts)),
        "h": (xi, w.khybrid_want(xi, HAMMING, K, 2, 6, starts)),
        "k": (x, k),
        "wk": (x, w.pam_update_mpi(x, MANHATTAN, wmed, wa, wd, starts,
                                   random_state=np.random.RandomState(8))),
        "i": (x, w.khybrid_want(x, EUCLIDEAN, K, 1, 9, starts,
                                [x[5], x[n // 2], x[7]])),
    }
    for key, (X, (med, d, a)) in wants.items():
        for p in parts:
            got = [starts[int(r)] + int(i) for r, i in p[key + "_ci"]]
            assert got == med, key
            assert p[key + "_c"].dtype == X.dtype, key
            np.testing.assert_array_equal(p[key + "_c"], X[med])
        np.testing.assert_array_equal(
            np.concatenate([p[key + "_a"] for p in parts]), a)
        np.testing.assert_array_equal(
            np.concatenate([p[key + "_d"] for p in parts]), d)
    # the KMedoids ESTIMATOR takes no random_state (as in the reference): its
    # warm-started fit draws from a seed of rank 0's, so only this can be said:
    # every rank reports the same medoids, each at distance 0
    for p in parts:
        np.testing.assert_array_equal(p["w_ci"], parts[0]["w_ci"])
    wd_all = np.concatenate([p["w_d"] for p in parts])
    for lab, (r, i) in enumerate(parts[0]["w_ci"]):
        g = starts[int(r)] + int(i)
        assert wd_all[g] == 0.0, lab
    if world == 1:
        p = parts[0]
        assert [int(i) for _, i in p["e_ci"]] == [int(i) for i in p["s_ci"]]
        np.testing.assert_array_equal(p["e_a"], p["s_a"])
        np.testing.assert_array_equal(p["e_d"], p["s_d"])
        np.testing.assert_array_equal(p["e_c"], p["s_c"])
