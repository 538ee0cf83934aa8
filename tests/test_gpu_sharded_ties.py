"""The RMSD multi-shard path (csrc/ek_mshard.hip, ek_api_ms.hip, ek_spec.hip,
ek_chain.hip, enspara_amd/sharded.py) at exact ties: frames that are copies of
one another within a shard and across shard boundaries (tests/_tied_cases.py),
and the degenerate structure families of tests/_structure_cases.py through
sharded rounds.  The reference's rule is "lowest rank wins ties"
(kcenters.py:337) = the lowest global index; the device spells it in the pick of
a shard's offers, in the combine of the maxima, in the plan's slot ranking and
greedy pick, and in the chain.  Every comparison is bit for bit with the
single-process oracle on the whole array.  The harness shapes are those of
tests/test_gpu_sharded.py; children regenerate the data from tests/."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import _tied_cases as tc
from test_gpu_sharded import _expected

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 120

_HEAD = r"""
import json, os, sys, threading, time
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _tied_cases as tc


def load(spec):
    # "tied:NAME" -> (x, K, K_more) ; "family:NAME" -> (x, 40, 0)
    kind, name = spec.split(":")
    if kind == "tied":
        shape = getattr(tc, name)
        x, _ = tc.tied_frames(*shape)
        K = {"MAIN": tc.MAIN_K, "TWO_SHARDS": tc.TWO_SHARDS_K,
             "EIGHT_SOME_EMPTY": tc.EIGHT_K}[name]
        return x, K, shape[2] + shape[2] // 3, shape[3]
    from _structure_cases import FIXED_ATOMS, structure_family
    return structure_family(name, 1000, FIXED_ATOMS.get(name, 7)), 40, 0, 3
"""


# ---- mailbox rounds between contexts of one process ------------------------------------
_CHILD_MBOX = _HEAD + r"""
from enspara_amd import sharded
from enspara_amd.device import FrameStore
from oracle import cluster as oc
spec, shards = sys.argv[2], int(sys.argv[3])
configs, modes = json.loads(sys.argv[4]), json.loads(sys.argv[5])
x, K, K_more, world = load(spec)
assert world == shards
n, A = x.shape[:2]
stores = []
for r in range(shards):
    lo, cnt = sharded.shard_bounds(n, shards, r)
    st = FrameStore(cnt, A, device=0, global_offset=lo)
    st.load(x[lo:lo + cnt])
    st.ms_setup(shards, r)
    # (allocated before any shard enters a run: an allocation inside ms_run waits
    # for the whole device, the other shards' waiting kernels included)
    st.reserve_centers(n)
    stores.append(st)
boxes = [st.ms_mailbox() for st in stores]
for st in stores:
    for p in range(shards):
        st.ms_connect(p, boxes[p][0], boxes[p][1])
out, errs = [None] * shards, []


def run(first, count, cutoff):
    def work(r):
        try:
            out[r] = stores[r].ms_run(first, count, cutoff)
        except Exception as e:      # noqa: BLE001 (reported below)
            errs.append("shard %d: %r" % (r, e))
    th = [threading.Thread(target=work, args=(r,)) for r in range(shards)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for r, st in enumerate(stores):
        assert st.ms_state()[2] == 0, (r, st.ms_state())
    return [np.array(o[0]) for o in out]


def check(tag, want):
    inds, wa, wd = want
    parts = [st.download_state() for st in stores]
    np.testing.assert_array_equal(np.concatenate([p[1] for p in parts]), wa, tag)
    np.testing.assert_array_equal(
        np.concatenate([p[0] for p in parts]).astype(np.float64), wd, tag)


def fresh():
    for st in stores:
        st.reset_state()
        st.sync()


wants = {}
ran = 0
for cands, two, sweep in configs:
    for st in stores:
        st.set_option(4, cands)
        st.set_option("ms_two_phase", two)
        st.set_option("pass_sweep", sweep)
    for mode in modes:
        tag = "%s shards=%d cands=%d two=%d sweep=%d %s" % (spec, shards, cands, two,
                                                          sweep, mode)
        if mode == "cut":
            cutoff, k_cut = tc.tied_cutoff(x, K, shards)
            Kr = 0
        else:
            cutoff, Kr = 0.0, K_more if mode == "more" else K
        if mode not in wants:
            wants[mode] = oc.kcenters(x, n_clusters=Kr or None,
                                      dist_cutoff=cutoff or None)
        inds, wa, wd = wants[mode]
        if mode == "cut":
            assert len(inds) == k_cut and wd.max() == cutoff
        fresh()
        t0 = time.time()
        if mode == "split":
            # the fit in two calls: a third of the centers, then the rest
            k1 = Kr // 3
            got = [np.concatenate(pair) for pair in
                   zip(run(0, k1, 0.0), run(k1, Kr - k1, 0.0))]
        else:
            got = run(0, Kr if Kr else n, cutoff)
        for r in range(shards):     # every shard reports the same centers
            np.testing.assert_array_equal(got[r], got[0], tag)
            np.testing.assert_array_equal(got[r], np.array(inds), tag)
        check(tag, wants[mode])
        # distances.max() after the last update (kcenters.py:226)
        assert out[0][2] == np.float32(wd.max()), (tag, out[0][2], wd.max())
        print("%s: %d centers, %.2f s" % (tag, len(inds), time.time() - t0), flush=True)
        ran += 1
print("ok", ran)
for st in stores:
    st.close()
"""


def _mbox(spec, shards, configs, modes):
    env = dict(os.environ)
    env["GPU_MAX_HW_QUEUES"] = "16"     # shards that wait for one another: a queue each
    p = subprocess.run([sys.executable, "-c", _CHILD_MBOX, ROOT, spec, str(shards),
                        json.dumps(configs), json.dumps(modes)], env=env,
                       capture_output=True, text=True, timeout=CHILD_SECONDS)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stdout.strip().splitlines()[-1] == "ok %d" % (len(configs) * len(modes))


_TIED_BY_SHARDS = {2: "TWO_SHARDS", 3: "MAIN", 8: "EIGHT_SOME_EMPTY"}
_MODES = ["count", "more", "cut", "split"]


# every width with every data / K mode at every shard count; both settings of
# ms_two_phase and of pass_sweep at every shard count (and, over the shard
# counts, with every width)
@pytest.mark.parametrize("shards,cands,two,sweep", [
    (2, 8, 0, 0), (2, 16, 1, 2), (2, 32, 0, 2), (2, -1, 1, 0),
    (3, 8, 1, 2), (3, 16, 0, 0), (3, 32, 1, 0), (3, -1, 0, 2),
    (8, 8, 1, 0), (8, 16, 0, 2), (8, 32, 1, 2), (8, -1, 0, 0)])
def test_tied_mailbox_rounds_between_contexts(shards, cands, two, sweep):
    """the shards are contexts of one process, every shard's loop in its own
    thread (ek_ms_run), on frames whose maxima are tied across the shard
    boundaries: K centers; more centers than distinct frames (3 shards: 80 of
    60); a cut-off that is exactly a tied maximum; the fit in two calls.  8
    shards: two hold no frames."""
    _mbox("tied:" + _TIED_BY_SHARDS[shards], shards, [(cands, two, sweep)], _MODES)


@pytest.mark.parametrize("family", ["identical", "rotated_copies", "collinear_exact",
                                    "two_atom_quantised", "scale_tiny", "scale_huge"])
def test_structure_families_through_sharded_rounds(family):
    """1000 frames of a degenerate family in 3 contexts (512 / 256 / 232), 40
    centers, rounds of 16 and the ladder, the exchange in one step and in two"""
    _mbox("family:" + family, 3, [(16, 0, 0), (16, 1, 0), (-1, 0, 0), (-1, 1, 0)],
          ["count"])


# ---- two processes on one GPU -----------------------------------------------------------
_GLOO = r"""
import torch
import torch.distributed as dist
rank, world, port, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
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
"""

_CHILD2 = _HEAD + _GLOO + r"""
from enspara_amd import sharded
from enspara_amd.device import FrameStore
K, iters, cands, transport, ti = (int(sys.argv[6]), int(sys.argv[7]), int(sys.argv[8]),
                                  sys.argv[9], int(sys.argv[10]))
x, _, _, w = load("tied:TWO_SHARDS")
assert w == world
n, A = x.shape[:2]
lo, cnt = sharded.shard_bounds(n, world, rank)
torch.cuda.set_device(0)
ts = torch.cuda.Stream(device=0)
with FrameStore(cnt, A, device=0, global_offset=lo, stream=ts.cuda_stream) as st:
    st.load(x[lo:lo + cnt])
    st.set_option(4, cands)
    st.reset_state()
    sh = sharded.DeviceShard(st)
    if transport == "ipc":      # the k-centers rounds exchange on the device (hipIpc)
        assert sharded.connect_mailboxes(sh)
    with torch.cuda.stream(ts):
        if ti:
            med, _ = sharded.kcenters_sharded(sh, 0, K, 0.0,
                                              use_triangle_inequality=True)
        else:
            med = sharded.khybrid_sharded(sh, K, 0.0, iters, random_state=5)
    d, a = st.download_state()
np.savez(out + ".%d.npz" % rank, med=np.array(med), d=d, a=a, lo=lo)
dist.barrier()
dist.destroy_process_group()
"""


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    return port


def _ranks(child, world, tmp_path, args):
    out = str(tmp_path / "r")
    port = _port()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["GPU_MAX_HW_QUEUES"] = "16"
    procs = [subprocess.Popen([sys.executable, "-c", child, ROOT, str(r), str(world),
                               port, out] + [str(a) for a in args], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for r in range(world)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=CHILD_SECONDS)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-4000:]
    return [np.load(out + ".%d.npz" % r) for r in range(world)]


@pytest.mark.parametrize("transport,cands,iters,ti", [
    ("gather", 16, 1, 0), ("ipc", 16, 1, 0), ("gather", 8, 1, 0), ("ipc", 8, 1, 0),
    ("gather", 1, 1, 0),        # the one-center exchange
    ("gather", 1, 0, 1)])       # use_triangle_inequality, against the plain oracle
def test_tied_two_device_shards_on_one_gpu(tmp_path, transport, cands, iters, ti):
    """two processes, a FrameStore each on the one GPU (collectives staged through
    gloo as in tests/test_gpu_sharded.py), tied frames, 40 centers and one PAM
    sweep whose proposals are drawn among copies"""
    K = tc.TWO_SHARDS_K
    parts = _ranks(_CHILD2, 2, tmp_path, [K, iters, cands, transport, ti])
    x, _ = tc.tied_frames(*tc.TWO_SHARDS)
    inds, wa, wd = _expected(x, K, iters, 5)
    for p in parts:
        np.testing.assert_array_equal(p["med"], inds)
    np.testing.assert_array_equal(np.concatenate([p["a"] for p in parts]), wa)
    np.testing.assert_array_equal(
        np.concatenate([p["d"] for p in parts]).astype(np.float64), wd)


# ---- the estimators' mpi_mode=True -------------------------------------------------------
_CHILD3 = _HEAD + _GLOO + r"""
from enspara_amd import sharded
from enspara_amd.cluster import KCenters, KHybrid
torch.cuda.set_device(0)
K = int(sys.argv[6])
x, _, _, w = load("tied:TWO_SHARDS")
n = len(x)
lo, cnt = sharded.shard_bounds(n, world, rank)
mine = x[lo:lo + cnt]
init = [x[i] for i in json.loads(sys.argv[7])]
kc = KCenters("rmsd", n_clusters=K, mpi_mode=True).fit(mine)
hy = KHybrid("rmsd", n_clusters=K, kmedoids_updates=2, random_state=3,
             mpi_mode=True).fit(mine)
ws = KCenters("rmsd", n_clusters=K, mpi_mode=True).fit(mine, init_centers=init)
wh = KHybrid("rmsd", n_clusters=K, kmedoids_updates=1, random_state=5,
             mpi_mode=True).fit(mine, init_centers=init)
res = {}
for key, est in (("kc", kc), ("hy", hy), ("ws", ws), ("wh", wh)):
    res[key + "_ci"] = np.array(est.center_indices_)
    res[key + "_a"], res[key + "_d"] = est.labels_, est.distances_
np.savez(out + ".%d.npz" % rank, **res)
dist.barrier()
dist.destroy_process_group()
"""


def test_tied_estimators_in_mpi_mode(tmp_path):
    """KCenters and KHybrid with mpi_mode=True at world 2 on tied frames, and a
    warm start whose init_centers are late copies of store frames, one of them
    twice: every occupied label is represented by the first copy in the global
    order, in another shard than the copy that was passed in"""
    from enspara_amd import sharded
    from oracle import cluster as oc
    n, A, B, world, seed = tc.TWO_SHARDS
    K = tc.TWO_SHARDS_K
    x, ids = tc.tied_frames(*tc.TWO_SHARDS)
    sp = tc.specials(n, B, world)
    every = np.flatnonzero(ids == 3)
    # (the copy that attracts nothing comes last, so that the loop's first new
    # label fills it: with an empty label in the middle the reference's own PAM
    # sweep draws from no members, kmedoids.py:514)
    init_frames = [int(every[-1]), int(np.flatnonzero(ids == sp["last_id"])[-1]),
                   int(sp["tail_pos"][-1]), int(every[len(every) // 2])]
    parts = _ranks(_CHILD3, world, tmp_path, [K, json.dumps(init_frames)])
    starts = [sharded.shard_bounds(n, world, r)[0] for r in range(world)]
    inds, a, d = oc.kcenters(x, n_clusters=K)
    rs = np.random.RandomState(3)
    wi, wd, wa = list(inds), d.copy(), a.copy()
    for _ in range(2):
        wi, wd, wa = oc.pam_update(x, wi, wa, wd, random_state=rs)
    init = [x[i] for i in init_frames]
    si, sa, sd = oc.kcenters(x, n_clusters=K, init_centers=init)
    assert [int(i) for i in si[:3]] == [int(every[0]), sp["last_pos"],
                                        int(sp["tail_pos"][0])]
    hi, hd, ha = oc.pam_update(x, list(si), sa.copy(), sd.copy(),
                               random_state=np.random.RandomState(5))
    for key, want_i, want_a, want_d in (("kc", inds, a, d), ("hy", wi, wa, wd),
                                        ("ws", si, sa, sd), ("wh", hi, ha, hd)):
        for p in parts:             # (rank, local index) pairs, kcenters.py:375-376
            got = [starts[int(r)] + int(i) for r, i in p[key + "_ci"]]
            assert got == [int(i) for i in want_i], key
        np.testing.assert_array_equal(
            np.concatenate([p[key + "_a"] for p in parts]), want_a, key)
        np.testing.assert_array_equal(
            np.concatenate([p[key + "_d"] for p in parts]), want_d, key)
