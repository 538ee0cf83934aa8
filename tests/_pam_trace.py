"""Fixed PAM scenarios and what the window path does on them, sweep by sweep: the
medoids, the accept flags, and the counters that say which form every window took
(tests/test_gpu_pam_trace.py holds them against tests/golden/pam_window_trace.json;
`python tests/_pam_trace.py OUT.json` records that file).

The frames: 5 atoms around 40 templates laid out so that k-centers finds 32 small
clusters first and 8 large ones last (K = 40 in windows of 32: one full window whose
clusters hold a fifth of the frames -- a short list --, and one of 8 that holds the
rest -- a long one):
  * template 0, the hub, holds frame 0 (the first center);
  * 16 templates far from everything, 15 of them with a partner at about the reach
    of its members (an ambiguous member has another medoid to search: what a window
    with `pam_max_pairs` = 1 hands back);
  * 8 tight, populous templates near the hub -- nearer than partners are to each
    other, so they are found last, and farther than twice their own spread.
"""
import json
import os
import sys

import numpy as np

N_ATOMS = 5
K = 40
WIDTH = 32
N_LARGE, N_PER_SMALL = 8, 112

# name -> (frames, K, options, sweeps)
SCENARIOS = {
    "n16384": (16384, K, (), 2),
    "n16383": (16383, K, (), 2),
    # (every sweep opens with its waits at rest -- ek_pam_begin -- and has two windows:
    # this one shows the hand-back, the next one what the wait after it does)
    "n16384_max_pairs_1": (16384, K, (("pam_max_pairs", 1),), 12),
    "n16384_bounds_off": (16384, K, (("pam_bounds", 0),), 2),
    "n16384_one_workgroup_off": (16384, K, (("pam_one_workgroup", 0),), 2),
    # 400 small clusters, 13 windows and more a sweep, every list short: windows that
    # hand a proposal back, the windows of the wait behind each, the next one eligible
    "pairs_k400_max_pairs_1": (20000, 400, (("pam_max_pairs", 1),), 2),
}


def _step(rng, size):
    """a displacement of all atoms whose RMSD (before superposition) is `size`"""
    v = rng.normal(size=(N_ATOMS, 3))
    return v * (size * np.sqrt(N_ATOMS) / np.linalg.norm(v))


def frames(n, seed=20):
    rng = np.random.RandomState(seed)
    hub = rng.normal(size=(N_ATOMS, 3))
    tmpl, sigma = [hub], [0.004]
    for j in range(16):
        base = rng.normal(size=(N_ATOMS, 3))
        tmpl.append(base)
        sigma.append(0.02)
        if j < 15:
            tmpl.append(base + _step(rng, 0.17))
            sigma.append(0.02)
    for _ in range(N_LARGE):
        tmpl.append(hub + _step(rng, 0.13))
        sigma.append(0.004)
    n_small = len(tmpl) - N_LARGE
    assert len(tmpl) == K and n_small == 32
    which = np.repeat(np.arange(n_small), N_PER_SMALL)
    which = np.concatenate([which, n_small + np.arange(16384 - len(which)) % N_LARGE])
    which[1:] = rng.permutation(which[1:])      # (frame 0 stays with the hub)
    x = np.asarray(tmpl)[which] + rng.normal(size=(16384, N_ATOMS, 3)) * \
        np.asarray(sigma)[which][:, None, None]
    return np.ascontiguousarray(x[:n], dtype=np.float32)


def pair_frames(n, k, seed=21):
    """k / 2 pairs of partner templates, far from each other, n / k frames each"""
    rng = np.random.RandomState(seed)
    tmpl = []
    for _ in range(k // 2):
        base = rng.normal(size=(N_ATOMS, 3))
        tmpl += [base, base + _step(rng, 0.17)]
    which = rng.permutation(np.arange(n) % k)
    x = np.asarray(tmpl)[which] + rng.normal(size=(n, N_ATOMS, 3)) * 0.02
    return np.ascontiguousarray(x, dtype=np.float32)


def _counters(st):
    return [int(v) for v in st.pam_prefetch_stats() + st.pam_prefetch_passes() +
            st.pam_sparse_stats() + (st.pam_ahead_stats(),)]


def run(name):
    """-> {"first_window_share": .., "sweeps": [{"medoids", "accept", "counters"}]}"""
    from enspara_amd.cluster import kmedoids as km
    from enspara_amd.device import FrameStore
    n, K, options, n_sweeps = SCENARIOS[name]
    out = []
    with FrameStore.from_array(frames(n) if K == 40 else pair_frames(n, K)) as st:
        for key, value in (("pam_pairs_mfma", 1),) + tuple(options):   # (process-wide: said)
            st.set_option(key, value)
        st.reset_state()
        idx, _, _ = st.kcenters_run(0, K, 0.0)
        _, labels = st.download_state()
        share = float((labels < WIDTH).mean())
        med = np.ascontiguousarray([int(i) for i in idx], dtype=np.int64)
        rs = np.random.RandomState(5)
        for _ in range(n_sweeps):
            stream = km._DrawStream(rs)
            accept = np.zeros(K, dtype=np.int32)
            oc, nc = np.zeros(K), np.zeros(K)
            na = np.zeros(K, dtype=np.int64)
            st.pam_begin([int(m) for m in med])
            cid = 0
            while True:
                stream._need(stream.pos + 4 * (K - cid) + 64)
                status, cid, stream.pos = st.pam_sweep_run(
                    WIDTH, stream.raw, stream.pos, None, cid, med, accept, oc, nc, na)
                if status == 0:
                    break
                assert status == 1, "cluster %d is empty" % cid
                stream._need(len(stream.raw) + stream.BLOCK)
            stream.close()
            out.append({"medoids": [int(m) for m in med],
                        "accept": [int(a) for a in accept],
                        "counters": _counters(st)})
    return {"first_window_share": share, "sweeps": out}


def run_all():
    return {name: run(name) for name in SCENARIOS}


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    got = run_all()
    for name, r in got.items():
        print(name, "share of the first window's clusters %.3f" % r["first_window_share"],
              "counters", [s["counters"] for s in r["sweeps"]], flush=True)
    first = got["n16384"]["sweeps"][-1]["counters"]
    assert first[2] > 0 and first[4] > 0, "no restricted pass / one-workgroup window"
    for name in ("n16384_max_pairs_1", "pairs_k400_max_pairs_1"):
        assert got[name]["sweeps"][-1]["counters"][5] > 0, "no window ended early"
    for r in got.values():
        del r["first_window_share"]
    with open(sys.argv[1], "w") as f:
        json.dump(got, f, indent=0, sort_keys=True)
        f.write("\n")
