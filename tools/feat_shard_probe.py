"""Measurement only: microseconds per center of the sharded feature-space
k-centers step (csrc/ek_feat_kcenters.hip feat_shard_step_kernel, ONE launch per
center and shard) against the resident single-handle loop ek_feat_kcenters
(feat_step_kernel + feat_pick_kernel, two launches per center) on the same
data, in the same process, alternating.

  feat_shard_probe.py [--n 1000000] [--features 64] [--centers 1000]
                      [--repeats 5] [--out FILE] [--trace-only]

Three legs, float32 euclidean:
  resident  ek_feat_kcenters (state up / down inside the call)
  one       one FeatureShard under sharded.kcenters_sharded, no process group
            (what world == 1 runs, minus the one-rank all-gather)
  eight     the same samples as 8 handles of n / 8 on the one GPU and one
            stream, the records concatenated on the device between steps

Per leg and repeat the host clock is taken around a run of `centers` and a run
of `centers / 5` (both end in a device synchronise); the per-center figure is
the difference over the difference in centers, which cancels what a run costs
once (uploads, read-backs, the first record).  Reported: the median over the
repeats, and the spread (min .. max).  The centers, labels and distances of the
legs are compared before anything is timed.  --trace-only runs each leg once
for `centers / 5` centers and prints nothing: for a kernel trace by a profiler
around this script.  No GPU: the script fails, it has no CPU path."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12       # bytes / s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--centers", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    import torch
    from enspara_amd import sharded
    from enspara_amd.geometry.libdist import FeatureStore
    if not torch.cuda.is_available():
        raise SystemExit("feat_shard_probe: no GPU (nothing is measured on a CPU)")
    n, F, K = args.n, args.features, args.centers
    K0 = max(1, K // 5)
    X = np.random.RandomState(0).normal(size=(n, F)).astype(np.float32)
    ts = torch.cuda.Stream(device=0)
    whole = FeatureStore.from_array(X, 0, device=0, stream=ts.cuda_stream)
    shard = sharded.FeatureShard(whole, 0)
    S = 8
    cuts = [n * s // S for s in range(S + 1)]
    parts = [FeatureStore.from_array(X[cuts[s]:cuts[s + 1]], 0, device=0,
                                     global_offset=cuts[s],
                                     stream=ts.cuda_stream) for s in range(S)]
    rb = whole.record_bytes

    def resident(k):
        d = np.full(n, np.inf)
        a = np.full(n, -1, dtype=np.int32)
        t0 = time.perf_counter()
        c, _ = whole.kcenters(0, 0, k, 0.0, d, a)
        return time.perf_counter() - t0, c, d, a

    def one(k):
        with torch.cuda.stream(ts):
            shard.reset_state()
            ts.synchronize()
            t0 = time.perf_counter()
            c, _ = sharded.kcenters_sharded(shard, 0, k, 0.0)   # ends in a read-back
            dt = time.perf_counter() - t0
        d, a = shard.state()
        return dt, c, d, a

    def eight(k):
        with torch.cuda.stream(ts):
            mine = [torch.empty(rb, dtype=torch.uint8, device="cuda")
                    for _ in range(S)]
            for st in parts:
                st.reset_state()
            ts.synchronize()
            t0 = time.perf_counter()
            for st, m in zip(parts, mine):
                st.local_candidate(m.data_ptr())
            for label in range(k):
                everyone = torch.cat(mine)
                for st, m in zip(parts, mine):
                    st.kcenters_step(0, everyone.data_ptr(), S, label, 0.0,
                                     m.data_ptr())
            c, _, _ = parts[0].history(0, k)
            ts.synchronize()
            dt = time.perf_counter() - t0
        st8 = [p.download_state() for p in parts]
        return (dt, c, np.concatenate([d for d, _ in st8]),
                np.concatenate([a for _, a in st8]))

    legs = {"resident": resident, "one": one, "eight": eight}
    if args.trace_only:
        for f in legs.values():
            f(K0)
        return
    # same results first (and the warm-up of every kernel the timed runs use)
    ref = resident(K0)
    for name in ("one", "eight"):
        got = legs[name](K0)
        assert [int(i) for i in got[1]] == [int(i) for i in ref[1]], name
        assert np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), name
    per = {name: [] for name in legs}
    for _ in range(args.repeats):
        for name, f in legs.items():        # alternating
            t_small = f(K0)[0]
            t_big = f(K)[0]
            per[name].append((t_big - t_small) / (K - K0) * 1e6)
    bytes_per_center = n * F * 4 + n * 8     # the tiles once + the float64 distances
    res = {"n": n, "features": F, "centers": K, "repeats": args.repeats,
           "bytes_per_center": bytes_per_center}
    for name, v in per.items():
        med = float(np.median(v))
        res[name] = {"us_per_center": [round(x, 2) for x in v],
                     "median": round(med, 2), "min": round(min(v), 2),
                     "max": round(max(v), 2),
                     "fraction_of_8TBps": round(bytes_per_center / (med * 1e-6)
                                                / HBM_PEAK, 3)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
