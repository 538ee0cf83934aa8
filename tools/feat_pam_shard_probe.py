"""Cost per proposal of the sharded PAM sweep in feature space (measurement).

Times, on the same samples and the same start (k-centers on the device):
  single   ek_feat_pam_sweep, the single-process sweep;
  world1   pam_sweep_sharded over the product's shard -- sharded.FeatureShard as
           sharded._device_feature_shard builds it, on a torch stream of its
           own -- without a process group (the all-gathers are skipped);
  timed    the world1 run again through a proxy that adds up the host time
           spent inside each shard method (its total is not the headline);
  harness8 the same samples as 8 handles on one device behind the TEST harness
           tests/_feature_pam_handles.py, which waits for the stream and
           recombines the records on the host per proposal: a figure for the
           harness, not for eight GPUs and not for the product's path.
Prints one JSON line; --out also writes it to a file.  --only world1: that run
alone (what a kernel trace or a counter run wraps).

    python tools/feat_pam_shard_probe.py --n 1000000 --features 64 --medoids 1000
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Timed:
    """delegates to a shard, adding up wall time per method"""

    def __init__(self, shard):
        object.__setattr__(self, "_s", shard)
        object.__setattr__(self, "spent", {})
        object.__setattr__(self, "calls", {})

    def __getattr__(self, name):
        v = getattr(self._s, name)
        if not callable(v):
            return v

        def f(*a, **k):
            t0 = time.perf_counter()
            try:
                return v(*a, **k)
            finally:
                self.spent[name] = self.spent.get(name, 0.0) + time.perf_counter() - t0
                self.calls[name] = self.calls.get(name, 0) + 1
        return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--medoids", type=int, default=1000)
    ap.add_argument("--clustered", action="store_true")
    ap.add_argument("--only", default=None, choices=[None, "world1"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from enspara_amd import sharded
    from enspara_amd.cluster import kmedoids as km
    from enspara_amd.cluster import util
    from enspara_amd.geometry import libdist
    n, F, K = args.n, args.features, args.medoids
    rng = np.random.RandomState(0)
    if args.clustered:
        ctr = rng.normal(size=(K, F)) * 4
        X = (ctr[rng.randint(0, K, size=n)] + rng.normal(size=(n, F))).astype(np.float32)
    else:
        X = rng.normal(size=(n, F)).astype(np.float32)
    med, d0, a0, _ = libdist.kcenters_resident(
        X, 0, 0, K, 0.0, np.full(n, np.inf), np.full(n, -1, dtype=np.int64))
    med = [int(i) for i in med]
    res = {"n": n, "features": F, "medoids": K, "clustered": bool(args.clustered)}

    single = None
    if args.only is None:
        metric = util._get_distance_method("euclidean").bind(X)
        for rep in range(2):                    # (the second run is the warm one)
            rs = np.random.RandomState(1)
            t0 = time.perf_counter()
            single = km._kmedoids_pam_update(X, metric, list(med), a0.copy(),
                                             d0.copy(), random_state=rs)
            res["single_us_per_proposal"] = (time.perf_counter() - t0) / K * 1e6

    with sharded._device_feature_shard(X, 0, 0) as shard:
        for rep in range(2):
            shard.set_state(d0, a0.astype(np.int32))
            rs = np.random.RandomState(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m2 = sharded.pam_sweep_sharded(shard, list(med), random_state=rs)
            torch.cuda.synchronize()
            res["world1_us_per_proposal"] = (time.perf_counter() - t0) / K * 1e6
        d2, a2 = shard.state()
        if single is not None:
            res["world1_equals_single"] = bool(
                m2 == [int(i) for i in single[0]] and np.array_equal(d2, single[1])
                and np.array_equal(a2, single[2]))
        if args.only is None:
            timed = _Timed(shard)
            shard.set_state(d0, a0.astype(np.int32))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sharded.pam_sweep_sharded(timed, list(med),
                                      random_state=np.random.RandomState(1))
            torch.cuda.synchronize()
            res["timed_us_per_proposal"] = (time.perf_counter() - t0) / K * 1e6
            res["timed_us_per_proposal_by_method"] = {
                k: round(v / K * 1e6, 2) for k, v in sorted(timed.spent.items())}
            res["timed_calls_per_sweep"] = dict(sorted(timed.calls.items()))

    if args.only is None:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from _feature_pam_handles import Handles
        h = Handles(X, 0, [int(v) for v in np.linspace(0, n, 9)])
        try:
            for rep in range(2):
                h.set_state(d0, a0)
                rs = np.random.RandomState(1)
                with torch.cuda.stream(h.ts):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    sharded.pam_sweep_sharded(h, list(med), random_state=rs)
                    torch.cuda.synchronize()
                    res["harness8_us_per_proposal"] = (time.perf_counter() - t0) / K * 1e6
        finally:
            h.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
