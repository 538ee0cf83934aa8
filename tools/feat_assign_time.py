"""Time cluster.util.assign_to_nearest_center for the libdist metrics at the
README's feature shapes: the whole call (upload of X, the scan, the download)
and, where the library has it, ek_feat_assign_nearest alone with X resident
(center upload, launch, completion).  Runs on this commit and on its parent
(where the whole call is the per-center loop); the two JSON files are compared
by hand or with --against.

    python tools/feat_assign_time.py --label this --out profiles/feat_assign_time.json
    python tools/feat_assign_time.py --label parent --out ... (in the parent's tree)

Warm-up calls first, then the median of --repeats timed calls, host clock
around work that ends in a device synchronise.  Needs a GPU: no fallback."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [
    # name, n, F, dtype, metric, K
    ("f32_euclidean_k1000", 10 ** 6, 64, "float32", "euclidean", 1000),
    ("f32_euclidean_k5000", 10 ** 6, 64, "float32", "euclidean", 5000),
    ("f64_manhattan_k400", 10 ** 6, 16, "float64", "manhattan", 400),
]


def _median_time(f, warmup, repeats):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [float(t) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default=None, help="comma-separated shape names")
    ap.add_argument("--scale", type=float, default=1.0,
                    help="fraction of the samples (rehearsals)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("feat_assign_time: no GPU visible; nothing to measure")
    from enspara_amd import _lib
    from enspara_amd.cluster import util
    from enspara_amd.geometry import libdist
    has_kernel = hasattr(libdist._Resident, "assign_nearest")
    result = {"label": args.label, "device": torch.cuda.get_device_name(0),
              "repeats": args.repeats, "warmup": args.warmup, "shapes": {}}
    for name, n, F, dt, metric, K in SHAPES:
        if args.only and name not in args.only.split(","):
            continue
        n = max(int(n * args.scale), 1)
        rng = np.random.RandomState(7)
        X = rng.normal(size=(n, F)).astype(dt)
        Cs = X[rng.choice(n, size=min(K, n), replace=False)].copy()
        out = {}

        def whole():
            out["a"], out["d"] = util.assign_to_nearest_center(X, Cs, metric)
        t_whole, all_whole = _median_time(whole, args.warmup, args.repeats)
        row = {"n": n, "F": F, "dtype": dt, "metric": metric, "K": len(Cs),
               "whole_call_s": t_whole, "whole_call_all_s": all_whole,
               "terms": float(n) * F * len(Cs),
               "labels_sha1": hashlib.sha1(np.asarray(out["a"]).astype(
                   np.int64).tobytes()).hexdigest(),
               "distances_sha1": hashlib.sha1(np.asarray(out["d"]).astype(
                   np.float64).tobytes()).hexdigest()}
        if has_kernel:
            mid = util._get_distance_method(metric).device_metric_id
            res = libdist._Resident(X, libdist._KIND[dt], 0)
            L = res.L

            def resident():
                _lib.check(L.ek_feat_assign_nearest(
                    res._h, mid, Cs.ctypes.data_as(C.c_void_p), len(Cs)))
            t_res, all_res = _median_time(resident, max(args.warmup, 2),
                                          max(args.repeats, 7))
            row["resident_call_s"] = t_res
            row["resident_call_all_s"] = all_res
            row["resident_terms_per_s"] = row["terms"] / t_res
            del res
        result["shapes"][name] = row
        print(json.dumps({name: {k: v for k, v in row.items()
                                 if not k.endswith("_all_s")}}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
