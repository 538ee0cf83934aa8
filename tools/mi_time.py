#!/usr/bin/env python3
"""Time enspara_amd.info_theory on the device at a CARDS-like shape, from a host array.

    python tools/mi_time.py [--frames 1000000] [--features 1000] [--states 3]
                            [--repeats 3] [--cpu-frames 16384]

One JSON line.  X and Y are two seeded int8 arrays [frames, features].  After a
warm-up on the first 65536 frames (code objects) and one untimed pass at the full
shape (its allocations), `repeats` times:
JointCounts.add(X, Y) and mutual_information(), each with
  * the milliseconds between device events around the upload and the pack kernels,
    around the count kernel and around the information kernel (ek_mi_last_timing),
  * the wall time of the whole call (validation and conversion to bytes on the host,
    upload, kernels, synchronise).
From the best count-kernel time: its rate 2 (F n)^2 frames / t beside the int8
matrix peak (twice the dense bf16 figure), and the bytes it has to move -- the packed
codes of both sides once, the counts once per chunk of frames as atomic adds -- beside
HBM.  For scale, tests/_numpy_mi.py's float64 one-hot product on `cpu-frames` frames
on this box's CPU threads, and that time scaled to all frames (an extrapolation, marked
as one).  The device's counts of those frames are compared with it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _numpy_mi as nm  # noqa: E402
from enspara_amd import info_theory  # noqa: E402

I8_PEAK_OPS = 2 * 2.5e15        # dense, per second
HBM_PEAK = 8.0e12               # bytes per second (spec); about 6.3e12 achievable


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--states", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=16384)
    a = ap.parse_args()
    T, F, n = a.frames, a.features, a.states
    rng = np.random.RandomState(0)
    X = rng.randint(0, n, size=(T, F), dtype=np.int8)
    Y = rng.randint(0, n, size=(T, F), dtype=np.int8)
    Y[:, F - 1] = X[:, 0]

    res = {"frames": T, "features": F, "states": n,
           "threads": os.environ.get("OMP_NUM_THREADS"), "runs": []}
    with info_theory.JointCounts(F, F, n, n) as d:
        w = min(T, 65536)
        d.add(X[:w], Y[:w])
        d.mutual_information()
    cpu_T = min(T, a.cpu_frames)
    with info_theory.JointCounts(F, F, n, n) as d:
        small = d.add(X[:cpu_T], Y[:cpu_T]).counts()
    with info_theory.JointCounts(F, F, n, n) as d:
        d.add(X, Y)             # the timed shape once, untimed: its allocations
        d.mutual_information()
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            d.add(X, Y)
            t1 = time.perf_counter()
            mi = d.mutual_information()
            t2 = time.perf_counter()
            ms = d.last_timing()
            res["runs"].append({"upload_pack_ms": round(float(ms[0]), 3),
                                "count_ms": round(float(ms[1]), 3),
                                "information_ms": round(float(ms[2]), 3),
                                "add_wall_s": round(t1 - t0, 4),
                                "information_wall_s": round(t2 - t1, 4)})
        assert d.n_observations == (a.repeats + 1) * T and np.all(np.isfinite(mi))
    best = min(r["count_ms"] for r in res["runs"]) * 1e-3
    ops = 2.0 * (F * n) ** 2 * T
    tpad = (T + 63) // 64 * 64
    chunks = -(-tpad // info_theory.MI_CHUNK)
    code_bytes = 2.0 * F * tpad
    atomic_bytes = 4.0 * (F * n) ** 2 * chunks
    res["count_kernel"] = {
        "best_s": best, "ops": ops, "ops_per_s": ops / best,
        "i8_peak_ops_per_s": I8_PEAK_OPS, "share_of_i8_peak": ops / best / I8_PEAK_OPS,
        "code_bytes": code_bytes, "atomic_add_bytes": atomic_bytes,
        "bytes_per_s": (code_bytes + atomic_bytes) / best, "hbm_peak_bytes_per_s": HBM_PEAK,
        "least_s_by_ops": ops / I8_PEAK_OPS,
        "least_s_by_bytes": (code_bytes + atomic_bytes) / HBM_PEAK}
    up = min(r["upload_pack_ms"] for r in res["runs"]) * 1e-3
    res["upload_pack"] = {"best_s": up, "host_bytes": 2.0 * T * F,
                          "host_bytes_per_s": 2.0 * T * F / up}
    res["information_kernel_best_s"] = min(r["information_ms"] for r in res["runs"]) * 1e-3

    t0 = time.perf_counter()
    want = nm.joint_counts(X[:cpu_T], Y[:cpu_T], n, n)
    dt = time.perf_counter() - t0
    res["restatement"] = {"frames": cpu_T, "counts_s": dt,
                          "counts_s_scaled_to_all_frames_EXTRAPOLATED": dt * T / cpu_T,
                          "device_counts_equal": bool(np.array_equal(small, want))}
    print(json.dumps(res))
    if not res["restatement"]["device_counts_equal"]:
        sys.exit("the device's counts differ from the restatement's")


if __name__ == "__main__":
    main()
