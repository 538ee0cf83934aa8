#!/usr/bin/env python3
"""Time info_theory.entropy at two shapes, from host arrays.

    python tools/entropy_timing.py [--states 5000] [--frames 10000000] [--sc-frames 1000000]
                                   [--sc-features 1000] [--repeats 3] [--skip-cpu]

One JSON line.  Two shapes only:

1. relative_entropy_msm of two dense `states` x `states` matrices (seeded random rows),
   populations given (uniform: the eigenvector is not what is timed), with Q given and
   with assignments= of `frames` frames (10 trajectories of independent uniform states).
   Of each, after one untimed call: `repeats` calls, of each the milliseconds between
   device events around the uploads, the building of Q and the KL kernel
   (entropy.last_timing) and the wall time of the whole call.  kernel_TBps = 2 n^2 8 bytes
   over the KL kernel's time.  Beside them the wall time of the numpy restatement
   (tests/_numpy_entropy.py) on this host for the same answers, which the device's must
   match within the tests' bound.  js_kernel_ms and shannon_kernel_ms: the same row walk
   with twice the divisions and logarithms on the same bytes, and with one logarithm and
   no division on half the bytes, to tell what bounds the KL kernel.
2. state_counts of `sc-frames` x `sc-features` codes of 3 states: device-event times of the
   upload and of the kernel (StateCounts.last_timing), the wall time of the call, and
   kernel_TBps = frames x features bytes over the kernel's time.  Beside it the only other
   route to these counts: joint_counts(X, X) and its diagonal, wall time and its count
   kernel's device time (JointCounts.last_timing), equal counts."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _numpy_entropy as ne  # noqa: E402
from enspara_amd.info_theory import entropy, mutual_info  # noqa: E402


def timed(f, repeats, timing):
    f()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = f()
        wall = 1e3 * (time.perf_counter() - t0)
        runs.append(dict(zip(("upload_ms", "build_ms", "kernel_ms"),
                             [float(x) for x in timing()]), wall_ms=wall))
    return out, runs


def relative_entropy(a):
    n = a.states
    rng = np.random.RandomState(0)
    P, Q = ne.random_rows(rng, n, n), ne.random_rows(rng, n, n)
    A = rng.randint(0, n, size=(10, a.frames // 10)).astype(np.int32)
    pops = np.full(n, 1.0 / n)
    res = {"states": n, "frames": int(A.size)}
    for tag, kw in (("Q_given", {"Q": Q}), ("assignments", {"assignments": A})):
        got, runs = timed(lambda: entropy.relative_entropy_msm(P, populations=pops, **kw),
                          a.repeats, entropy.last_timing)
        best = min(r["kernel_ms"] for r in runs)
        r = {"runs": runs, "value_bits": float(got), "best_kernel_ms": best,
             "best_wall_ms": min(r["wall_ms"] for r in runs),
             "kernel_TBps": 2.0 * n * n * 8 / (best * 1e-3) / 1e12}
        if not a.skip_cpu:
            t0 = time.perf_counter()
            Qn = Q if tag == "Q_given" else ne.Q_from_assignments(A, n_states=n)
            per, S = ne.kl_divergence(P, Qn)
            want = np.sum(per * pops)
            r["numpy_wall_ms"] = 1e3 * (time.perf_counter() - t0)
            r["numpy_value_bits"] = float(want)
            bound = np.sum(ne.kl_bound(n, S) * pops) + n * ne.U * np.sum(np.abs(per) * pops)
            r["abs_diff_over_bound"] = float(abs(got - want) / bound)
            assert abs(got - want) <= bound
        res[tag] = r
    # what bounds the KL kernel: the same walk over the same 2 n^2 8 bytes with two
    # divisions and two logarithms per element (JS), and over half the bytes with one
    # logarithm and no division (Shannon, not normalised)
    for tag, f in (("js", lambda: entropy.js_divergence(P, Q)),
                   ("shannon", lambda: entropy.shannon_entropy_rows(P, normalize=False))):
        _, runs = timed(f, a.repeats, entropy.last_timing)
        res[tag + "_kernel_ms"] = min(r["kernel_ms"] for r in runs)
    return res


def counts(a):
    T, F = a.sc_frames, a.sc_features
    X = np.random.RandomState(1).randint(0, 3, size=(T, F), dtype=np.uint8)
    res = {"frames": T, "features": F, "n_states": 3, "runs": []}
    with entropy.StateCounts(F, 3) as sc:
        sc.add(X[:1000])
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            got = entropy.state_counts(X, 3)
            wall = 1e3 * (time.perf_counter() - t0)
            sc.add(X)
            up, k = (float(x) for x in sc.last_timing())
            res["runs"].append({"upload_ms": up, "kernel_ms": k, "wall_ms": wall})
    best = min(r["kernel_ms"] for r in res["runs"])
    res["best_kernel_ms"] = best
    res["best_wall_ms"] = min(r["wall_ms"] for r in res["runs"])
    res["kernel_TBps"] = float(T) * F / (best * 1e-3) / 1e12
    with mutual_info.JointCounts(F, F, 3, 3) as jc:
        jc.add(X[:1000])
        t0 = time.perf_counter()
        jc.add(X)
        full = jc.counts()
        res["joint_counts_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        res["joint_counts_kernel_ms"] = float(jc.last_timing()[1])
    diag = full[np.arange(F), np.arange(F)].sum(axis=-1).astype(np.int64)
    assert np.array_equal(diag, got + ne.state_counts([X[:1000]], 3))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=5000)
    ap.add_argument("--frames", type=int, default=10 ** 7)
    ap.add_argument("--sc-frames", type=int, default=10 ** 6)
    ap.add_argument("--sc-features", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-cpu", action="store_true")
    a = ap.parse_args()
    print(json.dumps({"relative_entropy_msm": relative_entropy(a), "state_counts": counts(a)}))


if __name__ == "__main__":
    main()
