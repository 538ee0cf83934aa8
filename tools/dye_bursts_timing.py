#!/usr/bin/env python3
"""Time the explicit-dye burst samplers next to dyes_from_expt_dist.sample_FRET_histograms, on
the same chains, in one process.

    python tools/dye_bursts_timing.py [--states 5000] [--bursts 10000] [--burst-frames 100000]
                                      [--events 1000] [--conformations 50] [--repeats 3]
                                      [--rules histogram,lifetime,k2] [--package-root DIR]

The shapes are those of tools/kmc_timing.py's bursts: a `states`-state T, once with dense rows
and once with ~50 nonzeros a row, `bursts` bursts of 50 to 150 photons with last frames up to
`burst-frames`, uniform populations, one seed (so all three rules run the same chains).  The
histogram rule has 40 bins a state; the lifetime rule `events` photon events a state; the
kappa-squared rule `conformations` conformations a state and side.

One JSON line per (T, rule) as it finishes, then one line with all of them.  Every figure is
taken after one untimed call of the same form on 64 bursts: `repeats` calls, of each the wall
time of the whole call (it ends in a device synchronise) and the milliseconds between device
events around upload, kernels and download, summed over the call's device calls.  Rates are
burst frames over the median kernel time and over the median wall time; min and max are the
spread.

--package-root imports enspara_amd from another tree (a build of another commit) to put its
sample_FRET_histograms beside this one's; use it with --rules histogram.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def matrices(n):
    rng = np.random.RandomState(0)
    dense = rng.rand(n, n)
    dense /= dense.sum(axis=1)[:, None]
    k = min(50, n)
    cols = np.stack([rng.choice(n, size=k, replace=False) for _ in range(n)])
    vals = rng.dirichlet(np.ones(k), size=n)
    sparse = scipy.sparse.csr_matrix(
        (vals.ravel(), (np.repeat(np.arange(n), k), cols.ravel())), shape=(n, n))
    return dense, sparse


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def timed(f, warm, repeats, work, timing):
    warm()
    wall, ms = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        wall.append(1e3 * (time.perf_counter() - t0))
        ms.append(np.asarray(timing(), dtype=np.float64))
    ms = np.array(ms)
    return {"work": int(work), "wall_ms": spread(wall), "upload_ms": spread(ms[:, 0]),
            "kernel_ms": spread(ms[:, 1]), "download_ms": spread(ms[:, 2]),
            "per_s_kernel": work / (np.median(ms[:, 1]) * 1e-3),
            "per_s_wall": work / (np.median(wall) * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=5000)
    ap.add_argument("--bursts", type=int, default=10 ** 4)
    ap.add_argument("--burst-frames", type=int, default=10 ** 5)
    ap.add_argument("--events", type=int, default=1000)
    ap.add_argument("--conformations", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rules", default="histogram,lifetime,k2")
    ap.add_argument("--package-root", default=ROOT)
    a = ap.parse_args()
    sys.path[:0] = [os.path.abspath(a.package_root)]
    from enspara_amd.geometry import dyes_from_expt_dist as dyes
    from enspara_amd.msm import synthetic_data as sd
    rules = a.rules.split(",")
    if set(rules) - {"histogram"}:
        from enspara_amd.geometry import dye_lifetimes as dl
        from enspara_amd.geometry import explicit_r0_calc as r0c

    n = a.states
    rng = np.random.RandomState(2)
    lasts = rng.randint(a.burst_frames // 100 + 1, a.burst_frames + 1, size=a.bursts)
    frames = [np.sort(rng.randint(0, last + 1, size=rng.randint(50, 151))) for last in lasts]
    work = int(sum(f[-1] for f in frames))
    pops = np.full(n, 1.0 / n)
    dd = [np.stack([2.0 + 0.1 * np.arange(40), np.full(40, 1 / 40.)], axis=1)] * n
    params = (2.5e15, 0.92, 4.1)
    calls = {"histogram": lambda s, fr, keep: dyes.sample_FRET_histograms(
        s, pops, dd, fr, 5.4, random_state=1, return_trajectories=keep)}
    timings = {"histogram": dyes.last_timing}
    if "lifetime" in rules:
        table = dl.event_table([(rng.exponential(3.0, size=a.events),
                                 rng.choice([0, 2], size=a.events)) for _ in range(n)])
        calls["lifetime"] = lambda s, fr, keep: dl.sample_lifetime_bursts(
            s, pops, table, fr, random_state=1, return_trajectories=keep)
        timings["lifetime"] = dl.burst_timing
    if "k2" in rules:
        c = a.conformations
        centre = rng.randn(n, 1, 3)
        dc = np.concatenate([centre + 0.5 * rng.randn(n, c, 3), centre + 0.5 * rng.randn(n, c, 3),
                             0.3 * rng.randn(n, c, 3)], axis=2)
        centre = centre + [4.5, 0.0, 0.0]
        ac = np.concatenate([centre + 0.5 * rng.randn(n, c, 3), centre + 0.5 * rng.randn(n, c, 3),
                             0.3 * rng.randn(n, c, 3)], axis=2)
        calls["k2"] = lambda s, fr, keep: r0c.sample_k2_bursts(
            s, pops, dc, ac, fr, params, random_state=1, return_trajectories=keep)
        timings["k2"] = dl.burst_timing
    out = {"package_root": os.path.relpath(os.path.abspath(a.package_root), ROOT),
           "states": n, "bursts": a.bursts, "photons": int(sum(len(f) for f in frames)),
           "frames": work, "events": a.events, "conformations": a.conformations}
    for tag, T in zip(("dense", "sparse"), matrices(n)):
        with sd.Sampler(T) as s:
            for rule in rules:
                for keep in (False, True):
                    key = "%s_%s_%s" % (tag, rule, "trajectories" if keep else "photons_only")
                    out[key] = timed(lambda: calls[rule](s, frames, keep),
                                     lambda: calls[rule](s, frames[:64], keep), a.repeats, work,
                                     timings[rule])
                    print(json.dumps({key: out[key]}), flush=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
