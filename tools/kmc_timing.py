#!/usr/bin/env python3
"""Time msm.synthetic_data and geometry.dyes_from_expt_dist at the shapes a user runs.

    python tools/kmc_timing.py [--states 5000] [--long-steps 10000000] [--chains 10000]
                               [--chain-steps 100000] [--bursts 10000] [--burst-frames 100000]
                               [--ens-steps 1000] [--repeats 3] [--host-seconds 60]
                               [--only single,many,crossover,bursts,ensemble,host]

One JSON line per part as it finishes (so a long run shows progress), then one line with
all of them.  Every device figure is taken after one untimed call of the same form at a
small size (code objects load on the first launch): `repeats` calls, of each the wall
time of the whole call (it ends in a device synchronise) and the milliseconds between
device events around upload, kernels and download (synthetic_data.last_timing).  Rates
are steps (or burst frames) over the median kernel time and over the median wall time;
min and max are the spread.

  single    one chain x `long-steps` on a `states`-state T, dense rows and ~50 nonzeros a
            row, through the wave form; the lane form on a tenth of the steps beside it
  many      `chains` x `chain-steps` on both T, the form the library picks, and both forms
            at a tenth of the steps
  crossover 2048 chains (the most that take a wave each when the library picks) x a tenth
            of `chain-steps`, both forms
  bursts    `bursts` bursts of ~100 photons with last frames up to `burst-frames`, with and
            without trajectories
  ensemble  `states` x `ens-steps`, dense and sparse
  host      the reference-shaped loop (one rng.choice(n, 1, p=T[state]) per step, the
            sparse row densified first as the reference does) on this machine's CPU for
            `host-seconds` each: steps per second
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from enspara_amd.geometry import dyes_from_expt_dist as dyes  # noqa: E402
from enspara_amd.msm import synthetic_data as sd  # noqa: E402


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


def timed(f, warm, repeats, work, timing=sd.last_timing):
    """work: steps of one call -> wall / kernel spreads and the rates of their medians"""
    warm()
    wall, kernel, download = [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        wall.append(1e3 * (time.perf_counter() - t0))
        ms = timing()
        kernel.append(float(ms[1]))
        download.append(float(ms[2]))
    return {"work": int(work), "wall_ms": spread(wall), "kernel_ms": spread(kernel),
            "download_ms": spread(download),
            "per_s_kernel": work / (np.median(kernel) * 1e-3),
            "per_s_wall": work / (np.median(wall) * 1e-3)}


def emit(name, res):
    print(json.dumps({name: res}), flush=True)
    return res


def single(a, mats):
    res = {}
    for tag, T in mats:
        with sd.Sampler(T) as s:
            for form, steps in (("wave", a.long_steps), ("lane", max(2, a.long_steps // 10))):
                res["%s_%s" % (tag, form)] = timed(
                    lambda: s.trajectories([0], steps, 1, form=form),
                    lambda: s.trajectories([0], 1000, 1, form=form), a.repeats, steps - 1)
    return emit("single", res)


def many(a, mats):
    res = {}
    start = np.arange(a.chains) % a.states
    for tag, T in mats:
        with sd.Sampler(T) as s:
            for form, steps in (("auto", a.chain_steps), ("lane", max(2, a.chain_steps // 10)),
                                ("wave", max(2, a.chain_steps // 10))):
                res["%s_%s" % (tag, form)] = timed(
                    lambda: s.trajectories(start, steps, 1, form=form),
                    lambda: s.trajectories(start[:64], 100, 1, form=form), a.repeats,
                    a.chains * (steps - 1))
    return emit("many", res)


def crossover(a, mats):
    """both forms at the largest number of chains that still takes a wave each"""
    res = {"chains": 2048}
    start = np.arange(2048) % a.states
    steps = max(2, a.chain_steps // 10)
    for tag, T in mats:
        with sd.Sampler(T) as s:
            for form in ("lane", "wave"):
                res["%s_%s" % (tag, form)] = timed(
                    lambda: s.trajectories(start, steps, 1, form=form),
                    lambda: s.trajectories(start[:64], 100, 1, form=form), a.repeats,
                    2048 * (steps - 1))
    return emit("crossover", res)


def bursts(a, mats):
    n = a.states
    rng = np.random.RandomState(2)
    lasts = rng.randint(a.burst_frames // 100 + 1, a.burst_frames + 1, size=a.bursts)
    frames = [np.sort(rng.randint(0, last + 1, size=rng.randint(50, 151))) for last in lasts]
    work = int(sum(f[-1] for f in frames))
    pops = np.full(n, 1.0 / n)
    dd = [np.stack([2.0 + 0.1 * np.arange(40), np.full(40, 1 / 40.)], axis=1)] * n
    res = {"bursts": a.bursts, "photons": int(sum(len(f) for f in frames))}
    for tag, T in mats:
        with sd.Sampler(T) as s:
            for keep in (False, True):
                res["%s_%s" % (tag, "trajectories" if keep else "photons_only")] = timed(
                    lambda: dyes.sample_FRET_histograms(s, pops, dd, frames, 5.4, random_state=1,
                                                        return_trajectories=keep),
                    lambda: dyes.sample_FRET_histograms(s, pops, dd, frames[:64], 5.4,
                                                        random_state=1, return_trajectories=keep),
                    a.repeats, work, dyes.last_timing)
    return emit("bursts", res)


def ensemble(a, mats):
    n = a.states
    p0 = np.full(n, 1.0 / n)
    obs = np.arange(n, dtype=np.float64)
    res = {}
    for tag, T in mats:
        for otag, o in (("all", None), ("observable", obs)):
            res["%s_%s" % (tag, otag)] = timed(
                lambda: sd.synthetic_ensemble(T, p0, a.ens_steps, o),
                lambda: sd.synthetic_ensemble(T, p0, 3, o), a.repeats, a.ens_steps - 1)
    return emit("ensemble", res)


def host(a, mats):
    res = {}
    for tag, T in mats:
        rng = np.random.default_rng(1)
        n, state, steps = T.shape[0], 0, 0
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < a.host_seconds:
            for _ in range(100):
                p = T[state, :].toarray()[0] if scipy.sparse.issparse(T) else T[state, :]
                state = int(rng.choice(n, 1, p=p)[0])
            steps += 100
        res[tag] = {"steps": steps, "steps_per_s": steps / (time.perf_counter() - t0)}
    return emit("host", res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=5000)
    ap.add_argument("--long-steps", type=int, default=10 ** 7)
    ap.add_argument("--chains", type=int, default=10 ** 4)
    ap.add_argument("--chain-steps", type=int, default=10 ** 5)
    ap.add_argument("--bursts", type=int, default=10 ** 4)
    ap.add_argument("--burst-frames", type=int, default=10 ** 5)
    ap.add_argument("--ens-steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-seconds", type=float, default=60.0)
    ap.add_argument("--only", default="single,many,crossover,bursts,ensemble,host")
    a = ap.parse_args()
    dense, sparse = matrices(a.states)
    mats = (("dense", dense), ("sparse", sparse))
    parts = {"single": single, "many": many, "crossover": crossover, "bursts": bursts,
             "ensemble": ensemble, "host": host}
    out = {"states": a.states}
    for name in a.only.split(","):
        out[name] = parts[name](a, mats)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
