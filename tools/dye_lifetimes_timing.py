#!/usr/bin/env python3
"""Time geometry.dye_lifetimes at the shapes a labelling run has.

    python tools/dye_lifetimes_timing.py [--states 500] [--nnz 20] [--samples 1000]
                                         [--centres 1000] [--means 100,2000]
                                         [--caps 32,64,128,256,1024,0] [--repeats 3]
                                         [--host-seconds 20] [--only one,many,host]
                                         [--out FILE]

One JSON line per part as it finishes, then one line with all of them (also written to
``--out``).  Every device figure is taken after one untimed call of the same form (code
objects load on the first launch): ``repeats`` calls, of each the wall time of the whole
call (it ends in a device synchronise) and the milliseconds between device events around
the kernels (dye_lifetimes.last_timing).  Rates are excitation steps over the median kernel
time and over the median wall time; min and max are the spread.

Both dye MSMs have ``states`` states with ``nnz`` nonzeros a row; the dyes are 9 nm apart, so
an excitation lasts Td / lag steps on average: the lag times are Td / mean for every mean
asked for.  Every centre holds the same problem (the device stores a copy per centre, as it
would for different ones).

  one    one centre x ``samples`` excitations
  many   ``centres`` centres x ``samples`` excitations in one handle
         both for every mean and every step cap; cap 0 stands for step_cap = max_steps: one
         launch, no compaction
  host   the reference-shaped loop (per step calc_k2_r, calc_R0, FRET_rate,
         calc_energy_transfer_prob and three rng.choice) on this machine's CPU for
         ``host-seconds``: steps per second
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from enspara_amd.geometry import dye_lifetimes as dl  # noqa: E402
from enspara_amd.geometry import explicit_r0_calc as r0c  # noqa: E402

PARAMS = (2.5e15, 0.92, 4.1)
MAX_STEPS = 1 << 20


def msm(rng, n, nnz):
    T = np.zeros((n, n))
    for i in range(n):
        cols = rng.choice(n, size=min(nnz, n), replace=False)
        T[i, cols] = rng.dirichlet(np.ones(len(cols)))
    return T / T.sum(axis=1)[:, None], rng.dirichlet(np.ones(n))


def coords(rng, n, centre):
    c = np.asarray(centre, dtype=np.float64) + 0.8 * rng.randn(n, 3)
    return np.hstack([c, c + 0.1 * rng.randn(n, 3), 0.3 * rng.randn(n, 3)])


def inputs(a):
    rng = np.random.RandomState(0)
    dT, de = msm(rng, a.states, a.nnz)
    aT, ae = msm(rng, a.states, a.nnz)
    return coords(rng, a.states, (0, 0, 0)), dT, de, coords(rng, a.states, (9, 0, 0)), aT, ae


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def timed(pair, n, cap, repeats):
    kw = dict(random_state=1, step_cap=cap or MAX_STEPS, max_steps=MAX_STEPS)
    steps, _ = pair.resolve(n, **kw)                # untimed
    work = int(steps.sum())
    wall, kernel = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        pair.resolve(n, **kw)
        wall.append(1e3 * (time.perf_counter() - t0))
        kernel.append(float(dl.last_timing()[1]))
    return {"work": work, "mean_steps": work / steps.size, "longest": int(steps.max()),
            "wall_ms": spread(wall), "kernel_ms": spread(kernel),
            "steps_per_s_kernel": work / (np.median(kernel) * 1e-3),
            "steps_per_s_wall": work / (np.median(wall) * 1e-3)}


def emit(name, res):
    print(json.dumps({name: res}), flush=True)
    return res


def device(a, q, centres, name):
    res = {"centres": centres, "samples": a.samples}
    for mean in a.means:
        p = dl.problem(q[0], q[1], q[2], q[3], q[4], q[5], PARAMS, PARAMS[2] / mean)
        with dl.DyePair([p] * centres) as pair:
            for cap in a.caps:
                res["mean%d_cap%d" % (mean, cap)] = timed(pair, a.samples, cap, a.repeats)
    return emit(name, res)


def host(a, q):
    """the reference's loop, on the arrays the device gets"""
    dc, dT, de, ac, aT, ae = q
    J, Qd, Td = PARAMS
    krad, k_non_rad = dl.calc_dye_radiative_rates(Qd, Td)
    lag = Td / a.means[0]
    outcomes = np.arange(4)
    rng = np.random.default_rng(1)
    n, steps, done = len(de), 0, 0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.host_seconds:
        d, c, state = rng.choice(n, p=de), rng.choice(n, p=ae), 3
        while state == 3:
            k2, r = r0c.calc_k2_r(dc[d], ac[c])
            kRET = dl.FRET_rate(r, r0c.calc_R0(k2, Qd, J), Td)
            state = rng.choice(outcomes, p=dl.calc_energy_transfer_prob(krad, k_non_rad, kRET, lag))
            d, c = rng.choice(n, p=dT[d, :]), rng.choice(n, p=aT[c, :])
            steps += 1
        done += 1
    dt = time.perf_counter() - t0
    return emit("host", {"steps": steps, "excitations": done, "steps_per_s": steps / dt})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=500)
    ap.add_argument("--nnz", type=int, default=20)
    ap.add_argument("--samples", type=int, default=1000)
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--means", default="100,2000")
    ap.add_argument("--caps", default="32,64,128,256,1024,0")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-seconds", type=float, default=20.0)
    ap.add_argument("--only", default="one,many,host")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.means = [int(v) for v in a.means.split(",")]
    a.caps = [int(v) for v in a.caps.split(",")]
    q = inputs(a)
    out = {"states": a.states, "nnz": a.nnz}
    for name in a.only.split(","):
        if name == "one":
            out[name] = device(a, q, 1, "one")
        elif name == "many":
            out[name] = device(a, q, a.centres, "many")
        else:
            out[name] = host(a, q)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
