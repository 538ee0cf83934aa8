#!/usr/bin/env python3
"""Time msm.bootstrap.MSMs against the per-trial loop it replaces.

    python tools/bootstrap_timing.py [--trials 128 1024] [--repeats 3] [--scale 1.0]
                                     [--out profiles/bootstrap/bootstrap_timing.json]

One JSON line, also written to --out.  Data: assignments from synthetic_data on a
metastable 1000-state matrix (20 basins of 50 states: 0.90 to stay, 0.0225 to each of the
four nearest states of the basin's ring, 0.01 to the same place in the next basin), 1000
trajectories x 1000 frames (--scale shrinks the trajectory count), lag 1.  Per trial
count, after a check of the first 3 trials against the loop and one untimed call:
`repeats` calls of MSMs(..., 'transpose') over fixed draws, wall time and the kernel
milliseconds between device events (squeeze and cells, scatter, batched build); and the
baseline, `MSM.from_assignments(assigns[idx], ...)` trial by trial over the same draws,
which uses only entry points this module leaves untouched.  Of the scatter also the
atomic wave-instructions it issues (counted here on the host from the frames: one per
run of equal cells inside a chunk of 256 positions and a trajectory, per block of 64
trials) as bytes over its time -- 256 bytes per instruction as issued, and the bytes of
the lanes that really add (a trial that never drew the trajectory adds nothing) -- next
to the ~1.3 TB/s the programming guide gives for FLOAT atomic adds of that shape; the
integer rate has not been measured by anyone, this is a record of it on this access
pattern, not a comparison with a known peak."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from enspara_amd.msm import MSM, synthetic_data  # noqa: E402
from enspara_amd.msm import bootstrap as bs  # noqa: E402

FLOAT_ATOMIC_RATE = 1.3e12      # bytes / s, float adds (guide); integer adds: unmeasured
N_STATES, BASIN, CHUNK = 1000, 50, 256


def matrix():
    T = np.zeros((N_STATES, N_STATES))
    for i in range(N_STATES):
        b0, k = i // BASIN * BASIN, i % BASIN
        T[i, i] = 0.90
        for d in (-2, -1, 1, 2):
            T[i, b0 + (k + d) % BASIN] = 0.0225
        T[i, (i + BASIN) % N_STATES] = 0.01
    return T


def scatter_atomics(assigns, idx, n_trials):
    """(wave instructions, bytes as issued, bytes of the lanes that add) of the scatter"""
    n_trj, n_frames = assigns.shape
    cell = assigns[:, :-1].astype(np.int64) * N_STATES + assigns[:, 1:]
    cell = np.concatenate([cell, np.full((n_trj, 1), -1, dtype=np.int64)], axis=1).ravel()
    p = np.arange(cell.size)
    start = np.ones(cell.size, dtype=bool)
    start[1:] = cell[1:] != cell[:-1]
    start |= (p % CHUNK == 0) | (p % n_frames == 0)
    runs = start & (cell >= 0)
    runs_per_trj = runs.reshape(n_trj, n_frames).sum(axis=1)
    blocks = (n_trials + 63) // 64
    drawn = np.zeros((n_trj, n_trials), dtype=bool)
    drawn[idx.ravel(), np.repeat(np.arange(n_trials), idx.shape[1])] = True
    n_instr = int(runs_per_trj.sum()) * blocks
    return n_instr, 256 * n_instr, int(4 * (runs_per_trj * drawn.sum(axis=1)).sum())


def measure(assigns, n_trials, a):
    idx = bs.resample_indices(len(assigns), n_trials, random_state=7)
    kw = dict(lag_time=1, method="transpose", max_n_states=N_STATES)
    # the check: the first 3 trials equal the loop's
    got = bs.MSMs(assigns, 1, "transpose", indices=idx[:3], max_n_states=N_STATES)
    for r in range(3):
        assert got[r] == MSM.from_assignments(assigns[idx[r]], **kw), r
    bs.MSMs(assigns, 1, "transpose", indices=idx, max_n_states=N_STATES)     # untimed
    out = {"trials": n_trials, "trajectories": int(assigns.shape[0]),
           "frames": int(assigns.shape[1]), "runs": []}
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        bs.MSMs(assigns, 1, "transpose", indices=idx, max_n_states=N_STATES)
        wall = time.perf_counter() - t0
        ms = bs.last_timing()
        out["runs"].append({"wall_ms": 1e3 * wall, "squeeze_cells_ms": ms[0],
                            "scatter_ms": ms[1], "build_ms": ms[2]})
    # where the one-pass call spends its wall time: table, build, host conversion
    t0 = time.perf_counter()
    with bs.bootstrap_counts(assigns, 1, indices=idx, max_n_states=N_STATES) as bc:
        t1 = time.perf_counter()
        b = bc.build("transpose")
        t2 = time.perf_counter()
        out["pattern_cells"] = int(bc.nnz)
        out["symmetrised_cells"] = int(len(b.rows))
        out["table_bytes"] = int(bc.nnz) * ((n_trials + 63) // 64 * 64) * 4
    out["open_wall_ms"] = 1e3 * (t1 - t0)
    out["build_wall_ms"] = 1e3 * (t2 - t1)
    loop_trials = n_trials if a.max_loop_trials is None else min(n_trials, a.max_loop_trials)
    MSM.from_assignments(assigns[idx[0]], **kw)                               # untimed
    t0 = time.perf_counter()
    for r in range(loop_trials):
        MSM.from_assignments(assigns[idx[r]], **kw)
    loop = time.perf_counter() - t0
    out["loop_trials_timed"] = loop_trials
    out["loop_wall_ms"] = 1e3 * loop * n_trials / loop_trials
    best = min(out["runs"], key=lambda r: r["wall_ms"])
    out["best_wall_ms"] = best["wall_ms"]
    out["loop_over_one_pass"] = out["loop_wall_ms"] / best["wall_ms"]
    out["host_conversion_ms"] = best["wall_ms"] - out["open_wall_ms"] - out["build_wall_ms"]
    n_instr, issued, active = scatter_atomics(assigns, idx, n_trials)
    scatter = min(r["scatter_ms"] for r in out["runs"])
    out["best_scatter_ms"] = scatter
    out["atomic_wave_instructions"] = n_instr
    out["atomic_bytes_issued_per_s"] = issued / (1e-3 * scatter)
    out["atomic_bytes_added_per_s"] = active / (1e-3 * scatter)
    out["float_atomic_rate_of_the_guide"] = FLOAT_ATOMIC_RATE
    out["integer_atomic_rate_known"] = False
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--max-loop-trials", type=int, default=None,
                    help="time the loop on this many trials and scale by the trial count")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap",
                                                  "bootstrap_timing.json"))
    a = ap.parse_args()
    n_trj = max(8, int(1000 * a.scale))
    starts = np.random.RandomState(3).randint(0, N_STATES, size=n_trj)
    assigns = synthetic_data.synthetic_trajectories(matrix(), starts, 1000, random_state=11)
    res = {"%d_trials" % n: measure(assigns, n, a) for n in a.trials}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
