#!/usr/bin/env python3
"""Time geometry.rmsf.rmsf_calc at three shapes, from host arrays.

    python tools/rmsf_timing.py [--repeats 3] [--cpu-seconds 3] [--scale 1.0]
                                [--out profiles/rmsf/rmsf_timing.json]

One JSON line, also written to --out.  Shapes: 10^6 frames of 300 atoms with all
atoms selected, 10^5 frames of 3000 atoms with every tenth atom selected, and the
small case 1000 x 175 (all atoms); seeded noisy copies of one random structure,
residues of 8 atoms, random populations.  --scale shrinks the two large frame counts.
Of each shape, after one untimed call: `repeats` calls of rmsf_calc, of each the
milliseconds between device events around the uploads, the kernels and the downloads
(ek_rmsf_last_timing) and the wall time of the whole call, validation included.  The
kernels' share of the HBM peak is the bytes the algorithm needs -- every frame read
once, 12 bytes per atom -- over the kernels' time, against the 6.29 TB/s a float4 copy
reaches on an MI355X (8 TB/s by the data sheet): a whole-path rate over the copy peak,
the fold kernel and every launch gap included.  Beside them the float64 numpy model
(tests/_numpy_rmsf.rmsf_reference) on the first frames on this host's CPU -- as many as
finish in about `cpu-seconds` -- scaled by frames."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _numpy_rmsf as nr  # noqa: E402
from enspara_amd.geometry import rmsf  # noqa: E402

HBM_COPY_PEAK = 6.29e12     # bytes / s, measured float4 copy
HBM_SPEC_PEAK = 8.0e12


def frames_of(n, atoms, seed, block=20000):
    rng = np.random.default_rng(seed)
    base = rng.normal(scale=1.5, size=(atoms, 3)).astype(np.float32)
    out = np.empty((n, atoms, 3), dtype=np.float32)
    for f0 in range(0, n, block):
        f1 = min(n, f0 + block)
        out[f0:f1] = base[None] + rng.normal(scale=0.1, size=(f1 - f0, atoms, 3)).astype(np.float32)
    return out


def measure(name, n, atoms, stride, a):
    x = frames_of(n, atoms, 7)
    sel = None if stride == 1 else np.arange(0, atoms, stride)
    res = np.arange(atoms) // 8
    w = np.random.default_rng(11).random(n)
    w /= w.sum()
    rmsf.rmsf_calc(x[:64], w[:64], 0, True, sel, res)
    first = rmsf.rmsf_calc(x, w, 0, True, sel, res)
    out = {"shape": name, "frames": n, "atoms": atoms,
           "selected": atoms if sel is None else len(sel), "runs": []}
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        again = rmsf.rmsf_calc(x, w, 0, True, sel, res)
        wall = time.perf_counter() - t0
        ms = rmsf.last_timing()
        assert again.tobytes() == first.tobytes()
        out["runs"].append({"upload_ms": ms[0], "kernel_ms": ms[1], "download_ms": ms[2],
                            "wall_ms": 1e3 * wall})
    best = min(r["kernel_ms"] for r in out["runs"])
    need = 12.0 * n * atoms
    out["best_kernel_ms"] = best
    out["best_wall_ms"] = min(r["wall_ms"] for r in out["runs"])
    out["needed_bytes"] = need
    out["kernel_bytes_per_s"] = need / (1e-3 * best)
    out["share_of_copy_peak"] = need / (1e-3 * best) / HBM_COPY_PEAK
    out["share_of_spec_peak"] = need / (1e-3 * best) / HBM_SPEC_PEAK
    # the numpy model on this host: double the frames until a call takes a while
    m, cpu = 16, 0.0
    while True:
        m = min(m, n)
        t0 = time.perf_counter()
        want = nr.rmsf_reference(x[:m], w[:m], 0, sel, nr.groups_of(res))
        cpu = time.perf_counter() - t0
        if m == n or cpu > a.cpu_seconds / 3:
            break
        m *= 4
    got = rmsf.rmsf_calc(x[:m], w[:m], 0, True, sel, res)
    out["model_frames"] = m
    out["model_ms"] = 1e3 * cpu
    out["model_ms_scaled_to_all_frames"] = 1e3 * cpu * n / m
    out["worst_relative_difference_from_model"] = float(np.max(np.abs(got - want) / want))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-seconds", type=float, default=3.0)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rmsf", "rmsf_timing.json"))
    a = ap.parse_args()
    res = {"small_1000x175": measure("1000 x 175, all atoms", 1000, 175, 1, a),
           "1e6x300": measure("10^6 x 300, all atoms", max(64, int(1e6 * a.scale)), 300, 1, a),
           "1e5x3000": measure("10^5 x 3000, every tenth atom", max(64, int(1e5 * a.scale)),
                               3000, 10, a)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
