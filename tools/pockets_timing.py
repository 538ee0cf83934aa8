#!/usr/bin/env python3
"""Time pocket detection at two shapes, from host arrays.

    python tools/pockets_timing.py [--frames 1000] [--atoms 3000] [--spacing 0.1]
                                   [--probe 0.14] [--min-rank 5] [--repeats 3]
                                   [--cpu-frames 4]

One JSON line.  Shapes: the beta-peptide frames of tests/golden/exposons_golden.npz (106
frames of 175 atoms, radii by element), and seeded uniform random atoms at protein density
(170 atoms per 1.3 nm cube, radii of H / C / N / O).  Of each shape, after one untimed
call: `repeats` calls of geometry.pockets.get_pockets, of each the milliseconds between
device events around the uploads, the touch kernels, the line-extent and rank kernels, the
label and compaction kernels (ek_pockets_last_timing) and the wall time of the whole call,
which includes the host's grid dimensions before and the pocket ordering after.  Beside
them the wall time of the numpy restatement (tests/_numpy_pockets.py) on the first
`cpu-frames` frames on this host's CPU, one thread, whose results the device's must equal."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _numpy_pockets as npk  # noqa: E402
import _numpy_sasa as ns  # noqa: E402
from enspara_amd.geometry import pockets  # noqa: E402


def measure(xyz, radii, a):
    args = (a.spacing, a.probe, a.min_rank)
    pockets.get_pockets(xyz[:2], radii, *args)
    out = pockets.get_pockets(xyz, radii, *args)
    res = {"frames": int(xyz.shape[0]), "atoms": int(xyz.shape[1]), "spacing": a.spacing,
           "probe": a.probe, "min_rank": a.min_rank,
           "cells_per_frame": float(np.mean([np.prod(r.shape) for r in out])),
           "pocket_cells_per_frame": float(np.mean([len(r.cells) for r in out])),
           "runs": []}
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        again = pockets.get_pockets(xyz, radii, *args)
        wall = time.perf_counter() - t0
        ms = pockets.last_timing()
        assert all(x.cells.tobytes() == y.cells.tobytes() and
                   x.pocket_ids.tobytes() == y.pocket_ids.tobytes() for x, y in zip(again, out))
        res["runs"].append({"upload_ms": ms[0], "touch_ms": ms[1], "rank_ms": ms[2],
                            "label_compact_ms": ms[3], "wall_ms": 1e3 * wall})
    best = min(res["runs"], key=lambda r: r["wall_ms"])
    res["best_wall_ms"] = best["wall_ms"]
    res["best_device_ms"] = min(r["upload_ms"] + r["touch_ms"] + r["rank_ms"] +
                                r["label_compact_ms"] for r in res["runs"])
    n = min(a.cpu_frames, len(xyz))
    t0 = time.perf_counter()
    want = [npk.frame_pockets(x, radii, *args) for x in xyz[:n]]
    cpu = time.perf_counter() - t0
    for w, g in zip(want, out):
        assert np.array_equal(g.pocket_ids, w["ids"])
        assert np.array_equal(g.cells, npk.coordinates(w["cells"], w["origin"], w["dims"],
                                                       a.spacing))
    res["restatement_frames"] = n
    res["restatement_ms_per_frame"] = 1e3 * cpu / n
    res["wall_ms_per_frame"] = best["wall_ms"] / len(xyz)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--atoms", type=int, default=3000)
    ap.add_argument("--spacing", type=float, default=0.1)
    ap.add_argument("--probe", type=float, default=0.14)
    ap.add_argument("--min-rank", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-frames", type=int, default=4)
    a = ap.parse_args()

    E = np.load(os.path.join(ROOT, "tests", "golden", "exposons_golden.npz"))
    res = {"beta_peptide": measure(np.ascontiguousarray(E["bp_xyz"]),
                                   npk.radii_of(E["bp_elements"]), a)}
    xyz, radii = ns.blob(np.random.RandomState(0), a.frames, a.atoms)
    res["synthetic"] = measure(xyz, radii.astype(np.float64), a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
