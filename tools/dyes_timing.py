#!/usr/bin/env python3
"""Time smFRET dye labelling at two frame counts, from host arrays.

    python tools/dyes_timing.py [--frames 1000] [--atoms 3000] [--points 20000]
                                [--repeats 3] [--cpu-points 2000]

One JSON line.  The protein is seeded uniform random atoms at protein density (170 atoms
per 1.3 nm cube, radii of H / C / N / O) with two three-atom backbones added on opposite
faces of the cube, their CB pointing away from it; every frame is another draw.  The two
clouds are `points` points uniform in a ball of 1.5 nm whose centre lies 1.2 nm along the
CB direction (the reference's cloud files have 20 000 points each and are not read here).
For 1 frame and for `frames` frames, after one untimed call: `repeats` calls of
geometry.dyes_from_expt_dist.dye_distance_distribution, of each the milliseconds between
device events around the uploads, the touch and compaction kernels, the histogram kernels
(maxima, plan, counts) and the download (ek_dyes_last_timing), and the wall time of the whole
call, which includes the rotation matrices before and the normalisation after, on the
host.  pairs_per_s = kept pairs of all frames / the histogram kernels' time.  Beside them
the wall time of the numpy model (tests/_numpy_dyes.py) on one frame with clouds thinned to
`cpu-points` points, on this host's CPU, one thread, scaled per pair."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _numpy_dyes as nd  # noqa: E402
import _numpy_sasa as ns  # noqa: E402
from enspara_amd.geometry import dyes_from_expt_dist as dyes  # noqa: E402


def system(frames, atoms, points):
    rng = np.random.RandomState(0)
    xyz, radii = ns.blob(rng, frames, atoms)
    side = float(xyz.max())
    extra = np.empty((frames, 6, 3), dtype=np.float32)
    for r, u in enumerate((np.array([1.0, 0, 0]), np.array([-1.0, 0, 0]))):
        v = np.array([0, 1.0, 0])
        ca = np.full(3, side / 2) + (side / 2 + 0.25) * u
        extra[:, 3 * r + 0] = ca - 0.08 * u + 0.12 * v       # N
        extra[:, 3 * r + 1] = ca                             # CA
        extra[:, 3 * r + 2] = ca - 0.08 * u - 0.12 * v       # C
    xyz = np.ascontiguousarray(np.concatenate([xyz, extra], axis=1))
    radii = np.concatenate([radii.astype(np.float64), [0.155, 0.17, 0.17] * 2])
    bbs = np.array([[atoms, atoms + 1, atoms + 2], [atoms + 3, atoms + 4, atoms + 5]])
    d1 = nd.ball(rng, points, 1.5, centre=(0, 0, 1.2))
    d2 = nd.ball(rng, points, 1.5, centre=(0, 0, 1.2))
    return xyz, radii, d1, d2, bbs


def measure(xyz, radii, d1, d2, bbs, repeats):
    dyes.dye_distance_distribution(xyz[:1], radii, d1, d2, bbs)
    out = dyes.dye_distance_distribution(xyz, radii, d1, d2, bbs)
    # kept pairs, from the model's touch test on frame 0 (every frame has the same backbones)
    kept = []
    for d in (d1, d2):
        for bb in bbs:
            M, t = nd.rot_mat(xyz[0], bb)
            kept.append(int(nd.keep_mask(nd.align(d, M, t), xyz[0], radii + 0.2).sum()))
    pairs0 = kept[0] * kept[3] + kept[1] * kept[2]
    res = {"frames": int(xyz.shape[0]), "atoms": int(xyz.shape[1]), "points": int(len(d1)),
           "kept_frame0": kept, "pairs_frame0": pairs0, "bins_frame0": int(len(out[0][0])),
           "runs": []}
    for _ in range(repeats):
        t0 = time.perf_counter()
        again = dyes.dye_distance_distribution(xyz, radii, d1, d2, bbs)
        wall = time.perf_counter() - t0
        ms = dyes.last_labelling_timing()
        assert all(np.array_equal(x, y) for x, y in zip(again[0], out[0]))
        res["runs"].append({"upload_ms": ms[0], "touch_ms": ms[1], "hist_ms": ms[2],
                            "download_ms": ms[3], "wall_ms": 1e3 * wall})
    best = min(res["runs"], key=lambda r: r["hist_ms"])
    res["best_wall_ms"] = min(r["wall_ms"] for r in res["runs"])
    res["best_touch_ms"] = min(r["touch_ms"] for r in res["runs"])
    res["best_hist_ms"] = best["hist_ms"]
    # (frames differ in their atoms, not in their backbones: frame 0's pairs stand for all)
    res["pairs_per_s_about"] = pairs0 * len(xyz) / (1e-3 * best["hist_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--atoms", type=int, default=3000)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-points", type=int, default=2000)
    a = ap.parse_args()

    xyz, radii, d1, d2, bbs = system(a.frames, a.atoms, a.points)
    res = {"one_frame": measure(xyz[:1], radii, d1, d2, bbs, a.repeats),
           "trajectory": measure(xyz, radii, d1, d2, bbs, a.repeats)}
    step = max(1, a.points // a.cpu_points)
    t0 = time.perf_counter()
    probs, edges, kept, counts = nd.frame_distribution(xyz[0], radii + 0.2, d1[::step], d2[::step],
                                                       bbs, 0.1)
    cpu = time.perf_counter() - t0
    got = dyes.dye_distance_distribution(xyz[:1], radii, np.ascontiguousarray(d1[::step]),
                                         np.ascontiguousarray(d2[::step]), bbs)
    assert np.array_equal(got[0][0], probs) and np.array_equal(got[1][0], edges)
    pairs = int(sum(c.sum() for c in counts))
    res["model"] = {"points": int(len(d1[::step])), "pairs": pairs, "wall_ms": 1e3 * cpu,
                    "pairs_per_s": pairs / cpu}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
