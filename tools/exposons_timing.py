#!/usr/bin/env python3
"""Time the two device stages of exposons at one shape each, from host arrays.

    python tools/exposons_timing.py [--frames 1000] [--atoms 3000] [--points 960]
                                    [--probe 0.14] [--wmi-frames 100000]
                                    [--wmi-features 300] [--wmi-states 2] [--repeats 3]

One JSON line.  Solvent accessibility: seeded uniform random atoms at protein density
(170 atoms per 1.3 nm cube), radii of H / C / N / O; after one untimed call at the full
shape, `repeats` calls of geometry.sasa.shrake_rupley, of each the milliseconds between
device events around the uploads, the count kernels and the group kernels
(ek_sasa_last_timing) and the wall time of the whole call.  Weighted mutual
information: seeded codes and weights; of each call of info_theory.weighted_mi the
milliseconds around upload and pack, the product kernel, the reduction and the
information kernel (ek_wmi_last_timing) and the wall time.  From the best product
time: its rate 2 (F S)^2 frames / t beside the float64 matrix peak, which is the share
of that peak the kernel reaches."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _numpy_sasa as ns  # noqa: E402
import _numpy_wmi as nw  # noqa: E402
from enspara_amd import info_theory  # noqa: E402
from enspara_amd.geometry import sasa  # noqa: E402

F64_MFMA_PEAK = 78.6e12         # flop/s, dense float64 matrix (MI355X data sheet)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--atoms", type=int, default=3000)
    ap.add_argument("--points", type=int, default=960)
    ap.add_argument("--probe", type=float, default=0.14)
    ap.add_argument("--wmi-frames", type=int, default=100000)
    ap.add_argument("--wmi-features", type=int, default=300)
    ap.add_argument("--wmi-states", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()

    rng = np.random.RandomState(0)
    xyz, radii = ns.blob(rng, a.frames, a.atoms)
    groups = [np.arange(g, min(g + 15, a.atoms)) for g in range(0, a.atoms, 15)]
    res = {"sasa": {"frames": a.frames, "atoms": a.atoms, "points": a.points,
                    "probe": a.probe, "groups": len(groups), "runs": []}}
    sasa.shrake_rupley(xyz[:8], radii, a.probe, a.points, atom_groups=groups)
    out = sasa.shrake_rupley(xyz, radii, a.probe, a.points, atom_groups=groups)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        again = sasa.shrake_rupley(xyz, radii, a.probe, a.points, atom_groups=groups)
        wall = time.perf_counter() - t0
        ms = sasa.last_timing()
        assert np.array_equal(again, out)
        res["sasa"]["runs"].append({"upload_ms": ms[0], "count_ms": ms[1], "group_ms": ms[2],
                                    "wall_ms": 1e3 * wall})
    best = min(r["count_ms"] for r in res["sasa"]["runs"])
    res["sasa"]["best_count_ms"] = best
    res["sasa"]["atom_points_per_s"] = a.frames * a.atoms * a.points / (best * 1e-3)
    _, cnt = sasa.shrake_rupley(xyz[:1], radii, a.probe, a.points, return_counts=True)
    res["sasa"]["buried_fraction_frame0"] = float((cnt == 0).mean())

    T, F, S = a.wmi_frames, a.wmi_features, a.wmi_states
    X = nw.codes(rng, T, F, S).astype(np.uint8)
    w = rng.rand(T)
    res["wmi"] = {"frames": T, "features": F, "states": S, "runs": []}
    info_theory.weighted_mi(X[:4096], w[:4096], n_feature_states=[S] * F)
    mi = info_theory.weighted_mi(X, w, n_feature_states=[S] * F)
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        again = info_theory.weighted_mi(X, w, n_feature_states=[S] * F)
        wall = time.perf_counter() - t0
        ms = info_theory.weighted_mi_last_timing()
        assert again.tobytes() == mi.tobytes()
        res["wmi"]["runs"].append({"upload_pack_ms": ms[0], "product_ms": ms[1],
                                   "reduce_ms": ms[2], "info_ms": ms[3],
                                   "wall_ms": 1e3 * wall})
    best = min(r["product_ms"] for r in res["wmi"]["runs"])
    flops = 2.0 * (F * S) ** 2 * T
    res["wmi"]["best_product_ms"] = best
    res["wmi"]["product_flops_per_s"] = flops / (best * 1e-3)
    res["wmi"]["f64_mfma_peak_flops_per_s"] = F64_MFMA_PEAK
    res["wmi"]["share_of_f64_mfma_peak"] = flops / (best * 1e-3) / F64_MFMA_PEAK
    print(json.dumps(res))


if __name__ == "__main__":
    main()
