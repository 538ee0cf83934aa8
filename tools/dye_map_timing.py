#!/usr/bin/env python3
"""Time explicit_r0_calc.map_dye_on_protein at two numbers of centres, from host arrays.

    python tools/dye_map_timing.py [--centres 1000] [--atoms 3001] [--confs 5000]
                                   [--dye-atoms 60] [--repeats 3] [--cpu-confs 50]

One JSON line.  The protein is seeded uniform random atoms at protein density
(tests/_numpy_sasa.blob: 170 atoms per 1.3 nm cube, radii of H / C / N / O; every centre is
another draw) with one residue of five atoms (N, CA, C, O, CB) added in a face of the cube,
its CB pointing away from it.  The dye library is tests/_numpy_dye_map.dye_library: five
backbone-like atoms and a random-walk tail from CB (steps of 0.07 nm, a slight outward
drift: about half the conformations clash, and the dye reaches 1.4 nm), every conformation
with its own rigid motion (the reference's libraries are not read here).  For 1 centre and
for `centres` centres, after one untimed call: `repeats` calls, of each the milliseconds
between device events around the upload, the fit, the cull and the touch kernels and the
download (DyeMap.timing, summed over the chunks) and the wall time of the whole call, which
includes the validation before and the ragged assembly after, on the host.  Beside them the
mean length of the culled atom lists, the share of the (centre, conformation, dye atom)
lanes that leave the touch loop early (1 - the sum of the counts over their number), and
the wall time of the numpy model (float64 Kabsch fit and the brute-force touch test of
tests/_numpy_dye_map.py) on one centre with the library thinned to `cpu-confs`
conformations, on this host's CPU, scaled per conformation."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _numpy_dye_map as dm  # noqa: E402
import _numpy_sasa as ns  # noqa: E402
from enspara_amd.geometry import explicit_r0_calc as r0c  # noqa: E402

PROBE, TOL = 0.04, 6


def system(centres, atoms, confs, dye_atoms):
    rng = np.random.RandomState(0)
    xyz, radii = ns.blob(rng, centres, atoms)
    side = float(xyz.max())
    u, v, w = np.eye(3)
    ca = np.full(3, side / 2) + (side / 2) * u
    res = np.array([ca - 0.08 * u + 0.12 * v, ca, ca - 0.08 * u - 0.12 * v,
                    ca - 0.20 * u - 0.16 * v, ca + 0.10 * u + 0.10 * w])    # N, CA, C, O, CB
    extra = np.broadcast_to(res.astype(np.float32), (centres, 5, 3))
    xyz = np.ascontiguousarray(np.concatenate([xyz, extra], axis=1))
    radii = np.concatenate([radii.astype(np.float64), [0.155, 0.17, 0.17, 0.152, 0.17]])
    names = ("N", "CA", "CB", "C", "O")
    template = res[[0, 1, 4, 2, 3]] - res[1]
    dye = dm.dye_library(rng, confs, dye_atoms, template, 2, step=0.07, drift=0.15)
    own = atoms + np.arange(5, dtype=np.int32)
    return dict(xyz=xyz, radii=radii, dye_xyz=dye, prot_sel=own[[0, 1, 4, 2, 3]],
                dye_sel=np.arange(len(names), dtype=np.int32), exclude_atoms=own,
                r_atom=dye_atoms - 1, mu_atoms=(dye_atoms - 6, dye_atoms - 3))


def measure(case, repeats):
    one = dict(case, xyz=case["xyz"][:1])
    r0c.map_dye_on_protein(probe_radius=PROBE, atom_tol=TOL, **one)
    out = r0c.map_dye_on_protein(probe_radius=PROBE, atom_tol=TOL, **case)
    P, atoms = case["xyz"].shape[:2]
    D, A = case["dye_xyz"].shape[:2]
    res = {"centres": int(P), "atoms": int(atoms), "confs": int(D), "dye_atoms": int(A),
           "distance_tests_uncut": float(P) * D * A * (atoms - 5),
           "culled_list_mean": float(out.list_len.mean()),
           "culled_list_max": int(out.list_len.max()),
           "kept_mean": float(np.mean([len(k) for k in out.kept])),
           "lanes_leaving_early": 1.0 - float(out.counts.sum(dtype=np.int64)) / (float(P) * D * A),
           "runs": []}
    for _ in range(repeats):
        t0 = time.perf_counter()
        again = r0c.map_dye_on_protein(probe_radius=PROBE, atom_tol=TOL, **case)
        wall = time.perf_counter() - t0
        assert np.array_equal(again.counts, out.counts)
        ms = again.timing
        res["runs"].append({"upload_ms": ms[0], "fit_ms": ms[1], "cull_ms": ms[2],
                            "touch_ms": ms[3], "download_ms": ms[4], "wall_ms": 1e3 * wall})
    for k in ("upload_ms", "fit_ms", "cull_ms", "touch_ms", "download_ms", "wall_ms"):
        res["best_" + k] = min(r[k] for r in res["runs"])
    return res, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--atoms", type=int, default=3001)
    ap.add_argument("--confs", type=int, default=5000)
    ap.add_argument("--dye-atoms", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-confs", type=int, default=50)
    a = ap.parse_args()

    case = system(a.centres, a.atoms, a.confs, a.dye_atoms)
    res = {}
    res["one_centre"], one = measure(dict(case, xyz=case["xyz"][:1]), a.repeats)
    res["all_centres"], _ = measure(case, a.repeats)

    step = max(1, a.confs // a.cpu_confs)
    thin = np.ascontiguousarray(case["dye_xyz"][::step])
    cutoff = case["radii"] + PROBE
    t0 = time.perf_counter()
    m = dm.model_align(thin, case["xyz"][0], case["prot_sel"], case["dye_sel"])
    t1 = time.perf_counter()
    counts = dm.touch_counts(m["aligned"].astype(np.float32), case["xyz"][0], cutoff,
                             case["exclude_atoms"])
    t2 = time.perf_counter()
    agree = int((counts == one.counts[0][::step]).sum())
    res["model"] = {"confs": int(len(thin)), "fit_ms": 1e3 * (t1 - t0), "touch_ms": 1e3 * (t2 - t1),
                    "counts_equal_to_the_device": agree,
                    "s_per_conformation": (t2 - t0) / len(thin),
                    "extrapolated_s_all_centres": (t2 - t0) / len(thin) * a.confs * a.centres}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
