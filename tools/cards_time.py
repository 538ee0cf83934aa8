#!/usr/bin/env python3
"""Time enspara_amd.cards and enspara_amd.geometry.rotamer on the device at the shape
tools/mi_time.py measures: 10^6 frames x 1000 features x 3 states, as four trajectories
of 250 000 frames.

    python tools/cards_time.py [--frames 250000] [--trajectories 4] [--features 1000]
                               [--atoms 400] [--repeats 3] [--out profiles/cards/cards_time.json]

One JSON record, printed and written to --out.  The state codes switch at a rate of 0.1
per frame (feature j from a seed of its own); the angles and coordinates are uniform
noise (the scans' work does not depend on the data).  After a warm-up on 4096 frames
(code objects), `repeats` times a whole analysis: four CardsStates.add, disorder,
matrices, each with the milliseconds between device events (ek_cards_last_timing):
  * upload + pack and the statistics kernels of each add,
  * the disorder kernels of all four trajectories,
  * the S-S, D-D and S-D count passes, the transpose that makes the D-S counts, and the
    four information kernels;
then the rotamer scan of one trajectory's angles [frames, features], the dihedral kernel
of one trajectory's coordinates [frames, atoms, 3] with `features` dihedrals, and both
fused.  For each scan the bytes it has to move over its best time, beside the HBM peak:
  stats     the packed codes once
  disorder  the packed codes once, the disorder codes once
  rotamer   the angles twice (the map pass and the emit pass), the states once
  dihedral  the coordinates once, the angles once
  fused     the coordinates twice, the states once
The statistics of a prefix are compared with tests/_numpy_cards.py."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _numpy_cards as nc  # noqa: E402
from enspara_amd.cards import disorder  # noqa: E402
from enspara_amd.geometry import rotamer  # noqa: E402

HBM_PEAK = 8.0e12               # bytes per second (spec); about 6.3e12 achievable
NAMES = ("upload_pack_ms", "stats_ms", "disorder_ms", "count_ss_ms", "count_dd_ms",
         "count_sd_ms", "transpose_ms", "information_ms")


def codes(T, F, n, seed):
    rng = np.random.default_rng(seed)
    jump = (rng.random((T, F), dtype=np.float32) < 0.1) * rng.integers(
        1, n, (T, F), dtype=np.int8)
    return (np.cumsum(jump, axis=0, dtype=np.int32) % n).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250000)
    ap.add_argument("--trajectories", type=int, default=4)
    ap.add_argument("--features", type=int, default=1000)
    ap.add_argument("--states", type=int, default=3)
    ap.add_argument("--atoms", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cards", "cards_time.json"))
    a = ap.parse_args()
    T, K, F, n = a.frames, a.trajectories, a.features, a.states
    X = codes(T, F, n, 0)
    trajs = [np.ascontiguousarray(np.roll(X, k, axis=1)) for k in range(K)]

    res = {"frames_per_trajectory": T, "trajectories": K, "features": F, "states": n,
           "scan_chunk": disorder.SCAN_CHUNK, "runs": []}
    with disorder.CardsStates(F, n) as d:       # warm-up, and the check of a prefix
        d.add(X[:4096])
        ok = bool(np.array_equal(d.stats()[0], nc.stats(X[:4096])))
        d.disorder(*disorder.disorder_interval(*d.mean_times()))
        d.matrices()
    res["prefix_stats_equal_the_restatement"] = ok
    for _ in range(a.repeats):
        run = {"adds": []}
        with disorder.CardsStates(F, n) as d:
            for t in trajs:
                d.add(t)
                ms = d.last_timing()
                run["adds"].append({NAMES[0]: round(float(ms[0]), 3),
                                    NAMES[1]: round(float(ms[1]), 3)})
            lo, hi = disorder.disorder_interval(*d.mean_times())
            d.disorder(lo, hi)
            mats = d.matrices()
            ms = d.last_timing()
            for k in range(2, 8):
                run[NAMES[k]] = round(float(ms[k]), 3)
            share = float(np.mean([d.disorder_codes(0)[:4096].mean()]))
        run["stats_ms_all"] = round(sum(x["stats_ms"] for x in run["adds"]), 3)
        assert np.all(np.isfinite(mats))
        res["runs"].append(run)
    res["disordered_share_of_a_prefix"] = share
    tpad = (T + 63) // 64 * 64
    best = {k: min(r[k] for r in res["runs"]) * 1e-3
            for k in NAMES[2:] + ("stats_ms_all",)}
    res["best_s"] = best
    res["count_passes_s"] = best["count_ss_ms"] + best["count_dd_ms"] + best["count_sd_ms"]

    def scan(seconds, nbytes):
        return {"best_s": seconds, "bytes": nbytes, "bytes_per_s": nbytes / seconds,
                "share_of_hbm_peak": nbytes / seconds / HBM_PEAK}

    res["stats_scan"] = scan(best["stats_ms_all"], 1.0 * K * F * tpad)
    res["disorder_scan"] = scan(best["disorder_ms"], 2.0 * K * F * tpad)

    rng = np.random.default_rng(1)
    A = rng.random((T, F), dtype=np.float32) * np.float32(359.9)
    kind = np.arange(F) % 3
    hb = [rotamer.KINDS[k][0] for k in ("phi", "psi", "chi")]
    sh = [rotamer.KINDS[k][1] for k in ("phi", "psi", "chi")]
    ms = np.zeros(2)
    rot = []
    rotamer.rotamer_states(A[:4096], kind, hb, sh, 15)
    for _ in range(a.repeats):
        rotamer.rotamer_states(A, kind, hb, sh, 15, timing=ms)
        rot.append(float(ms[1]))
    res["rotamer_scan_ms"] = [round(x, 3) for x in rot]
    res["rotamer_scan"] = scan(min(rot) * 1e-3, (2.0 * 4 + 1.0) * T * F)
    del A

    xyz = rng.random((T, a.atoms, 3), dtype=np.float32) * np.float32(5.0)
    start = rng.integers(0, a.atoms - 3, F)
    quads = start[:, None] + np.arange(4)[None, :]
    dih, fused = [], []
    rotamer.dihedral_rotamers(xyz[:4096], quads, kind, hb, sh, 15)
    rotamer.dihedral_angles(xyz[:4096], quads)
    for _ in range(a.repeats):
        # (ek_dihedral_angles through ctypes, for its event times)
        from enspara_amd import _lib
        out = np.zeros((T, F), dtype=np.float32)
        q32 = np.ascontiguousarray(quads, dtype=np.int32)
        _lib.check(_lib.load().ek_dihedral_angles(0, _lib.f32p(xyz), T, a.atoms, _lib.i32p(q32),
                                                  F, _lib.f32p(out), _lib.f64p(ms)))
        dih.append(float(ms[0]))
        rotamer.dihedral_rotamers(xyz, quads, kind, hb, sh, 15, timing=ms)
        fused.append(float(ms[1]))
    res["dihedral_ms"] = [round(x, 3) for x in dih]
    res["fused_ms"] = [round(x, 3) for x in fused]
    coord_b = 12.0 * T * a.atoms
    res["atoms"] = a.atoms
    res["dihedral_kernel"] = scan(min(dih) * 1e-3, coord_b + 4.0 * T * F)
    res["fused_scan"] = scan(min(fused) * 1e-3, 2 * coord_b + 1.0 * T * F)

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    if not ok:
        sys.exit("the device's statistics differ from the restatement's")


if __name__ == "__main__":
    main()
