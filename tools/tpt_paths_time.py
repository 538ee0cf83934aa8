#!/usr/bin/env python3
"""Time enspara_amd.tpt.path on the device.

    python tools/tpt_paths_time.py [--sizes 1500,4200] [--edges 20] [--paths 20]
                                   [--repeats 5] [--timeout 120]

One JSON line.  The sizes are measured in turn, `repeats` times over (so that a
drift of the machine touches all sizes alike), and every single measurement is a
process of its own (`--one N`) under its own time limit: this process never
touches the device, and it stops at the first measurement that fails.  Per size:
median and range over the repeats of
  compaction_s   the dense matrix to CSR on the device (count, scan, fill;
                 between HIP events, the upload not included), and the rate at
                 which it reads the n^2 doubles
  us_per_pop     the search launches' time (between HIP events) over the pops of
                 all searches
  ms_per_path    the same time over the paths found
  call_s         the whole paths() call on the host clock: upload, compaction,
                 searches, downloads
A measurement builds a seeded random matrix (tests/_numpy_tpt_paths.py
sparse_fluxes: `edges` entries from (0, 1) per row), runs the call once untimed
(code objects load on first use) and once timed, with remove_path='subtract',
sources [0], sinks [n - 1].
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

KEYS = ("compaction_s", "compaction_gb_s", "us_per_pop", "ms_per_path", "call_s")


def measure(n, edges, n_paths):
    import _numpy_tpt_paths as npp
    from enspara_amd.tpt import path as tp
    F = np.ascontiguousarray(npp.sparse_fluxes(n, edges, seed=n).toarray())
    src, snk = np.array([0], dtype=np.int32), np.array([n - 1], dtype=np.int32)
    total = tp._total_flux(F, src)
    out = {}
    for timed in (False, True):
        t0 = time.perf_counter()
        found = 0
        with tp._Search(F, src, snk, tp._SUBTRACT, n_paths, total, 1 - 1E-10, 0) as search:
            done = False
            while not done:
                batch, _, done = search.next()
                found += len(batch)
            (nnz, pops, paths, in_lds), (ms_compact, ms_search) = search.stats()
        out["call_s"] = time.perf_counter() - t0
    assert paths == found
    out.update(n=n, entries=nnz, pops=pops, paths=paths, in_lds=in_lds,
               compaction_s=ms_compact * 1e-3,
               compaction_gb_s=n * n * 8 / (ms_compact * 1e-3) / 1e9,
               us_per_pop=ms_search * 1e3 / pops, ms_per_path=ms_search / paths)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1500,4200")
    ap.add_argument("--edges", type=int, default=20)
    ap.add_argument("--paths", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=120)
    ap.add_argument("--one", type=int, default=0, help="measure this size once, here")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a.one, a.edges, a.paths)))
        return
    sizes = [int(s) for s in a.sizes.split(",") if s]
    runs = {n: [] for n in sizes}
    for _ in range(a.repeats):
        for n in sizes:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(n),
                                "--edges", str(a.edges), "--paths", str(a.paths)],
                               stdout=subprocess.PIPE, timeout=a.timeout)
            if r.returncode != 0:
                sys.exit("n = %d: the measurement ended with status %d" % (n, r.returncode))
            runs[n].append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    res = {"edges": a.edges, "repeats": a.repeats, "sizes": {}}
    for n in sizes:
        d = {k: runs[n][0][k] for k in ("entries", "pops", "paths", "in_lds")}
        for k in KEYS:
            v = [r[k] for r in runs[n]]
            d[k] = {"median": float(np.median(v)), "min": min(v), "max": max(v)}
        res["sizes"][str(n)] = d
    print(json.dumps(res))


if __name__ == "__main__":
    main()
