#!/usr/bin/env python3
"""Time enspara_amd.tpt on the device against the numpy restatement on the host.

    python tools/tpt_time.py [--sizes 1000,5000] [--cpu-sizes 1000,5000]

One JSON line: per n the wall time of committors, mfpts(sinks=...) and all-to-all
mfpts on the device (whole call: upload, kernels, download; the second of two
calls), the kernel times of the all-to-all call by kind of launch from HIP events
(a call of its own with ek_lu_set_timing(1): the events serialise nothing but
cost a little), the trailing update's rate (its flops -- the right-hand sides'
columns included, as launched -- over its summed kernel time), and the same
three functions on the host: tests/_numpy_tpt.py's formulas on numpy.linalg.solve
(LAPACK on the threads OMP_NUM_THREADS allows; the restatement's own unblocked LU
is a correctness tool and would only time Python).  The reference itself is not
needed."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import _numpy_tpt as nt  # noqa: E402
from enspara_amd import _lib, tpt  # noqa: E402

KINDS = ["other", "panel", "swap", "trsm", "gemm", "back_trsm", "back_gemm"]


chain = nt.weighted_chain     # the chain tests/test_gpu_lu_large.py checks results on


def timed(fn, repeat=2):
    best = None
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return best, out


def np_solver(A, B):
    return np.linalg.solve(A, B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,5000")
    ap.add_argument("--cpu-sizes", default="1000,5000")
    a = ap.parse_args()
    L = _lib.load()
    res = {"threads": os.environ.get("OMP_NUM_THREADS"), "device": {}, "cpu": {}}
    cpu_sizes = [int(s) for s in a.cpu_sizes.split(",") if s]
    for n in [int(s) for s in a.sizes.split(",") if s]:
        T, pops = chain(n)
        src, snk, snk3 = [0], [n - 1], [0, n // 2, n - 1]
        d = {}
        d["committors_s"], q = timed(lambda: tpt.committors(T, src, snk))
        d["mfpts_sinks_s"], t3 = timed(lambda: tpt.mfpts(T, sinks=snk3))
        d["mfpts_all_s"], m = timed(lambda: tpt.mfpts(T, populations=pops))
        L.ek_lu_set_timing(1)
        tpt.mfpts(T, populations=pops)
        ms = np.zeros(7)
        fl = np.zeros(2)
        L.ek_lu_last_timing(ms.ctypes.data_as(C.POINTER(C.c_double)),
                            fl.ctypes.data_as(C.POINTER(C.c_double)))
        L.ek_lu_set_timing(0)
        d["mfpts_all_kernel_ms"] = {k: round(float(v), 3) for k, v in zip(KINDS, ms)}
        d["trailing_update_flops"] = float(fl[0])
        d["trailing_update_tflops"] = float(fl[0] / (ms[4] * 1e-3) / 1e12) if ms[4] else None
        d["back_update_tflops"] = float(fl[1] / (ms[6] * 1e-3) / 1e12) if ms[6] else None
        d["lu_only_flops_2n3_over_3"] = 2.0 * n ** 3 / 3
        res["device"][str(n)] = d
        if n in cpu_sizes:
            c = {}
            c["committors_s"], q0 = timed(lambda: nt.committors(T, src, snk, solver=np_solver))
            c["mfpts_sinks_s"], t0 = timed(lambda: nt.mfpts(T, sinks=snk3, solver=np_solver))
            c["mfpts_all_s"], m0 = timed(
                lambda: nt.mfpts(T, populations=pops, solver=np_solver), repeat=1)
            c["max_abs_diff"] = {"committors": float(np.abs(q - q0).max()),
                                 "mfpts_sinks_rel": float(np.abs(t3 - t0).max() / np.abs(t0).max()),
                                 "mfpts_all_rel": float(np.abs(m - m0).max() / np.abs(m0).max())}
            res["cpu"][str(n)] = c
    print(json.dumps(res))


if __name__ == "__main__":
    main()
