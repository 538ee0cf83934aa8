#!/usr/bin/env python3
"""Generate tests/golden/tpt_golden.npz by running the REAL reference's transition
path theory (bowman-lab/enspara, enspara/tpt/core.py and tpt.py) on seeded
metastable chains.

    python tests/golden/make_tpt_golden.py

The reference's tpt package needs nothing but enspara/exception.py and
enspara/msm/transition_matrices.py (numpy and scipy), so those files are copied
into a temporary package and imported from there; nothing is compiled.  Only
inputs and outputs are stored; no reference source is copied.

A chain `<c>` (n17, n63, n64, n65, n130, n130x with cross = 1e-5, n300) is stored
as its integer counts C_<c> (symmetric, so T = C / row sums is reversible with
populations = row sums / total: tests/_numpy_tpt.py tprob_from_counts,
pops_from_counts -- T itself would be eight times the bytes and is one exact
division away) and its seed.  Per result `<r>` = `<c>_<what>`:
  src_, snk_   the source and sink sets (as far as the function takes them)
  ref_<r>      the reference function's output x_ref (vectors; matrices at n = 17
               only -- the larger ones would take the file past its size limit,
               and tests need err_ only)
  hp_<r>       the high-precision result x_hp rounded to float64: the system solved
               by iterative refinement in long double with exact residuals
               (_numpy_tpt.solve_hp, accepted only when two successive iterates
               agree to 4 long-double ulps of max|x|), the epilogue in long double
  err_<r>      max|x_ref - x_hp|, taken in long double
`<what>`: qA / qM committors for the absorbing sets A = ({0}, {n - 1}) and M =
({n // 2}, {n // 2 + 1}); t1 / t3 mfpts to the sinks {n - 1} / {0, n // 2, n - 1};
tall all-to-all mfpts; fA / nA reactive and net fluxes for set A.  The
populations passed are always pops_from_counts(C).

The generator checks itself: it evaluates the tests' acceptance criteria
(backward error against numpy.linalg.solve's, forward error against err_) with
the numpy restatement standing in for the device, and moves to the next seed if
the restatement fails: a case in the file is one a second correct
implementation passes.
"""
import importlib
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import REF  # noqa: E402
import _numpy_tpt as nt  # noqa: E402

LD = np.longdouble

# chain -> (n, cross, all-to-all?, fluxes?)
CHAINS = {
    "n17": (17, 0.01, True, True),
    "n63": (63, 0.01, False, False),
    "n64": (64, 0.01, False, False),
    "n65": (65, 0.01, True, True),
    "n130": (130, 0.01, True, True),
    "n130x": (130, 1e-5, True, False),
    "n300": (300, 0.01, False, False),
}


def sets_of(n):
    return {"A": ([0], [n - 1]), "M": ([n // 2], [n // 2 + 1])}


def sinks_of(n):
    return {"t1": [n - 1], "t3": [0, n // 2, n - 1]}


def import_reference_tpt():
    tmp = tempfile.mkdtemp(prefix="enspara_ref_tpt_")
    for d in ("", "msm", "tpt"):
        os.makedirs(os.path.join(tmp, "enspara", d), exist_ok=True)
    open(os.path.join(tmp, "enspara", "__init__.py"), "w").close()
    open(os.path.join(tmp, "enspara", "msm", "__init__.py"), "w").close()
    shutil.copy(os.path.join(REF, "enspara", "exception.py"), os.path.join(tmp, "enspara"))
    shutil.copy(os.path.join(REF, "enspara", "msm", "transition_matrices.py"),
                os.path.join(tmp, "enspara", "msm"))
    for f in os.listdir(os.path.join(REF, "enspara", "tpt")):
        if f.endswith(".py"):
            shutil.copy(os.path.join(REF, "enspara", "tpt", f),
                        os.path.join(tmp, "enspara", "tpt"))
    sys.path.insert(0, tmp)
    return tmp, importlib.import_module("enspara.tpt")


class Reject(Exception):
    pass


def check(tag, x_np, x_hp, err_ref, system=None):
    """the tests' criteria with the restatement's x_np in the device's place"""
    fwd = float(np.max(np.abs(x_np.astype(LD) - x_hp)))
    bound = nt.forward_bound(err_ref, x_hp)
    line = "%-12s err_ref %.2e  restatement %.2e (%.2f of the bound)" % (
        tag, err_ref, fwd, fwd / bound)
    if system is not None:
        A, B, X = system
        eta = nt.backward_error(A, X, B)
        eta_ref = nt.backward_error(A, np.linalg.solve(A, B), B)
        line += "  eta %.2f u, numpy's %.2f u" % (eta / nt.U, eta_ref / nt.U)
        if not eta <= 8 * max(eta_ref, nt.U):
            raise Reject(line)
    if not fwd <= bound:
        raise Reject(line)
    print("   ", line, flush=True)


def chain_results(rtpt, name, C):
    n, _, want_all, want_flux = CHAINS[name]
    T = nt.tprob_from_counts(C)
    pops = nt.pops_from_counts(C)
    out = {}

    def store(r, x_ref, x_hp, keep_ref):
        err = float(np.max(np.abs(np.asarray(x_ref).astype(LD) - x_hp)))
        if keep_ref:
            out["ref_" + r] = np.asarray(x_ref, dtype=np.float64)
        out["hp_" + r] = x_hp.astype(np.float64)
        out["err_" + r] = np.array(err)
        return err

    q_hp = {}
    for tag, (src, snk) in sets_of(n).items():
        r = "%s_q%s" % (name, tag)
        out["src_" + r] = np.array(src, dtype=np.int32)
        out["snk_" + r] = np.array(snk, dtype=np.int32)
        A, b = nt.committor_system(T, src, snk)
        x_hp, _ = nt.solve_hp(A, b)
        x_hp[snk] = 1
        x_hp[src] = 0
        q_hp[tag] = x_hp
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x_ref = rtpt.committors(T.copy(), src, snk)
        err = store(r, x_ref, x_hp, True)
        X, _, info = nt.lu_solve(A, b)
        assert info < 0
        check(r, nt.committors(T, src, snk), x_hp, err, (A, b, X))
    for tag, snk in sinks_of(n).items():
        r = "%s_%s" % (name, tag)
        out["snk_" + r] = np.array(snk, dtype=np.int32)
        A, c = nt.mfpt_sink_system(T, snk)
        x_hp, _ = nt.solve_hp(A, c)
        x_ref = rtpt.mfpts(T.copy(), sinks=snk, populations=pops)
        err = store(r, x_ref, x_hp, True)
        check(r, nt.mfpts(T, sinks=snk), x_hp, err, (A, c, nt.solve(A, c)))
    if want_all:
        r = name + "_tall"
        A, eye = nt.mfpt_all_system(T, pops)
        Z, _ = nt.solve_hp(A, eye)
        x_hp = (np.diag(Z)[None, :] - Z) / pops.astype(LD)[None, :]
        x_ref = rtpt.mfpts(T.copy(), populations=pops)
        err = store(r, x_ref, x_hp, n <= 17)
        check(r, nt.mfpts(T, populations=pops), x_hp, err, (A, eye, nt.solve(A, eye)))
    if want_flux:
        src, snk = sets_of(n)["A"]
        f_hp = nt.fluxes_from(T.astype(LD), pops.astype(LD), q_hp["A"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            f_ref = rtpt.reactive_fluxes(T.copy(), src, snk, populations=pops)
            n_ref = rtpt.net_fluxes(T.copy(), src, snk, populations=pops)
        err = store(name + "_fA", f_ref, f_hp, n <= 17)
        check(name + "_fA", nt.reactive_fluxes(T, src, snk, pops), f_hp, err)
        n_hp = nt.net_from(f_hp.copy())
        err = store(name + "_nA", n_ref, n_hp, n <= 17)
        check(name + "_nA", nt.net_fluxes(T, src, snk, pops), n_hp, err)
    return out


def main():
    tmp, rtpt = import_reference_tpt()
    out = {}
    try:
        for name, (n, cross, _, _) in CHAINS.items():
            for seed in range(40):
                # (a chain that leaves a block once in 1e5 steps needs a long walk to
                # connect its blocks at all)
                C = nt.chain_counts(n, seed, cross=cross,
                                    steps=3000000 if cross < 1e-3 else None)
                print("%s seed %d" % (name, seed), flush=True)
                try:
                    res = chain_results(rtpt, name, C)
                except np.linalg.LinAlgError as e:
                    print("    rejected: disconnected (%s)" % e, flush=True)
                    continue
                except Reject as e:
                    print("    rejected:", e, flush=True)
                    continue
                break
            else:
                sys.exit("%s: no seed passes the restatement's check" % name)
            T = nt.tprob_from_counts(C)
            pops = nt.pops_from_counts(C)
            assert np.abs(pops @ T - pops).max() < 1e-15
            assert C.max() < 2 ** 31
            out["C_" + name] = C.astype(np.int32)
            out["seed_" + name] = np.array(seed)
            out.update(res)
        out["chains"] = np.array(list(CHAINS))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(HERE, "tpt_golden.npz")
    np.savez_compressed(path, **out)
    print("tpt_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
