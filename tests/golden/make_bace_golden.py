#!/usr/bin/env python3
"""Generate tests/golden/bace_golden.npz by running the REAL reference's BACE
(bowman-lab/enspara, enspara/msm/bace.py) on seeded count matrices.

    python tests/golden/make_bace_golden.py

bace.py needs nothing of the reference but enspara/exception.py, so the two files
(and the reference's test module, for its 9-state table and recorded results)
are copied into a temporary package and imported from there; nothing is
compiled.  Only inputs and outputs are stored; no reference source is copied.

Per case `<name>` the file holds
  C_          the input counts
  nmacro_     n_macrostates as enspara_amd is called
  p_          states the prune removes
  refnmacro_  n_macrostates the REFERENCE was called with: nmacro + p, so that it
              performs the m - nmacro merges that exist (its own count, n -
              n_macrostates, runs p merges on an all-zero matrix); its `labels`
              keys are then enspara_amd's + p, its `bayes_factors` keys equal
  bfk_, bfv_  the reference's bayes_factors (keys, float32 values)
  labk_, lab_ the reference's labels (keys, one row per key)
  rec_        (minX, minY) of every step, step 0 the initial matrix
  gap_        per step, (largest - second largest) / largest entry of the
              reference's matrix: the distance of its choice from a tie
  pd_, pc_, pl_, pk_   baysean_prune: the float32 factors, pruned counts, labels,
              kept states
The generator scans seeds until every step of a case has gap >= 1e-5 and no prune
factor lies within 1e-3 (relative) of log 3, so that the tests' conditions (1e-6,
1e-4) hold with a margin; `tcounts9`, the table of the paper, has exact ties and is
exempt.
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
import _numpy_bace as nb  # noqa: E402

MIN_GAP = 1e-5
MIN_PRUNE_MARGIN = 1e-3


def import_reference_bace():
    tmp = tempfile.mkdtemp(prefix="enspara_ref_bace_")
    os.makedirs(os.path.join(tmp, "enspara", "msm"))
    os.makedirs(os.path.join(tmp, "enspara", "test"))
    for d in ("", "msm", "test"):
        open(os.path.join(tmp, "enspara", d, "__init__.py"), "w").close()
    shutil.copy(os.path.join(REF, "enspara", "exception.py"),
                os.path.join(tmp, "enspara"))
    shutil.copy(os.path.join(REF, "enspara", "msm", "bace.py"),
                os.path.join(tmp, "enspara", "msm"))
    shutil.copy(os.path.join(REF, "enspara", "test", "test_bace.py"),
                os.path.join(tmp, "enspara", "test"))
    sys.path.insert(0, tmp)
    rbace = importlib.import_module("enspara.msm.bace")
    rtest = importlib.import_module("enspara.test.test_bace")
    return tmp, rbace, rtest


def ref_prune(rbace, C, **kw):
    seen = []
    orig = rbace.multiDistHelper

    def spy(*a, **k):
        r = orig(*a, **k)
        seen.append(np.array(r))
        return r
    rbace.multiDistHelper = spy
    try:
        pruned, labels, kept = rbace.baysean_prune(C.copy(), **kw)
    finally:
        rbace.multiDistHelper = orig
    return seen[0].astype(np.float32), np.asarray(pruned), np.asarray(labels), np.asarray(kept)


def ref_bace(rbace, C, nmacro):
    """The reference on C -> dict of arrays (see the module's docstring)."""
    d, pruned, plabels, kept = ref_prune(rbace, C)
    p = C.shape[0] - len(kept)
    steps = []
    orig = rbace.calcDMat

    def spy(*a, **k):
        dMat, x, y = orig(*a, **k)
        steps.append((int(x), int(y), nb.gap(dMat)))
        return dMat, x, y
    rbace.calcDMat = spy
    try:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            bf, labels = rbace.bace(C.copy(), nmacro + p)
    finally:
        rbace.calcDMat = orig
    bfk = np.array(sorted(bf, reverse=True), dtype=np.int64)
    labk = np.array(sorted(labels, reverse=True), dtype=np.int64)
    return {
        "C": C, "nmacro": np.array(nmacro), "p": np.array(p),
        "refnmacro": np.array(nmacro + p),
        "bfk": bfk, "bfv": np.array([bf[k] for k in bfk], dtype=np.float32),
        "labk": labk,
        "lab": (np.array([labels[k] for k in labk], dtype=np.int16)
                if len(labk) else np.zeros((0, C.shape[0]), dtype=np.int16)),
        "rec": np.array([s[:2] for s in steps], dtype=np.int32).reshape(-1, 2),
        "gap": np.array([s[2] for s in steps], dtype=np.float64),
        "pd": d, "pc": pruned, "pl": plabels.astype(np.int16), "pk": kept.astype(np.int32),
    }


def n24_counts(seed):
    """22 sampled states, one all-zero row and column (5) and one under-sampled
    state (17): p = 2"""
    inner = nb.block_chain_counts(22, 3, 6000, seed)
    idx = np.array([i for i in range(24) if i not in (5, 17)])
    C = np.zeros((24, 24), dtype=np.int64)
    C[np.ix_(idx, idx)] = inner
    C[17, 3] = 1
    C[3, 17] = 1
    return C


def asym_counts(seed):
    """pairs with c[s, d] > 1 and c[d, s] <= 1: listed from one side only"""
    C = nb.block_chain_counts(16, 2, 6000, seed)
    rng = np.random.RandomState(seed + 1000)
    iu = np.argwhere(np.triu(C > 1, 1) & (np.tril(C > 1, -1).T))
    for (s, d) in iu[rng.rand(len(iu)) < 0.5]:
        if rng.rand() < 0.5:
            C[d, s] = rng.randint(0, 2)
        else:
            C[s, d] = rng.randint(0, 2)
    return C


# name -> (counts(seed), n_macrostates or None for m, first seed)
CASES = {
    "n24_p2": (n24_counts, 2, 0),
    "n24_nomerge": (n24_counts, None, 0),
    "n70": (lambda seed: nb.block_chain_counts(70, 4, 40000, seed), 2, 0),
    "n300_sparse": (lambda seed: nb.block_chain_counts(300, 5, 150000, seed, degree=20),
                    2, 0),
    "asym16": (asym_counts, 2, 0),
}


def main():
    tmp, rbace, rtest = import_reference_bace()
    out = {}
    try:
        # the paper's table with the reference's recorded results
        g = ref_bace(rbace, np.array(rtest.TCOUNTS), 2)
        for k, v in g.items():
            out[k + "_tcounts9"] = v
        out["exp_bf_tcounts9"] = np.array(rtest.EXP_BAYES_FACTORS, dtype=np.float64)
        out["exp_labk_tcounts9"] = np.array(sorted(rtest.EXP_LABELS), dtype=np.int64)
        out["exp_lab_tcounts9"] = np.array(
            [rtest.EXP_LABELS[k] for k in sorted(rtest.EXP_LABELS)], dtype=np.int16)
        g = ref_bace(rbace, np.array([[400, 3], [4, 300]]), 2)
        for k, v in g.items():
            out[k + "_n2"] = v
        names = ["tcounts9", "n2"]
        for name, (make, nmacro, seed0) in CASES.items():
            for seed in range(seed0, seed0 + 40):
                C = make(seed)
                d, _, _, kept = ref_prune(rbace, C)
                nm = len(kept) if nmacro is None else nmacro
                g = ref_bace(rbace, C, nm)
                margin = np.abs(g["pd"] - nb.LOG3).min() / nb.LOG3
                if g["gap"].min() >= MIN_GAP and margin >= MIN_PRUNE_MARGIN:
                    break
            else:
                sys.exit("%s: no seed meets the gap condition" % name)
            if name.startswith("n24"):
                assert int(g["p"]) == 2 and g["pl"][5] == -1, (g["p"], g["pl"])
            if name == "asym16":
                c = g["pc"]
                assert np.any((c > 1) & ~(c.T > 1)), "no one-sided pair"
            print("%-14s seed %2d  n %3d  p %d  steps %3d  min gap %.2e  prune margin %.2e"
                  % (name, seed, C.shape[0], int(g["p"]), len(g["gap"]), g["gap"].min(),
                     margin), flush=True)
            for k, v in g.items():
                out[k + "_" + name] = v
            out["seed_" + name] = np.array(seed)
            names.append(name)
        # the prune's own small table (reference test_bace.py) at both factors
        T3 = np.array([[100, 10, 1], [10, 100, 0], [1, 0, 5]])
        out["C_prune3"] = T3
        for tag, kw in (("", {}), ("f13", {"factor": 1.3})):
            d, pc, pl, pk = ref_prune(rbace, T3, **kw)
            out["pd_prune3" + tag] = d
            out["pc_prune3" + tag] = pc
            out["pl_prune3" + tag] = pl.astype(np.int16)
            out["pk_prune3" + tag] = pk.astype(np.int32)
        out["cases"] = np.array(names)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for k, v in list(out.items()):
        if k.startswith(("C_", "pc_")) and np.all(v == np.round(v)) and v.max() < 2**31:
            out[k] = v.astype(np.int32)
    path = os.path.join(HERE, "bace_golden.npz")
    np.savez_compressed(path, **out)
    print("bace_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
