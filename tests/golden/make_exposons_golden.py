#!/usr/bin/env python3
"""Generate tests/golden/exposons_golden.npz.

    python tests/golden/make_exposons_golden.py

Needs the reference's test data (make_golden.REF) and scikit-learn; only data is
stored.

  The reference's beta-peptide fixture (enspara/test/data/beta-peptide.{pdb,xtc}):
    bp_xyz [106, 175, 3] float32   coordinates in nm read by oracle.xtc.read_xtc:
                                   frames 0 .. 5 (the ones the reference's
                                   test_exposons.py uses) and every 50th of the 5001
                                   (all of them are ten times the size limit of a
                                   committed file); bp_frames holds their numbers
    bp_names, bp_elements [175]    atom names and element symbols of the .pdb, the names
                                   as mdtraj reads them (the C terminus' OC1, OC2 are O,
                                   OXT)
    bp_resid [175]                 residue index of every atom, from 0
    bp_sc_offsets [11], bp_sc_atoms   the ten sidechain id lists of the reference's
                                   test_exposons.py, concatenated (checked here against
                                   the rule 'not N, C, CA, O, HA, H, H1, H2, H3, OXT')
    bp_counts [106, 175] int16     accessible points of 960 at probe 0.28 nm, radii by
                                   element, by the brute-force restatement tests/
                                   _numpy_sasa.py (minutes of numpy: recorded here, and
                                   tests/test_exposons_host.py repeats two frames)
  Affinity propagation, scikit-learn's AffinityPropagation(affinity='precomputed',
  preference=0, max_iter=10000, random_state=0) on small mutual-information matrices:
    ap_S_<k> [n, n], ap_damping [4] = 0.5, 0.75, 0.9, 0.95,
    ap_labels_<k> [4, n], ap_iter_<k> [4]       k = 0 .. 3: 12 features x 200 frames
        (the matrix of the issue), 7 x 50, 25 x 400, and bp: the mutual information of
        the ten sidechains' exposure (threshold 1.0) over frames 0 .. 5
    ap_zero_labels [6]             the all-zero 6 x 6 matrix (the equal-similarities
                                   shortcut)
    ap_short_labels, ap_short_iter   matrix 0 at damping 0.9 with max_iter = 5: stopped
                                   before it converged
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [HERE, os.path.dirname(HERE), ROOT]
from make_golden import REF  # noqa: E402
import _numpy_sasa as ns  # noqa: E402
import _numpy_wmi as nw  # noqa: E402
from oracle.xtc import read_xtc  # noqa: E402

EXPECTED_IDS = [
    list(range(6, 24)), list(range(30, 36)), list(range(42, 53)), list(range(59, 63)),
    list(range(69, 80)), [85, 86], list(range(93, 109)), list(range(115, 128)),
    list(range(134, 148)), list(range(154, 172))]
BACKBONE = {"N", "C", "CA", "O", "HA", "H", "H1", "H2", "H3", "OXT"}
RADII = {"H": 0.120, "C": 0.170, "N": 0.155, "O": 0.152}
DAMPING = [0.5, 0.75, 0.9, 0.95]


def read_pdb(path):
    names, elements, resid, last = [], [], [], None
    for line in open(path):
        if line.startswith("ENDMDL"):
            break
        if not line.startswith(("ATOM", "HETATM")):
            continue
        # (as mdtraj reads a .pdb: the terminal carboxylate's oxygens by their standard names)
        names.append({"OC1": "O", "OC2": "OXT"}.get(line[12:16].strip(), line[12:16].strip()))
        elements.append(line[76:78].strip().capitalize())
        key = (line[21], line[22:27])
        if key != last:
            resid.append((resid[-1] + 1) if resid else 0)
            last = key
        else:
            resid.append(resid[-1])
    return names, elements, np.array(resid)


def mi_matrix(rng, T, F):
    """the normalised weighted MI of F correlated binary features over T frames"""
    base = rng.rand(T, 3) < 0.5
    X = np.where(rng.rand(T, F) < 0.25, rng.rand(T, F) < 0.5, base[:, rng.randint(0, 3, F)])
    w = rng.rand(T)
    P = nw.joint_probabilities(X, nw.normalise(w), 2)
    return nw.finish(nw.mutual_information(P)[0], 2)


def sk_labels(S, damping, max_iter=10000):
    from sklearn.cluster import AffinityPropagation
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        c = AffinityPropagation(damping=damping, affinity="precomputed", preference=0,
                                max_iter=max_iter, random_state=0).fit(S)
    return c.labels_, c.n_iter_


def main():
    out = {}
    data = os.path.join(REF, "enspara", "test", "data")
    names, elements, resid = read_pdb(os.path.join(data, "beta-peptide.pdb"))
    xyz = read_xtc(os.path.join(data, "beta-peptide.xtc"))["xyz"]
    assert xyz.shape[1] == len(names) == 175 and xyz.dtype == np.float32
    frames = np.array(sorted(set(range(6)) | set(range(0, len(xyz), 50))))
    xyz = np.ascontiguousarray(xyz[frames])
    ids = [[a for a in np.flatnonzero(resid == r) if names[a] not in BACKBONE]
           for r in range(resid.max() + 1)]
    assert [list(map(int, i)) for i in ids[:10]] == EXPECTED_IDS, ids
    out["bp_xyz"], out["bp_frames"] = xyz, frames
    out["bp_names"], out["bp_elements"] = np.array(names), np.array(elements)
    out["bp_resid"] = resid.astype(np.int32)
    out["bp_sc_offsets"] = np.cumsum([0] + [len(i) for i in EXPECTED_IDS]).astype(np.int32)
    out["bp_sc_atoms"] = np.concatenate(EXPECTED_IDS).astype(np.int32)
    radii = np.array([RADII[e] for e in elements], dtype=np.float32)
    counts = ns.counts(xyz, radii, 0.28, 960)
    out["bp_counts"] = counts.astype(np.int16)
    print("beta-peptide: %d frames, counts %d .. %d, %.0f%% of atoms buried"
          % (len(xyz), counts.min(), counts.max(), 100 * (counts == 0).mean()))

    sasas = ns.group_sums(ns.areas(counts[:6], radii, 0.28, 960), EXPECTED_IDS)
    P = nw.joint_probabilities(sasas > 1.0, np.full(6, 1 / 6), 2)
    bp_mi = nw.finish(nw.mutual_information(P)[0], 2)
    rng = np.random.RandomState(7)
    mats = [mi_matrix(rng, 200, 12), mi_matrix(rng, 50, 7), mi_matrix(rng, 400, 25), bp_mi]
    out["ap_damping"] = np.array(DAMPING)
    for k, S in enumerate(mats):
        res = [sk_labels(S, d) for d in DAMPING]
        out["ap_S_%d" % k] = S
        out["ap_labels_%d" % k] = np.array([r[0] for r in res])
        out["ap_iter_%d" % k] = np.array([r[1] for r in res])
        print("matrix %d %s: iterations %s, clusters %s"
              % (k, S.shape, [r[1] for r in res], [len(set(r[0])) for r in res]))
    out["ap_zero_labels"] = sk_labels(np.zeros((6, 6)), 0.9)[0]
    out["ap_short_labels"], out["ap_short_iter"] = sk_labels(mats[0], 0.9, max_iter=5)
    print("zero:", out["ap_zero_labels"], "short:", out["ap_short_labels"],
          out["ap_short_iter"])
    path = os.path.join(HERE, "exposons_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
