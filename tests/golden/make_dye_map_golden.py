#!/usr/bin/env python3
"""Generate tests/golden/dye_map_golden.npz by running the REAL reference's
remove_touches_protein_dye_traj and assemble_dye_r_mu of
enspara/geometry/explicit_r0_calc.py (mdtraj stubbed, as for the other goldens; small
duck-typed objects stand in for trajectories: ``top.select`` for exactly the strings those
two functions use, ``atom_slice``, ``.xyz``).

    python tests/golden/make_dye_map_golden.py

Only inputs and outputs are stored; no reference source is copied.  The reference's
align_full_dye_to_res is mdtraj's ``superpose`` and cannot be recorded: the goldens start
from coordinates aligned here with the float64 Kabsch model (tests/_numpy_rmsf.py), rounded
to float32.  Every recorded integer is checked against the numpy model
(tests/_numpy_dye_map.py) and the generator stops if they differ.

  pep_xyz [P, atoms, 3], pep_radii, pep_seqs        the synthetic peptides (one topology)
  resseq; aligned [P, D, A, 3] float32; dye_names [A]
  case<k>_probe, case<k>_tol, case<k>_counts [P, D], case<k>_kept (the centres' indices one
      after the other), case<k>_kept_off [P + 1]    remove_touches_protein_dye_traj, and the
      per-conformation counts of the remove_touches_protein it calls
  r_name, mu_names (as the library lists them), r_atom, mu_atoms (ascending: what select
      returns), rmu [P, D, 9]                       assemble_dye_r_mu on every conformation
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import import_reference  # noqa: E402
import _numpy_dye_map as dm  # noqa: E402

CASES = ((0.04, 6), (0.1, 2), (0.0, 0))


def check(ok, what):
    if not ok:
        sys.exit("check failed: " + what)


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class FakeTop(object):
    def __init__(self, names, seqs, radii):
        self.names = [str(n) for n in names]
        self.seqs = [int(s) for s in seqs]
        self.radii = [float(r) for r in radii]
        self.atoms = [_Obj(name=n, index=i, element=_Obj(radius=r))
                      for i, (n, r) in enumerate(zip(self.names, self.radii))]

    def select(self, text):
        """ascending indices, as mdtraj returns them, for the three forms in use"""
        m = re.fullmatch(r"not resSeq (\d+)", text)
        if m:
            return np.array([i for i, s in enumerate(self.seqs) if s != int(m.group(1))])
        m = re.fullmatch(r"\(name (\w+)\) or \(name (\w+)\)", text)
        if m:
            return np.array([i for i, n in enumerate(self.names) if n in m.groups()])
        m = re.fullmatch(r"\(name (\w+)\)", text)
        if m:
            return np.array([i for i, n in enumerate(self.names) if n == m.group(1)])
        raise ValueError("select(%r) is not one of the forms the two functions use" % text)


class FakeTraj(object):
    def __init__(self, xyz, top):
        self.xyz = np.asarray(xyz, dtype=np.float32)
        self.top = self.topology = top

    def atom_slice(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        t = self.top
        return FakeTraj(self.xyz[:, idx], FakeTop([t.names[i] for i in idx],
                                                  [t.seqs[i] for i in idx],
                                                  [t.radii[i] for i in idx]))


def main():
    import_reference()
    from enspara.geometry import dyes_from_expt_dist as rd
    from enspara.geometry import explicit_r0_calc as rr0

    resseq, D, A, P = 23, 48, 24, 3
    case = dm.peptide_case(2, resseq, D=D, A=A, P=P)
    rng = np.random.RandomState(2)
    _, names, seqs, radii = dm.nd.peptide(rng, 60)
    xyz, dye = case["xyz"], case["dye_xyz"]
    aligned = np.stack([dm.model_align(dye, xyz[p], case["prot_sel"], case["dye_sel"])["aligned"]
                        for p in range(P)]).astype(np.float32)
    dye_names = ["N", "CA", "CB", "C", "O"] + ["C%d" % i for i in range(5, A)]
    # the library lists the dipole's atoms in DESCENDING index order on purpose: select
    # returns them ascending, and the origin is the lower-indexed one
    library = {"dye": {"r": ["C23"], "mu": ["C21", "C18"]}}
    r_atom, mu_atoms = 23, (18, 21)
    dye_top = FakeTop(dye_names, [1] * A, [0.17] * A)
    out = dict(pep_xyz=xyz, pep_radii=radii, pep_seqs=seqs, resseq=resseq, aligned=aligned,
               dye_names=np.array(dye_names, dtype="U4"), r_name="C23",
               mu_names=np.array(library["dye"]["mu"], dtype="U4"), r_atom=r_atom,
               mu_atoms=np.array(mu_atoms))
    check(np.array_equal(np.flatnonzero(seqs == resseq), case["exclude_atoms"]),
          "the residue's atoms are what 'not resSeq' leaves out")

    rmu = []
    for p in range(P):
        got = rr0.assemble_dye_r_mu(FakeTraj(aligned[p], dye_top), "dye", library)
        check(np.array_equal(np.asarray(got, dtype=np.float64), dm.r_mu(aligned[p], r_atom, mu_atoms)),
              "r / mu model, centre %d" % p)
        rmu.append(np.asarray(got, dtype=np.float64))
    out["rmu"] = np.array(rmu)

    for k, (probe, tol) in enumerate(CASES):
        counts, kept = [], []
        for p in range(P):
            pdb = FakeTraj(xyz[p][None], FakeTop(names, seqs, radii))
            traj = FakeTraj(aligned[p], dye_top)
            if probe == 0.04 and tol == 6:      # the reference's defaults, left to it
                ref_kept = rr0.remove_touches_protein_dye_traj(pdb, traj, resseq)
            else:
                ref_kept = rr0.remove_touches_protein_dye_traj(pdb, traj, resseq,
                                                               probe_radius=probe, atom_tol=tol)
            sliced = pdb.atom_slice(pdb.top.select("not resSeq %d" % resseq))
            ref_counts = np.array([np.shape(rd.remove_touches_protein(f, sliced, probe_radius=probe))[0]
                                   for f in traj.xyz])
            m_counts = dm.touch_counts(aligned[p], xyz[p], radii + probe, case["exclude_atoms"])
            check(np.array_equal(ref_counts, m_counts), "counts model, case %d centre %d" % (k, p))
            check(np.array_equal(ref_kept, dm.kept(m_counts, A, tol)),
                  "kept model, case %d centre %d" % (k, p))
            counts.append(ref_counts.astype(np.int32))
            kept.append(np.asarray(ref_kept, dtype=np.int64))
        n_kept = sum(len(q) for q in kept)
        check(0 < n_kept < P * D, "case %d keeps some conformations and removes some" % k)
        out.update({"case%d_probe" % k: probe, "case%d_tol" % k: tol,
                    "case%d_counts" % k: np.array(counts),
                    "case%d_kept" % k: np.concatenate(kept),
                    "case%d_kept_off" % k: np.concatenate([[0], np.cumsum([len(q) for q in kept])])})
        print("case", k, "probe", probe, "atom_tol", tol, "kept", [len(q) for q in kept], "of", D)

    path = os.path.join(HERE, "dye_map_golden.npz")
    np.savez_compressed(path, **out)
    print("dye_map_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
