#!/usr/bin/env python3
"""Generate tests/golden/dyes_golden.npz by running the REAL reference's dye-labelling
functions of enspara/geometry/dyes_from_expt_dist.py (mdtraj stubbed, as for the other
goldens; a small duck-typed object stands in for a trajectory).

    python tests/golden/make_dyes_golden.py

Only inputs and outputs are stored; no reference source is copied.  Every recorded
integer is checked here against the model (tests/_numpy_dyes.py): kept index sets and
bin counts must be equal, which also holds np.histogram -- what the reference calls -- to
the model's edge rule.  On the end-to-end case the model aligns in its own float32 order
and the reference through np.matmul: the seed is one for which both keep the same points
and count the same bins.

  pep_xyz [atoms, 3], pep_names, pep_seqs, pep_radii    the synthetic peptide
  geo_res [k]; geo_cb [k, 3]; geo_M [k, 3, 3]; geo_t [k, 3]; geo_dye [n, 3];
  geo_aligned [k, n, 3]       calc_cb_coords, determine_rot_mat, align_dye_to_res
  rt_coords [n, 3], rt_probe, rt_kept (indices), rt_kept_public
                              _remove_touches_protein, remove_touches_protein
  rtc_seed, rtc_n, rtc_radius, rtc_count, rtc_index_sum
                              remove_touches_protein above its 5e7 threshold (seeded cloud)
  bc_dists, bc_width, bc_counts, bc_edges               bincount_dists
  pd_a, pd_b, pd_width, pd_probs, pd_edges              pairwise_distance_distribution
  pc_seed, pc_n1, pc_n2, pc_width, pc_probs, pc_edges, pc_counts, pc_chunk_nbins
                              the same above the threshold (_numpy_dyes.chunk_clouds)
  e2e_dye1, e2e_dye2, e2e_res [2], e2e_probs, e2e_edges, e2e_kept0..3, e2e_counts0..1
                              _dye_distance_distribution on the peptide
"""
import os
import sys

import numpy as np
import scipy.spatial.distance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import import_reference  # noqa: E402
import _numpy_dyes as nd  # noqa: E402


def check(ok, what):
    if not ok:
        sys.exit("check failed: " + what)


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class FakePdb(object):
    """.xyz [1, atoms, 3], .top / .topology with residues (resSeq, atoms: name, index)
    and atoms (element.radius): what the reference's functions touch"""

    def __init__(self, xyz, names, seqs, radii):
        self.xyz = np.asarray(xyz, dtype=np.float32)[None]
        atoms = [_Obj(name=str(n), index=i, element=_Obj(radius=float(r)))
                 for i, (n, r) in enumerate(zip(names, radii))]
        residues = []
        for s in sorted(set(int(v) for v in seqs)):
            residues.append(_Obj(resSeq=s, atoms=[a for a, v in zip(atoms, seqs) if v == s]))
        self.top = self.topology = _Obj(residues=residues, atoms=atoms)


def main():
    import_reference()
    from enspara.geometry import dyes_from_expt_dist as rd

    out = {}
    rng = np.random.RandomState(7)
    xyz, names, seqs, radii = nd.peptide(rng, 60)
    pdb = FakePdb(xyz, names, seqs, radii)
    out.update(pep_xyz=xyz, pep_names=names.astype("U4"), pep_seqs=seqs, pep_radii=radii)

    # is cdist the contract's formula, bit for bit?
    a, b = nd.ball(rng, 300, 3.0), nd.ball(rng, 400, 3.0)
    check(np.array_equal(scipy.spatial.distance.cdist(a, b), nd.distances(a, b)),
          "cdist is sqrt((dx dx + dy dy) + dz dz) bit for bit")

    # ---- geometry --------------------------------------------------------------------------
    res = np.array([3, 17, 41, 58])
    dye = nd.ball(rng, 40, 1.2, centre=(0, 0, 0.9))
    out.update(geo_res=res, geo_dye=dye,
               geo_cb=np.asarray(rd.calc_cb_coords(pdb, resSeqs=res), dtype=np.float64))
    Ms, ts, al = [], [], []
    for r in res:
        M, t = rd.determine_rot_mat(pdb, int(r))
        Ms.append(np.asarray(M, dtype=np.float64))
        ts.append(np.asarray(t, dtype=np.float64))
        al.append(np.asarray(rd.align_dye_to_res(pdb, dye, int(r)), dtype=np.float64))
    out.update(geo_M=np.array(Ms), geo_t=np.array(ts), geo_aligned=np.array(al))

    # ---- touches ---------------------------------------------------------------------------
    cutoff17 = radii + 0.17
    coords = nd.ball(rng, 900, 2.0, centre=xyz[150])
    kept = rd._remove_touches_protein(coords, pdb, probe_radius=0.17)
    kept_pub = rd.remove_touches_protein(coords, pdb, probe_radius=0.17)
    mask = nd.keep_mask(coords, xyz, cutoff17)
    check(0 < mask.sum() < len(coords), "the touch case keeps some points and removes some")
    check(np.array_equal(kept, coords[mask]) and np.array_equal(kept_pub, coords[mask]),
          "touch model")
    out.update(rt_coords=coords, rt_probe=0.17, rt_kept=np.flatnonzero(mask).astype(np.int32),
               rt_kept_public=np.flatnonzero(mask).astype(np.int32))
    seed, n, rad = 1234, 170000, 3.0
    big = nd.touch_cloud(seed, n, rad, xyz[150])
    check(len(big) * len(xyz) > 5e7, "above the threshold of remove_touches_protein")
    kept = rd.remove_touches_protein(big, pdb, probe_radius=0.17)
    mask = nd.keep_mask(big, xyz, cutoff17)
    check(np.array_equal(kept, big[mask]), "chunked touch model")
    out.update(rtc_seed=seed, rtc_n=n, rtc_radius=rad, rtc_count=int(mask.sum()),
               rtc_index_sum=int(np.flatnonzero(mask).sum()))

    # ---- histograms ------------------------------------------------------------------------
    dists = rng.rand(7, 500) * 6.3
    counts, edges = rd.bincount_dists(dists, 0.1)
    check(np.array_equal(counts, nd.chunk_hist(dists, 0.1)), "bincount_dists against the edge rule")
    out.update(bc_dists=dists, bc_width=0.1, bc_counts=counts, bc_edges=edges)

    a, b = nd.ball(rng, 150, 1.4), nd.ball(rng, 170, 1.1, centre=(2.5, 1.0, -0.5))
    probs, edges = rd.pairwise_distance_distribution(a, b, bin_width=0.1)
    m_probs, m_edges = nd.pair_distribution(a, b, 0.1)
    check(np.array_equal(probs, m_probs) and np.array_equal(edges, m_edges), "pair model")
    out.update(pd_a=a, pd_b=b, pd_width=0.1, pd_probs=probs, pd_edges=edges)

    seed, n1, n2 = 99, 2049, 24500
    a, b = nd.chunk_clouds(seed, n1, n2)
    check(n1 * n2 > 5e7, "above the threshold of pairwise_distance_distribution")
    probs, edges = rd.pairwise_distance_distribution(a, b, bin_width=0.1)
    m_counts, m_nbins = nd.pair_counts(a, b, 0.1)
    m_edges = np.linspace(0, len(m_counts) * 0.1, len(m_counts) + 1)
    check(len(set(m_nbins)) > 1, "the chunks' numbers of bins differ")
    check(np.array_equal(probs, nd.int_norm_hist(m_edges, m_counts)) and
          np.array_equal(edges, m_edges), "chunked pair model")
    out.update(pc_seed=seed, pc_n1=n1, pc_n2=n2, pc_width=0.1, pc_probs=probs, pc_edges=edges,
               pc_counts=m_counts, pc_chunk_nbins=np.array(m_nbins))

    # ---- end to end ------------------------------------------------------------------------
    # With numpy 2 the reference's M comes out float64 (a float64 scalar times a float32
    # array) and so do its aligned clouds, where the contract rounds to float32: 2e-7 nm
    # at these coordinates, about one pair in 1.6e5 on the other side of an edge.  Of the
    # seeds 11 .. 21, 12, 15 and 18 give equal counts; 12 it is.
    rng = np.random.RandomState(12)
    dye1 = nd.ball(rng, 300, 1.3, centre=(0, 0, 1.0))
    dye2 = nd.ball(rng, 350, 1.5, centre=(0, 0, 1.1))
    res2 = [12, 47]
    probs, edges = rd._dye_distance_distribution(
        pdb, _Obj(xyz=dye1[None]), _Obj(xyz=dye2[None]), res2)
    bbs = [[int(np.flatnonzero((seqs == r) & (names == a))[0]) for a in ("N", "CA", "C")]
           for r in res2]
    m_probs, m_edges, m_kept, m_counts = nd.frame_distribution(
        xyz, radii + 0.2, dye1, dye2, bbs, 0.1)
    # the reference's own kept sets, placement by placement
    for p, (d, r) in enumerate(((dye1, 12), (dye1, 47), (dye2, 12), (dye2, 47))):
        al = rd.align_dye_to_res(pdb, d, r)
        ref_kept = rd.remove_touches_protein(al, pdb, probe_radius=0.2)
        check(0 < len(ref_kept) < len(d), "placement %d keeps some points" % p)
        ref_mask = nd.keep_mask(np.asarray(al), xyz, radii + 0.2)
        check(np.array_equal(np.flatnonzero(ref_mask), m_kept[p]),
              "end to end: kept set of placement %d" % p)
    check(np.array_equal(probs, m_probs) and np.array_equal(edges, m_edges),
          "end to end: the model's distribution is the reference's")
    out.update(e2e_dye1=dye1, e2e_dye2=dye2, e2e_res=np.array(res2), e2e_probs=probs,
               e2e_edges=edges, e2e_counts0=m_counts[0], e2e_counts1=m_counts[1])
    for p in range(4):
        out["e2e_kept%d" % p] = m_kept[p].astype(np.int32)

    path = os.path.join(HERE, "dyes_golden.npz")
    np.savez_compressed(path, **out)
    print("dyes_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
