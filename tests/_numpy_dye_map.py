"""A brute-force numpy model of the dye-mapping contract and the fixtures
its host and GPU tests share (numpy only).

The touch test takes every square root and looks at every atom that is not excluded:
nothing of the device's thresholds on squared distances or of its cull is in here.  The
alignment is NOT restated operation for operation: the float64 Kabsch model of
tests/_numpy_rmsf.py is the yardstick for it, and everything after it is checked on the
bits the device returned (``return_aligned``).
"""
import numpy as np

import _numpy_dyes as nd
import _numpy_rmsf as nr

F32 = np.float32
# the synthetic peptide's atoms of a residue are N, CA, C, O, CB (_numpy_dyes.peptide); the
# reference fits N, CA, CB, C, O
RESIDUE_ORDER = {"N": 0, "CA": 1, "C": 2, "O": 3, "CB": 4}
FIT_NAMES = ("N", "CA", "CB", "C", "O")
# local geometry of a residue (nm), as _numpy_dyes.peptide lays it out along (direction,
# side, up)
LOCAL = {"N": (-0.12, 0.05, 0.0), "CA": (0.0, 0.0, 0.0), "C": (0.13, 0.06, 0.0),
         "O": (0.15, 0.17, 0.0), "CB": (-0.02, -0.08, 0.12)}


# ---- the contract ------------------------------------------------------------------------------
def free_atoms(points, frame_xyz, cutoff, exclude=()):
    """bool [n]: the points farther than the cutoff from every atom outside ``exclude``:
    sqrt((dx dx + dy dy) + dz dz) > cutoff, d = float64(atom) - float64(point)"""
    use = np.ones(len(frame_xyz), dtype=bool)
    use[np.asarray(exclude, dtype=np.int64)] = False
    if not use.any():
        return np.ones(len(points), dtype=bool)
    return nd.keep_mask(np.asarray(points), np.asarray(frame_xyz)[use],
                        np.asarray(cutoff, np.float64)[use])


def touch_counts(aligned, frame_xyz, cutoff, exclude=()):
    """int32 [D]: the atoms of every conformation of aligned [D, A, 3] that touch nothing"""
    aligned = np.asarray(aligned)
    D, A = aligned.shape[:2]
    free = free_atoms(aligned.reshape(D * A, 3), frame_xyz, cutoff, exclude)
    return free.reshape(D, A).sum(axis=1).astype(np.int32)


def kept(counts, n_dye_atoms, atom_tol):
    """the reference's np.where(counts >= len(dye.xyz[0]) - atom_tol)[0]"""
    return np.flatnonzero(np.asarray(counts) >= n_dye_atoms - atom_tol).astype(np.int64)


def r_mu(aligned, r_atom, mu_atoms):
    """float64 [D, 9] of float32 coordinates: the emission centre, the first dipole atom, and
    the float32 difference first - second (assemble_dye_r_mu of the reference)"""
    a = np.asarray(aligned)
    assert a.dtype == F32
    out = np.empty((len(a), 9), dtype=np.float64)
    out[:, 0:3] = a[:, r_atom]
    out[:, 3:6] = a[:, mu_atoms[0]]
    out[:, 6:9] = a[:, mu_atoms[0]] - a[:, mu_atoms[1]]       # float32, one rounding
    return out


# ---- the float64 alignment model ---------------------------------------------------------------
def padded_ref(frame_xyz, prot_sel, dye_sel, n_dye_atoms):
    """[A, 3] with the frame's prot_sel coordinates at the dye_sel rows: what
    _numpy_rmsf.kabsch_superpose(dye_xyz, padded_ref, dye_sel) fits on"""
    ref = np.zeros((n_dye_atoms, 3), dtype=np.float64)
    ref[np.asarray(dye_sel)] = np.asarray(frame_xyz, dtype=np.float64)[np.asarray(prot_sel)]
    return ref


def model_align(dye_xyz, frame_xyz, prot_sel, dye_sel):
    """_numpy_rmsf.kabsch_superpose on the padded reference.  One repair: the model signs its
    third singular vector like det H, and for a selection of three atoms (always planar: H has
    rank two) det H is rounding noise of either sign, so that about half its 'rotations' come
    out as reflections.  Where det R < 0 the frame is fitted again with the sign taken from
    det(V U^T), which is the same sign wherever det H is not noise, and always gives the
    proper rotation."""
    ref = padded_ref(frame_xyz, prot_sel, dye_sel, np.shape(dye_xyz)[1])
    m = nr.kabsch_superpose(dye_xyz, ref, dye_sel)
    sel = np.asarray(dye_sel)
    X = np.asarray(dye_xyz, dtype=np.float64)
    for f in np.flatnonzero(np.linalg.det(m["R"]) < 0):
        cx, cy = X[f, sel].mean(axis=0), ref[sel].mean(axis=0)
        H = (X[f, sel] - cx).T @ (ref[sel] - cy)
        U, s, Vt = np.linalg.svd(H / np.abs(H).max())
        assert s[2] <= 1e-12 * s[0], "det H < 0 on a selection that is not planar"
        d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
        m["R"][f] = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
        m["aligned"][f] = (X[f] - cx) @ m["R"][f].T + cy
    return m


def count_range(model_aligned, bound, frame_xyz, cutoff, exclude=()):
    """What the model decides when the device's atoms may lie anywhere within bound [D] (per
    coordinate) of the model's: (lo, hi, model) int32 [D] -- the atoms that are free for
    certain, those plus the undecided ones, and the model's own count.  An atom is undecided
    iff some distance lies within sqrt(3) bound of its cutoff and no other distance decides
    'touch'."""
    m = np.asarray(model_aligned, dtype=np.float64)
    D, A = m.shape[:2]
    use = np.ones(len(frame_xyz), dtype=bool)
    use[np.asarray(exclude, dtype=np.int64)] = False
    dist = nd.distances(np.asarray(frame_xyz)[use], m.reshape(D * A, 3))        # [atoms, D A]
    cut = np.asarray(cutoff, np.float64)[use][:, None]
    e = np.repeat(np.sqrt(3.0) * np.asarray(bound, dtype=np.float64), A)[None, :]
    sure_free = np.all(dist > cut + e, axis=0).reshape(D, A)
    sure_touch = np.any(dist <= cut - e, axis=0).reshape(D, A)
    model = np.all(dist > cut, axis=0).reshape(D, A)
    lo = sure_free.sum(axis=1)
    hi = A - sure_touch.sum(axis=1)
    return lo.astype(np.int32), hi.astype(np.int32), model.sum(axis=1).astype(np.int32)


# ---- fixtures ----------------------------------------------------------------------------------
def residue_atoms(resseq):
    """atom indices of residue resseq (1-based) of _numpy_dyes.peptide: all five"""
    return 5 * (resseq - 1) + np.arange(5, dtype=np.int32)


def residue_sel(resseq, names=FIT_NAMES):
    return np.array([5 * (resseq - 1) + RESIDUE_ORDER[n] for n in names], dtype=np.int32)


def random_rotation(rng):
    q, r = np.linalg.qr(rng.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def dye_library(rng, D, A, template, tail_from, step=0.14, noise=0.005, drift=0.8):
    """D conformations of A atoms, float32: the first len(template) atoms are the template
    (nm) with a little noise -- the atoms the fit uses --, the rest a random walk that
    starts at atom tail_from and drifts away from the template's centre (by `drift`); every
    conformation then gets its own random rigid motion."""
    template = np.asarray(template, dtype=np.float64)
    n = len(template)
    out = np.empty((D, A, 3))
    for d in range(D):
        x = np.empty((A, 3))
        x[:n] = template + noise * rng.randn(n, 3)
        pos = x[tail_from].copy()
        away = x[tail_from] - x[:n].mean(axis=0)
        away /= np.linalg.norm(away)
        for i in range(n, A):
            v = rng.randn(3) + drift * away
            pos = pos + step * v / np.linalg.norm(v)
            x[i] = pos
        out[d] = x @ random_rotation(rng).T + 2.0 * rng.randn(3)
    return out.astype(F32)


def peptide_case(seed, resseq, D=96, A=24, names=FIT_NAMES, P=6):
    """P peptides of 60 residues (one topology, P conformations) labelled at residue resseq,
    and a dye library whose first len(names) atoms are backbone-like: a dict of the
    arguments of map_dye_on_protein"""
    rng = np.random.RandomState(seed)
    peps = [nd.peptide(rng, 60) for _ in range(P)]
    xyz = np.stack([p[0] for p in peps])
    radii = peps[0][3]
    template = np.array([LOCAL[n] for n in names])
    tail_from = names.index("CB") if "CB" in names else names.index("CA")
    dye = dye_library(rng, D, A, template, tail_from)
    return dict(xyz=xyz, radii=radii, dye_xyz=dye, prot_sel=residue_sel(resseq, names),
                dye_sel=np.arange(len(names), dtype=np.int32),
                exclude_atoms=residue_atoms(resseq), r_atom=A - 1, mu_atoms=(A - 3, A - 6))


def window_case(seed, resseq, n_sel=16, D=96, A=24, P=6):
    """a selection of n_sel atoms: the protein atoms from the residue before resseq on, paired
    with a dye whose first n_sel atoms are those atoms of centre 0 (with noise)"""
    rng = np.random.RandomState(seed)
    peps = [nd.peptide(rng, 60, spacing=0.38) for _ in range(P)]
    # (centres 1.. are centre 0 with small displacements, so that the window keeps its shape)
    xyz = np.stack([peps[0][0] + (0.01 * rng.randn(*peps[0][0].shape)).astype(F32)
                    for _ in range(P)])
    radii = peps[0][3]
    first = 5 * (resseq - 2)
    prot_sel = np.arange(first, first + n_sel, dtype=np.int32)
    template = xyz[0][prot_sel].astype(np.float64)
    template -= template.mean(axis=0)
    dye = dye_library(rng, D, A, template, n_sel - 1, noise=0.01)
    return dict(xyz=xyz, radii=radii, dye_xyz=dye, prot_sel=prot_sel,
                dye_sel=np.arange(n_sel, dtype=np.int32), exclude_atoms=residue_atoms(resseq),
                r_atom=A - 1, mu_atoms=(A - 2, A - 4))


def blob_case(seed, D=130, A=70, n_blob=3000):
    """one centre: a residue at the origin inside a dense blob of n_blob random atoms in a
    ball of 2 nm around it"""
    rng = np.random.RandomState(seed)
    res = np.array([LOCAL[n] for n in ("N", "CA", "C", "O", "CB")]) + 0.005 * rng.randn(5, 3)
    blob = nd.ball(rng, n_blob, 2.0)
    xyz = np.concatenate([res.astype(F32), blob])[None]
    radii = np.concatenate([[0.155, 0.17, 0.17, 0.152, 0.17], 0.12 + 0.06 * rng.rand(n_blob)])
    template = np.array([LOCAL[n] for n in FIT_NAMES])
    dye = dye_library(rng, D, A, template, 2, step=0.05)
    return dict(xyz=xyz, radii=radii, dye_xyz=dye, prot_sel=residue_sel(1),
                dye_sel=np.arange(5, dtype=np.int32), exclude_atoms=residue_atoms(1),
                r_atom=A - 1, mu_atoms=(A - 3, A - 6))
