"""Superposition on a reference structure and population-weighted RMSF on the
device (reference enspara/geometry/rmsf.py and the ``md.Trajectory.superpose`` it
calls; csrc/ek_rmsf.hip, csrc/ek_superpose.h; the contract is DESIGN.md 4o).

Every frame is superposed on one reference structure over a selection of atoms:
centroid of the selection in float64, centred coordinates and the 3x3
inner-product matrix rounded to float32, the largest root of Theobald's quartic
by the iteration of the RMSD kernels, the rotation from the adjugate of
``K - lambda I`` in float64.  ``aligned = float32(R (x - c_x) + c_ref)`` moves the
centroid of a frame's selected atoms onto the reference's, as
``md.Trajectory.superpose`` does.  The RMSF is ``sqrt(sum_f w_f d_fa^2)`` per atom,
``sqrt(sum_f w_f mean_{a in res} d_fa^2)`` per residue, ``d_fa`` the distance of
aligned frame ``f`` from the unmoved reference frame at atom ``a``; the sums are
float64 in a fixed tree over absolute frame indices (tiles of ``TILE`` frames in
frame order, the tiles then in order), so the bits do not depend on
``chunk_frames``; the square roots are numpy's.

There is no topology reader: residues are an integer per atom
(``residue_index``), selections are index arrays.

Two differences from mdtraj, on purpose:

1. The reference frame is not rotated onto itself: its aligned copy is its own
   bits and its deviation is exactly 0.
2. A frame whose optimal rotation is not determined -- a collinear or two-point
   selection, or singular values with ``s2 + s3 ~ 0``: the gap of the two largest
   eigenvalues of the key matrix at most ``2e-5 (Gx + Gy)`` -- raises
   ``DataInvalid`` naming the first such frame, where mdtraj returns an arbitrary
   member of the solution set.  (A gap of ``1e-7 (Gx + Gy)`` or less is always
   refused, one of ``1e-4 (Gx + Gy)`` or more never.)
"""
import ctypes as C

import numpy as np

from .. import _lib, exception

__all__ = ["superpose", "rmsf_calc", "bfactors_from_rmsfs", "last_timing", "TILE",
           "LDS_ATOMS", "WAVE_ATOMS"]

# RMSF_TILE, RMSF_LDS_ATOMS, RMSF_WAVE_ATOMS of csrc/ek_rmsf.hip
TILE = 32
LDS_ATOMS = 3072
WAVE_ATOMS = 512

_timing = np.zeros(3)


def _frames(xyz, name):
    xyz = np.asarray(xyz)
    if xyz.ndim != 3 or xyz.shape[2] != 3 or xyz.shape[0] < 1:
        raise exception.DataInvalid("%s is [frames, atoms, 3], not %s" % (name, xyz.shape))
    if xyz.dtype != np.float32:
        raise exception.DataInvalid("%s is float32, not %s" % (name, xyz.dtype))
    if xyz.shape[1] < 3:
        raise exception.DataInvalid(
            "%s has %d atoms; a superposition needs at least 3." % (name, xyz.shape[1]))
    if not np.isfinite(xyz).all():
        raise exception.DataInvalid("%s holds coordinates that are not finite." % name)
    return np.ascontiguousarray(xyz)


def _selection(atom_indices, atoms):
    if atom_indices is None:
        return np.arange(atoms, dtype=np.int32)
    sel = np.asarray(atom_indices)
    if sel.ndim != 1 or not np.issubdtype(sel.dtype, np.integer):
        raise exception.DataInvalid("atom_indices is a 1-D integer array.")
    if sel.size < 3:
        raise exception.DataInvalid(
            "atom_indices selects %d atoms; a superposition needs at least 3." % sel.size)
    if sel.min() < 0 or sel.max() >= atoms:
        raise exception.DataInvalid(
            "atom_indices index atoms %d .. %d; there are %d atoms."
            % (sel.min(), sel.max(), atoms))
    if np.unique(sel).size != sel.size:
        raise exception.DataInvalid("atom_indices must be unique.")
    return np.ascontiguousarray(sel, dtype=np.int32)


def _chunk(chunk_frames):
    if chunk_frames is None:
        return 0
    if isinstance(chunk_frames, bool) or not isinstance(chunk_frames, (int, np.integer)) \
            or chunk_frames < 1:
        raise exception.DataInvalid("chunk_frames = %r is not a positive integer" % (chunk_frames,))
    return int(chunk_frames)


def _residues(residue_index, atoms):
    """-> (offsets [groups + 1], atoms [atoms]) int32: the distinct values in order of
    first appearance, each residue's atoms ascending"""
    res = np.asarray(residue_index)
    if res.shape != (atoms,) or not np.issubdtype(res.dtype, np.integer):
        raise exception.DataInvalid(
            "residue_index is an integer array of shape (%d,), not %s of %s"
            % (atoms, res.dtype, res.shape))
    _, first, inverse = np.unique(res, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(first))        # sorted value -> order of appearance
    order = np.argsort(rank[inverse], kind="stable")
    counts = np.bincount(rank[inverse])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return offsets, np.ascontiguousarray(order, dtype=np.int32)


def _run(xyz, reference, sel, weights, ref_index, groups, chunk, device, want_aligned,
         want_transforms):
    frames, atoms = xyz.shape[:2]
    L = _lib.load()
    flags = np.zeros(frames, dtype=np.uint32)
    aligned = np.empty_like(xyz) if want_aligned else None
    rot = np.empty((frames, 3, 3), dtype=np.float64) if want_transforms else None
    rmsd = np.empty(frames, dtype=np.float32) if want_transforms else None
    goff, gidx = groups if groups is not None else (None, None)
    sums = np.empty(atoms, dtype=np.float64) if weights is not None else None
    gsums = np.empty(len(goff) - 1, dtype=np.float64) if groups is not None else None
    h = C.c_void_p()
    _check(L.ek_rmsf_open(int(device), atoms, len(sel), _lib.i32p(sel), _lib.f32p(reference),
                          0 if goff is None else len(goff) - 1,
                          None if goff is None else _lib.i32p(goff),
                          None if gidx is None else _lib.i32p(gidx), C.byref(h)))
    try:
        _check(L.ek_rmsf_run(h, _lib.f32p(xyz), frames,
                             None if weights is None else _lib.f64p(weights), int(ref_index),
                             int(chunk), None if aligned is None else _lib.f32p(aligned),
                             None if rot is None else _lib.f64p(rot),
                             None if rmsd is None else _lib.f32p(rmsd), _lib.u32p(flags)))
        _check(L.ek_rmsf_last_timing(h, _lib.f64p(_timing)))
        bad = np.flatnonzero(flags & 1)
        if bad.size:
            raise exception.DataInvalid(
                "The optimal rotation of frame %d is not determined (collinear or "
                "two-point selection, or s2 + s3 ~ 0); %d such frames." % (bad[0], bad.size))
        if weights is not None:
            _check(L.ek_rmsf_fetch(h, _lib.f64p(sums), None if gsums is None else _lib.f64p(gsums)))
    finally:
        L.ek_rmsf_close(h)
    return aligned, rot, rmsd, sums, gsums


def superpose(xyz, reference, atom_indices=None, return_transforms=False, chunk_frames=None,
              device=0):
    """Superpose every frame on ``reference`` over ``atom_indices``.

    Parameters
    ----------
    xyz : np.ndarray, shape=(frames, atoms, 3), float32
    reference : np.ndarray, shape=(atoms, 3), float32
    atom_indices : integer array, default=None
        The atoms that define the fit (unique, at least 3); all atoms by default.
    return_transforms : bool, default=False
        Also return the rotations and the minimal RMSD over the selection.
    chunk_frames : int, default=None
        Frames of one upload and launch; by default what fits the device.
    device : int
        The HIP device.

    Returns
    -------
    aligned : np.ndarray, float32, shape=(frames, atoms, 3)
        ``R (x - c_x) + c_ref``: the centroid of a frame's selected atoms lies on the
        reference's.
    rotations : np.ndarray, float64, shape=(frames, 3, 3)  (with ``return_transforms``)
    rmsd : np.ndarray, float32, shape=(frames,)  (with ``return_transforms``)
    """
    xyz = _frames(xyz, "xyz")
    atoms = xyz.shape[1]
    reference = np.asarray(reference)
    if reference.shape != (atoms, 3):
        raise exception.DataInvalid(
            "reference is [%d, 3], not %s" % (atoms, reference.shape))
    if reference.dtype != np.float32:
        raise exception.DataInvalid("reference is float32, not %s" % reference.dtype)
    if not np.isfinite(reference).all():
        raise exception.DataInvalid("reference holds coordinates that are not finite.")
    reference = np.ascontiguousarray(reference)
    sel = _selection(atom_indices, atoms)
    chunk = _chunk(chunk_frames)
    aligned, rot, rmsd, _, _ = _run(xyz, reference, sel, None, -1, None, chunk, device, True,
                                    bool(return_transforms))
    return (aligned, rot, rmsd) if return_transforms else aligned


def _rmsf_sums(centers, populations, ref_frame, atom_indices, groups, chunk_frames, device,
               want_aligned=False):
    """the validated device call behind rmsf_calc -> (atom sums, group sums, aligned)"""
    centers = _frames(centers, "centers")
    n, atoms = centers.shape[:2]
    if isinstance(ref_frame, bool) or not isinstance(ref_frame, (int, np.integer)) \
            or not 0 <= ref_frame < n:
        raise exception.DataInvalid("ref_frame = %r is not in [0, %d)" % (ref_frame, n))
    if populations is None:
        w = np.full(n, 1.0 / n, dtype=np.float64)
    else:
        w = np.asarray(populations)
        if w.shape != (n,) or not (np.issubdtype(w.dtype, np.floating) or
                                   np.issubdtype(w.dtype, np.integer)):
            raise exception.DataInvalid(
                "populations is a real array of shape (%d,), not %s of %s" % (n, w.dtype, w.shape))
        w = np.ascontiguousarray(w, dtype=np.float64)
        if not (np.isfinite(w).all() and (w >= 0).all()):
            raise exception.DataInvalid("populations must be finite and non-negative.")
    sel = _selection(atom_indices, atoms)
    chunk = _chunk(chunk_frames)
    reference = np.ascontiguousarray(centers[ref_frame])
    aligned, _, _, sums, gsums = _run(centers, reference, sel, w, ref_frame, groups, chunk,
                                      device, want_aligned, False)
    return sums, gsums, aligned


def rmsf_calc(centers, populations=None, ref_frame=0, per_residue=True, atom_indices=None,
              residue_index=None, chunk_frames=None, device=0):
    """Population-weighted root mean square fluctuation about ``centers[ref_frame]``.

    Parameters
    ----------
    centers : np.ndarray, shape=(n, atoms, 3), float32
        Frames or cluster centres.
    populations : array, shape=(n,), default=None
        Weights; ``1 / n`` each by default.  Not renormalised.
    ref_frame : int, default=0
        The frame every other one is superposed on; it is not moved.
    per_residue : bool, default=True
        Average the mean square deviation over each residue's atoms.
    atom_indices : integer array, default=None
        The atoms that define the fit; all atoms by default.
    residue_index : integer array, shape=(atoms,)
        The residue of every atom; residues are the distinct values in order of first
        appearance.  Required with ``per_residue``.
    chunk_frames : int, default=None
        Frames of one upload and launch; the result's bits do not depend on it.
    device : int
        The HIP device.

    Returns
    -------
    rmsfs : np.ndarray, float64, shape=(residues,) or (atoms,)
    """
    if per_residue and residue_index is None:
        raise exception.ImproperlyConfigured(
            "per_residue=True needs residue_index (one integer per atom); there is no "
            "topology to read residues from.")
    groups = None
    if per_residue:
        shape = np.shape(centers)
        if len(shape) != 3:
            raise exception.DataInvalid("centers is [n, atoms, 3], not %s" % (shape,))
        groups = _residues(residue_index, shape[1])
    sums, gsums, _ = _rmsf_sums(centers, populations, ref_frame, atom_indices, groups,
                                chunk_frames, device)
    return np.sqrt(gsums if per_residue else sums)


def bfactors_from_rmsfs(residue_index, rmsfs):
    """Every atom gets its residue's value (the reference's ``_bfactors_from_rmsfs``
    with residues given per atom): float64 ``[atoms]``."""
    res = np.asarray(residue_index)
    rmsfs = np.asarray(rmsfs, dtype=np.float64)
    if res.ndim != 1 or not np.issubdtype(res.dtype, np.integer):
        raise exception.DataInvalid("residue_index is a 1-D integer array.")
    _, first, inverse = np.unique(res, return_index=True, return_inverse=True)
    if rmsfs.shape != (first.size,):
        raise exception.DataInvalid(
            "rmsfs has shape %s for %d residues" % (rmsfs.shape, first.size))
    rank = np.argsort(np.argsort(first))
    return rmsfs[rank[inverse]]


def last_timing():
    """Milliseconds between device events of the last call: its uploads, its kernels,
    its downloads (ek_rmsf_last_timing)."""
    return _timing.copy()


def _check(rc):
    if rc == _lib.EK_ENOMEM:
        msg = _lib.load().ek_last_error().decode("utf-8", "replace")
        raise exception.InsufficientResourceError(msg)
    _lib.check(rc)
