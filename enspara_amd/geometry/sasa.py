"""Shrake-Rupley solvent-accessible surface area on the device (what the
reference's enspara/info_theory/exposons.py takes from ``mdtraj.shrake_rupley``;
csrc/ek_sasa.hip).

Every atom's sphere of radius ``R_i = radius_i + probe`` carries the same
``n_sphere_points`` points; a point is accessible if it lies inside no other
atom's sphere, and the atom's area is its share of accessible points times
``4 pi R_i^2``.  The arithmetic is a contract, float32 with
nothing fused, so that the result can be checked bit for bit:

* ``R_i = float32(radii_i) + float32(probe)``
* ``p = (R_i * s_k) + x_i`` per component
* blocked iff for some ``j != i``: ``(dx*dx + dy*dy) + dz*dz < R_j * R_j``,
  ``d = p - x_j``
* ``area_i = ((c * R_i) * R_i) * float32(count_i)``, ``c = float32(4 pi / n)``
* a group sum starts from ``0.0f`` and adds the areas in the order listed.

Where this differs from mdtraj, on purpose: there is no topology reader (the
caller passes radii, ``radii_from_elements`` helps, and index lists), atoms
are grouped by any index lists rather than by residue, and the input is
checked: coordinates are finite and within ``MAX_COORD`` nm of the origin (the
bound the neighbour culling's margin is derived for), ``radius + probe`` lies
in ``(0, MAX_R]``, ``n_sphere_points`` in ``[1, MAX_POINTS]``, groups are not
empty and index existing atoms; else ``DataInvalid``.
"""
import ctypes as C

import numpy as np

from .. import _lib, exception

__all__ = ["shrake_rupley", "sphere_points", "ATOMIC_RADII", "radii_from_elements",
           "MAX_POINTS", "MAX_COORD", "MAX_R", "last_timing"]

# SASA_MAX_POINTS, SASA_MAX_COORD, SASA_MAX_R, SASA_MAX_FRAMES of csrc/ek_sasa.hip
MAX_POINTS = 4096
MAX_COORD = 128.0
MAX_R = 4.0
MAX_CHUNK_FRAMES = 32768

# van der Waals radii in nm (Bondi, J. Phys. Chem. 68, 1964; H from Rowland and
# Taylor, J. Phys. Chem. 100, 1996; metals and the rest as commonly tabulated)
ATOMIC_RADII = {
    "H": 0.120, "He": 0.140, "Li": 0.182, "Be": 0.153, "B": 0.192, "C": 0.170,
    "N": 0.155, "O": 0.152, "F": 0.147, "Ne": 0.154, "Na": 0.227, "Mg": 0.173,
    "Al": 0.184, "Si": 0.210, "P": 0.180, "S": 0.180, "Cl": 0.175, "Ar": 0.188,
    "K": 0.275, "Ca": 0.231, "Fe": 0.200, "Ni": 0.163, "Cu": 0.140, "Zn": 0.139,
    "Se": 0.190, "Br": 0.185, "I": 0.198,
}

_timing = np.zeros(3)


def radii_from_elements(symbols):
    """van der Waals radii (nm, float32) of a sequence of element symbols
    (any letter case); an unknown symbol is ``DataInvalid``."""
    out = np.empty(len(symbols), dtype=np.float32)
    for i, s in enumerate(symbols):
        key = str(s).strip().capitalize()
        if key not in ATOMIC_RADII:
            raise exception.DataInvalid("No van der Waals radius for element %r." % (s,))
        out[i] = ATOMIC_RADII[key]
    return out


def _n_points(n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise exception.DataInvalid("n_sphere_points is an integer, not %r" % (n,))
    if not 1 <= n <= MAX_POINTS:
        raise exception.DataInvalid(
            "n_sphere_points = %d is not in [1, %d]" % (n, MAX_POINTS))
    return int(n)


def sphere_points(n):
    """``n`` points on the unit sphere, float32 ``[n, 3]``: the golden-section
    spiral ``y_i = i (2 / n) - 1 + 1 / n``, ``r = sqrt(1 - y^2)``, ``phi = i pi
    (3 - sqrt 5)``, point ``(cos(phi) r, y, sin(phi) r)``, in float64 and then
    cast."""
    n = _n_points(n)
    i = np.arange(n, dtype=np.float64)
    y = i * (2.0 / n) - 1.0 + 1.0 / n
    r = np.sqrt(1.0 - y * y)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([np.cos(phi) * r, y, np.sin(phi) * r], axis=1).astype(np.float32)


def _groups(atom_groups, n_atoms):
    """index lists -> (offsets [groups + 1], atoms [total]) int32"""
    offsets, atoms = [0], []
    for g, ids in enumerate(atom_groups):
        ids = np.asarray(ids)
        if ids.ndim != 1 or ids.size == 0:
            raise exception.DataInvalid("Atom group %d is empty or not a 1-D list." % g)
        if not np.issubdtype(ids.dtype, np.integer):
            raise exception.DataInvalid("Atom group %d holds indices, not %s." % (g, ids.dtype))
        if ids.min() < 0 or ids.max() >= n_atoms:
            raise exception.DataInvalid(
                "Atom group %d indexes atoms %d .. %d; there are %d atoms."
                % (g, ids.min(), ids.max(), n_atoms))
        atoms.append(ids.astype(np.int32))
        offsets.append(offsets[-1] + ids.size)
    if not atoms:
        raise exception.DataInvalid("atom_groups is empty.")
    return np.asarray(offsets, dtype=np.int32), np.concatenate(atoms)


def shrake_rupley(xyz, radii, probe_radius=0.14, n_sphere_points=960, atom_groups=None,
                  return_counts=False, chunk_frames=None, device=0):
    """Solvent-accessible surface areas of every frame.

    Parameters
    ----------
    xyz : np.ndarray, shape=(frames, atoms, 3), float32
        Coordinates in nm.
    radii : array, shape=(atoms,)
        van der Waals radii in nm.
    probe_radius : float, default=0.14
        Radius of the solvent probe in nm.
    n_sphere_points : int, default=960
        Points per atom.
    atom_groups : list of index arrays, default=None
        Return the sum of the areas of each group's atoms, in the order they
        are listed, instead of the atoms' areas.
    return_counts : bool, default=False
        Also return the number of accessible points of every atom.
    chunk_frames : int, default=None
        Frames of one upload and launch; by default what fits the device.
    device : int
        The HIP device.

    Returns
    -------
    areas : np.ndarray, float32, shape=(frames, atoms) or (frames, groups), nm^2
    counts : np.ndarray, int32, shape=(frames, atoms)  (with ``return_counts``)
    """
    xyz = np.asarray(xyz)
    if xyz.ndim != 3 or xyz.shape[2] != 3 or xyz.shape[1] < 1:
        raise exception.DataInvalid(
            "xyz is [frames, atoms, 3], not %s" % (xyz.shape,))
    if xyz.dtype != np.float32:
        raise exception.DataInvalid("xyz is float32 (nm), not %s" % xyz.dtype)
    xyz = np.ascontiguousarray(xyz)
    frames, atoms = xyz.shape[:2]
    if xyz.size and not np.abs(xyz).max() <= MAX_COORD:     # (NaN fails the comparison)
        raise exception.DataInvalid(
            "Coordinates must be finite and within %g nm of the origin." % MAX_COORD)
    radii = np.asarray(radii)
    if radii.shape != (atoms,):
        raise exception.DataInvalid(
            "radii has shape %s for %d atoms" % (radii.shape, atoms))
    radii = radii.astype(np.float32)
    probe = np.float32(probe_radius)
    if not np.all(radii > 0):
        raise exception.DataInvalid("Atomic radii must be positive.")
    R = np.ascontiguousarray(radii + probe, dtype=np.float32)
    if not (np.isfinite(probe) and np.all(R > 0) and np.all(R <= MAX_R)):
        raise exception.DataInvalid(
            "radius + probe must lie in (0, %g] nm for every atom." % MAX_R)
    points = sphere_points(n_sphere_points)
    if chunk_frames is None:
        chunk_frames = 0
    elif not 1 <= chunk_frames <= MAX_CHUNK_FRAMES:
        raise exception.DataInvalid(
            "chunk_frames = %r is not in [1, %d]" % (chunk_frames, MAX_CHUNK_FRAMES))
    if atom_groups is None:
        n_groups, goff, gidx = 0, None, None
    else:
        goff, gidx = _groups(atom_groups, atoms)
        n_groups = len(goff) - 1

    L = _lib.load()
    counts = np.zeros((frames, atoms), dtype=np.int32) if return_counts else None
    areas = np.zeros((frames, atoms), dtype=np.float32) if atom_groups is None else None
    sums = None if atom_groups is None else np.zeros((frames, n_groups), dtype=np.float32)
    h = C.c_void_p()
    _check(L.ek_sasa_open(int(device), atoms, _lib.f32p(R), len(points), _lib.f32p(points),
                          n_groups, None if goff is None else _lib.i32p(goff),
                          None if gidx is None else _lib.i32p(gidx), C.byref(h)))
    try:
        _check(L.ek_sasa_run(h, _lib.f32p(xyz), frames, int(chunk_frames),
                             None if counts is None else _lib.i32p(counts),
                             None if areas is None else _lib.f32p(areas),
                             None if sums is None else _lib.f32p(sums)))
        _check(L.ek_sasa_last_timing(h, _lib.f64p(_timing)))
    finally:
        L.ek_sasa_close(h)
    out = areas if atom_groups is None else sums
    return (out, counts) if return_counts else out


def last_timing():
    """Milliseconds between device events of the last ``shrake_rupley``: its
    uploads, its count kernels, its group kernels (ek_sasa_last_timing)."""
    return _timing.copy()


def _check(rc):
    if rc == _lib.EK_ENOMEM:
        msg = _lib.load().ek_last_error().decode("utf-8", "replace")
        raise exception.InsufficientResourceError(msg)
    _lib.check(rc)
