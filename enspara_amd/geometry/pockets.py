"""LIGSITE pocket detection on the device (the reference's enspara/geometry/
pockets.py; csrc/ek_pockets.hip).

A grid of cubic cells is laid over a frame.  Cells within ``probe_radius +
radius`` of an atom touch the protein; every other cell is ranked by how many of
seven scans through it (the three axes, the four space diagonals) meet protein on
both sides; the cells of rank ``>= min_rank`` are the pocket cells, and
contiguous ones form a pocket.  The arithmetic is a contract, so
that results can be compared element for element:

* per axis ``n = ceil((max - min) / spacing)`` cells, the subtraction and the
  quotient in float32; the grid stops short of ``max``; no padding
* cell ``i`` of an axis lies at ``float64(min) + float64(i) * spacing``, the flat
  index of a cell is ``(ix * ny + iy) * nz + iz``
* a cell touches iff for some atom ``(dx*dx + dy*dy) + dz*dz < cutoff * cutoff``
  in float64, ``d = cell - float64(x)``, ``cutoff = probe_radius + radius``
* along each of (1,0,0), (0,1,0), (0,0,1), (1,1,1), (-1,1,1), (-1,-1,1), (1,-1,1)
  a cell that does not touch and lies strictly between its line's first and last
  touching cell gains one rank
* a diagonal line (sx, sy, 1) whose first cell has x and y on their start faces
  (0 if s > 0, else n - 1) and z >= 1 is not scanned: the reference enumerates a
  diagonal's lines from three faces of the grid and misses the edge they share.
  This is reproduced, and there is no switch for it.
* pockets are the components of the pocket cells under 18-connectivity (face and
  edge neighbours: the reference's single linkage at 1.5 spacings), labelled by
  their smallest flat index; those of more than ``min_cluster_size`` cells are
  numbered from 0 by size, largest first, ties by the smaller label; the cells of
  a pocket are in flat-index order.

Where this differs from the reference, on purpose: there is no mdtraj here, so
the functions take coordinate arrays (float32, nm) and radii (nm; float64 values
such as ``ATOMIC_RADII`` holds reproduce the reference's cutoffs) instead of
trajectory objects and return arrays; a frame whose atoms are collinear or
coplanar along an axis (``n == 0`` there) has no cells and no pockets, where the
reference raises; equal-sized pockets have a fixed order, where the reference's
comes from an unstable sort.  The input is checked (``DataInvalid``): finite
coordinates, ``grid_spacing > 0`` and finite, ``probe_radius + radius > 0`` and
finite, an integer ``min_rank``, at most ``MAX_AXIS`` cells along an axis and
``MAX_CELLS`` in a frame (so that flat indices fit int32).
"""
import collections
import ctypes as C

import numpy as np

from .. import _lib, exception
from .sasa import ATOMIC_RADII  # noqa: F401  (radii in nm by element symbol)

__all__ = ["create_grid", "determine_touches_protein", "rank_cells", "label_cells",
           "get_pocket_cells", "cluster_pocket_cells", "get_pockets", "pocket_volumes",
           "FramePockets", "MAX_AXIS", "MAX_CELLS", "MAX_CHUNK_FRAMES", "last_timing"]

# POCK_MAX_AXIS, POCK_MAX_CELLS, POCK_MAX_FRAMES of csrc/ek_pockets.hip
MAX_AXIS = 2048
MAX_CELLS = 1 << 26
MAX_CHUNK_FRAMES = 32768

# the 9 of the 18 face and edge neighbours with a larger flat index
_FORWARD = np.array([(0, 0, 1), (0, 1, -1), (0, 1, 0), (0, 1, 1), (1, -1, 0), (1, 0, -1),
                     (1, 0, 0), (1, 0, 1), (1, 1, 0)])

FramePockets = collections.namedtuple("FramePockets", "cells pocket_ids origin shape")
FramePockets.__doc__ = """The pockets of one frame: ``cells`` float64 [n, 3] (nm, the
largest pocket first), ``pocket_ids`` int [n] (0, 1, ..), the grid's ``origin`` float32 [3]
and ``shape`` (nx, ny, nz)."""

_timing = np.zeros(4)


def _spacing(grid_spacing):
    try:
        s = float(grid_spacing)
    except (TypeError, ValueError):
        raise exception.DataInvalid("grid_spacing is a number, not %r" % (grid_spacing,))
    if not (s > 0 and np.isfinite(s)):
        raise exception.DataInvalid("grid_spacing = %r must be positive and finite." % (s,))
    return s


def _coordinates(xyz, ndim):
    xyz = np.asarray(xyz)
    if xyz.ndim != ndim or xyz.shape[-1] != 3 or xyz.shape[-2] < 1:
        raise exception.DataInvalid(
            "xyz is %s, not %s" % ("[frames, atoms, 3]" if ndim == 3 else "[atoms, 3]",
                                   xyz.shape))
    if xyz.dtype != np.float32:
        raise exception.DataInvalid("xyz is float32 (nm), not %s" % xyz.dtype)
    if not np.all(np.isfinite(xyz)):
        raise exception.DataInvalid("Coordinates must be finite.")
    return np.ascontiguousarray(xyz)


def _cutoffs(radii, probe_radius, atoms):
    radii = np.asarray(radii)
    if radii.shape != (atoms,):
        raise exception.DataInvalid("radii has shape %s for %d atoms" % (radii.shape, atoms))
    try:
        cutoff = float(probe_radius) + radii.astype(np.float64)
    except (TypeError, ValueError):
        raise exception.DataInvalid("probe_radius and radii are numbers.")
    if not np.all((cutoff > 0) & np.isfinite(cutoff)):
        raise exception.DataInvalid("probe_radius + radius must be positive and finite for "
                                    "every atom.")
    return np.ascontiguousarray(cutoff)


def _min_rank(min_rank):
    if isinstance(min_rank, bool) or not isinstance(min_rank, (int, np.integer)):
        raise exception.DataInvalid("min_rank is an integer, not %r" % (min_rank,))
    if not -2**31 <= min_rank < 2**31:
        raise exception.DataInvalid("min_rank = %d does not fit 32 bits" % min_rank)
    return int(min_rank)


def _grids(xyz, spacing):
    """origin [frames, 3] float32 and dims [frames, 3] int32 of xyz [frames, atoms, 3]"""
    byaxis = np.ascontiguousarray(xyz.transpose(0, 2, 1))   # (extrema over a contiguous axis)
    lo, hi = byaxis.min(axis=2), byaxis.max(axis=2)
    with np.errstate(over="ignore"):
        n = np.ceil((hi - lo) / np.float32(spacing))        # float32 throughout
    if not np.all(n <= MAX_AXIS):       # (an overflow to inf fails this too)
        raise exception.DataInvalid(
            "A frame spans more than %d cells of %g nm along an axis." % (MAX_AXIS, spacing))
    dims = n.astype(np.int32)
    if dims.size and dims.astype(np.int64).prod(axis=1).max() > MAX_CELLS:
        raise exception.DataInvalid("A frame's grid has more than %d cells." % MAX_CELLS)
    return np.ascontiguousarray(lo, dtype=np.float32), np.ascontiguousarray(dims)


def _dense(a, what, dtype=None):
    a = np.asarray(a)
    if a.ndim != 3:
        raise exception.DataInvalid("%s is a 3-D grid, not %s" % (what, a.shape))
    if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.integer):
        raise exception.DataInvalid("%s holds booleans, not %s" % (what, a.dtype))
    if max(a.shape) > MAX_AXIS or a.size > MAX_CELLS:
        raise exception.DataInvalid(
            "%s has shape %s: at most %d cells along an axis and %d in all"
            % (what, a.shape, MAX_AXIS, MAX_CELLS))
    return np.ascontiguousarray(a != 0).view(np.uint8)


def create_grid(xyz_frame, grid_spacing, padding=0):
    """The coordinates of the cells of the grid over one frame.

    Parameters
    ----------
    xyz_frame : np.ndarray, shape=(atoms, 3), float32
        Coordinates in nm.
    grid_spacing : float
        The edge of a cell in nm.
    padding : int, default=0
        Cells added on either side of every axis.

    Returns
    -------
    grid : np.ndarray, shape=(n_x, n_y, n_z, 3), float64
        ``grid[ix, iy, iz]`` = the coordinates of that cell.
    """
    xyz = _coordinates(xyz_frame, 2)
    s = _spacing(grid_spacing)
    if isinstance(padding, bool) or not isinstance(padding, (int, np.integer)) or padding < 0:
        raise exception.DataInvalid("padding is a non-negative integer, not %r" % (padding,))
    origin, dims = _grids(xyz[None], s)
    dims = dims[0].astype(np.int64) + 2 * int(padding)
    if dims.max() > MAX_AXIS or dims.prod() > MAX_CELLS:
        raise exception.DataInvalid("The padded grid has shape %s: at most %d cells along an "
                                    "axis and %d in all" % (tuple(dims), MAX_AXIS, MAX_CELLS))
    lo = origin[0] - np.float32(s * padding) if padding else origin[0]
    axes = [np.float64(lo[k]) + np.arange(dims[k], dtype=np.float64) * s for k in range(3)]
    grid = np.empty(tuple(dims) + (3,), dtype=np.float64)
    grid[..., 0] = axes[0][:, None, None]
    grid[..., 1] = axes[1][None, :, None]
    grid[..., 2] = axes[2][None, None, :]
    return grid


def determine_touches_protein(xyz_frame, radii, grid_spacing, probe_radius, device=0):
    """Which cells of the frame's grid lie within ``probe_radius + radius`` of an
    atom: bool ``[n_x, n_y, n_z]`` (the touch kernel alone)."""
    xyz = _coordinates(xyz_frame, 2)
    s = _spacing(grid_spacing)
    cutoff = _cutoffs(radii, probe_radius, len(xyz))
    origin, dims = _grids(xyz[None], s)
    out = np.zeros(tuple(dims[0]), dtype=np.uint8)
    if out.size:
        L = _lib.load()
        _check(L.ek_pockets_touches(int(device), _lib.f32p(xyz), len(xyz), _lib.f64p(cutoff), s,
                                    _lib.f32p(origin), _lib.i32p(dims), _lib.u8p(out)))
    return out.view(np.bool_)


def rank_cells(touches, device=0):
    """The rank (0 .. 7) of every cell of a grid of touches: uint8, the shape of
    ``touches`` (the line-extent and rank kernels alone)."""
    t = _dense(touches, "touches")
    out = np.zeros(t.shape, dtype=np.uint8)
    if out.size:
        dims = np.array(t.shape, dtype=np.int32)
        _check(_lib.load().ek_pockets_ranks(int(device), _lib.u8p(t), _lib.i32p(dims),
                                            _lib.u8p(out)))
    return out


def label_cells(mask, device=0):
    """The components of a mask under 18-connectivity: int32, the shape of
    ``mask``, every cell of the mask labelled with the smallest flat index of its
    component and -1 outside (the labelling kernels alone)."""
    m = _dense(mask, "mask")
    out = np.full(m.shape, -1, dtype=np.int32)
    if out.size:
        dims = np.array(m.shape, dtype=np.int32)
        _check(_lib.load().ek_pockets_labels(int(device), _lib.u8p(m), _lib.i32p(dims),
                                             _lib.i32p(out)))
    return out


def _run(xyz, radii, grid_spacing, probe_radius, min_rank, chunk_frames, device):
    """-> origin, dims, counts [frames], cells [total], labels [total] of the device run"""
    global _timing
    xyz = _coordinates(xyz, 3)
    s = _spacing(grid_spacing)
    frames, atoms = xyz.shape[:2]
    cutoff = _cutoffs(radii, probe_radius, atoms)
    min_rank = _min_rank(min_rank)
    if chunk_frames is None:
        chunk_frames = 0
    elif (isinstance(chunk_frames, bool) or not isinstance(chunk_frames, (int, np.integer))
          or not 1 <= chunk_frames <= MAX_CHUNK_FRAMES):
        raise exception.DataInvalid(
            "chunk_frames = %r is not in [1, %d]" % (chunk_frames, MAX_CHUNK_FRAMES))
    origin, dims = _grids(xyz, s)
    L = _lib.load()
    counts = np.zeros(frames, dtype=np.int64)
    h = C.c_void_p()
    _check(L.ek_pockets_open(int(device), atoms, _lib.f64p(cutoff), s, min_rank, C.byref(h)))
    try:
        _check(L.ek_pockets_run(h, _lib.f32p(xyz), frames, _lib.f32p(origin), _lib.i32p(dims),
                                int(chunk_frames)))
        if frames:
            _check(L.ek_pockets_counts(h, frames, _lib.i64p(counts)))
        total = int(counts.sum())
        cells = np.zeros(total, dtype=np.int32)
        labels = np.zeros(total, dtype=np.int32)
        _check(L.ek_pockets_fetch(h, _lib.i32p(cells), _lib.i32p(labels)))
        timing = np.zeros(4)
        _check(L.ek_pockets_last_timing(h, _lib.f64p(timing)))
        _timing = timing
    finally:
        L.ek_pockets_close(h)
    return s, origin, dims, counts, cells, labels


def _cell_coordinates(flat, origin, dims, spacing):
    """float64 [n, 3] of flat indices in a frame's grid"""
    flat = flat.astype(np.int64)
    idx = np.stack([flat // (int(dims[1]) * int(dims[2])), (flat // int(dims[2])) % int(dims[1]),
                    flat % int(dims[2])], axis=1) if flat.size else np.zeros((0, 3), np.int64)
    return origin.astype(np.float64)[None, :] + idx.astype(np.float64) * spacing


def get_pocket_cells(xyz_frame, radii, grid_spacing=0.1, probe_radius=0.07, min_rank=3,
                     device=0):
    """The pocket cells of one frame.

    Parameters
    ----------
    xyz_frame : np.ndarray, shape=(atoms, 3), float32
        Coordinates in nm.
    radii : array, shape=(atoms,)
        van der Waals radii in nm.
    grid_spacing : float, default=0.1
        The edge of a cell in nm.
    probe_radius : float, default=0.07
        Cells within this distance plus an atom's radius of the atom are protein.
    min_rank : int, default=3
        The rank from which a cell is part of a pocket.

    Returns
    -------
    pocket_cells : np.ndarray, shape=(n, 3), float64
        The coordinates of the pocket cells, in flat-index order.
    """
    xyz = _coordinates(xyz_frame, 2)
    s, origin, dims, _, cells, _ = _run(xyz[None], radii, grid_spacing, probe_radius, min_rank,
                                        None, device)
    return _cell_coordinates(cells, origin[0], dims[0], s)


def _components(n, a, b):
    """labels [n]: the smallest member of each component of the graph with edges a[i] --
    b[i] (host numpy: minimum over neighbours, then pointer jumping, until nothing moves)"""
    labels = np.arange(n, dtype=np.int64)
    while True:
        new = labels.copy()
        np.minimum.at(new, a, labels[b])
        np.minimum.at(new, b, labels[a])
        new = new[new]
        if np.array_equal(new, labels):
            return labels
        labels = new


def _number_pockets(labels, min_cluster_size):
    """-> (order, ids): the entries that belong to a pocket of more than min_cluster_size
    cells, pocket after pocket (largest first, ties by smaller label, a stable sort within),
    and the pockets' numbers"""
    uniq, inverse, sizes = np.unique(labels, return_inverse=True, return_counts=True)
    rank = np.lexsort((uniq, -sizes))           # pockets in their final order
    number = np.full(len(uniq), -1, dtype=np.int64)
    kept = rank[sizes[rank] > min_cluster_size]
    number[kept] = np.arange(len(kept))
    ids = number[inverse]
    order = np.flatnonzero(ids >= 0)
    order = order[np.argsort(ids[order], kind="stable")]
    return order, ids[order]


def cluster_pocket_cells(pocket_cells, grid_spacing=0.1, min_cluster_size=0):
    """Group pocket cells into contiguous pockets (host numpy; the reference's helper
    for the cells of one frame).

    The cells are snapped to the lattice of ``grid_spacing`` they lie on, and cells that
    are face or edge neighbours there are joined (the reference's single linkage at 1.5
    spacings).

    Returns
    -------
    sorted_cells : np.ndarray, shape=(n, 3)
        The cells of the pockets of more than ``min_cluster_size`` cells, the largest
        pocket first (equal sizes: the one with the earliest cell first), within a
        pocket in the order given.
    pocket_ids : np.ndarray, shape=(n,), int
        The pocket (0, 1, ..) of each of them.
    """
    cells = np.asarray(pocket_cells, dtype=np.float64)
    if cells.size == 0:
        return np.array([]), np.array([])
    if cells.ndim != 2 or cells.shape[1] != 3 or not np.all(np.isfinite(cells)):
        raise exception.DataInvalid("pocket_cells is a finite [n, 3] array, not %s"
                                    % (cells.shape,))
    s = _spacing(grid_spacing)
    lattice = np.rint((cells - cells.min(axis=0)) / s)
    if lattice.max() >= 2**20:
        raise exception.DataInvalid("pocket_cells span more than 2^20 spacings.")
    lattice = lattice.astype(np.int64) + 1      # (room for the -1 of a neighbour)
    key = (lattice[:, 0] << 42) | (lattice[:, 1] << 21) | lattice[:, 2]
    by_key = np.argsort(key, kind="stable")
    sorted_key = key[by_key]
    a, b = [], []
    for off in _FORWARD:
        want = key + ((int(off[0]) << 42) + (int(off[1]) << 21) + int(off[2]))
        at = np.minimum(np.searchsorted(sorted_key, want), len(key) - 1)
        hit = np.flatnonzero(sorted_key[at] == want)
        a.append(hit)
        b.append(by_key[at[hit]])
    labels = _components(len(cells), np.concatenate(a), np.concatenate(b))
    order, ids = _number_pockets(labels, min_cluster_size)
    return cells[order], ids.astype(int)


def get_pockets(xyz, radii, grid_spacing=0.1, probe_radius=0.14, min_rank=5,
                min_cluster_size=0, chunk_frames=None, device=0):
    """The pockets of every frame of a trajectory, on the device.

    Parameters
    ----------
    xyz : np.ndarray, shape=(frames, atoms, 3), float32
        Coordinates in nm.
    radii : array, shape=(atoms,)
        van der Waals radii in nm.
    grid_spacing : float, default=0.1
        The edge of a cell in nm.
    probe_radius : float, default=0.14
        Cells within this distance plus an atom's radius of the atom are protein.
    min_rank : int, default=5
        The rank from which a cell is part of a pocket.
    min_cluster_size : int, default=0
        Pockets have more cells than this.
    chunk_frames : int, default=None
        Frames of one upload; by default what fits the device.
    device : int
        The HIP device.

    Returns
    -------
    pockets : list of FramePockets, one per frame
        ``cells`` float64 [n, 3], the largest pocket first; ``pocket_ids`` int [n];
        ``origin`` float32 [3] and ``shape`` (n_x, n_y, n_z) of the frame's grid.
    """
    s, origin, dims, counts, cells, labels = _run(xyz, radii, grid_spacing, probe_radius,
                                                  min_rank, chunk_frames, device)
    out, end = [], np.cumsum(counts)
    for f in range(len(counts)):
        c, lab = cells[end[f] - counts[f]:end[f]], labels[end[f] - counts[f]:end[f]]
        order, ids = _number_pockets(lab, min_cluster_size)
        out.append(FramePockets(_cell_coordinates(c[order], origin[f], dims[f], s),
                                ids.astype(int), origin[f].copy(),
                                tuple(int(d) for d in dims[f])))
    return out


def pocket_volumes(result, grid_spacing):
    """Per frame of a ``get_pockets`` result, the volume of every pocket in nm^3:
    its number of cells times ``grid_spacing ** 3``."""
    s = _spacing(grid_spacing)
    return [np.bincount(r.pocket_ids).astype(np.float64) * s ** 3 if len(r.pocket_ids)
            else np.zeros(0) for r in result]


def last_timing():
    """Milliseconds between device events of the last ``get_pockets`` or
    ``get_pocket_cells``: its uploads, touch kernels, line-extent and rank kernels,
    label and compaction kernels (ek_pockets_last_timing)."""
    return _timing.copy()


def _check(rc):
    if rc == _lib.EK_ENOMEM:
        msg = _lib.load().ek_last_error().decode("utf-8", "replace")
        raise exception.InsufficientResourceError(msg)
    _lib.check(rc)
