"""A plain numpy restatement of the pocket-detection contract, written
from its description: what tests/test_pockets_host.py pins to the reference's recorded
results and tests/test_gpu_pockets.py compares the device with.

  grid      per axis n = ceil((max - min) / spacing), the subtraction and the quotient in
            float32; cell i at float64(min) + i * spacing; flat index (ix * ny + iy) * nz + iz
  touches   for some atom (dx*dx + dy*dy) + dz*dz < cutoff * cutoff in float64
  ranks     seven directions; +1 for a cell that does not touch and has a touching cell
            before it and one after it on the line; the diagonal lines that start on the
            edge shared by their three start faces, at z >= 1, are left out
  pockets   18-connected components of rank >= min_rank, labelled by smallest flat index;
            those of more than min_cluster_size cells, by size (largest first), then label
"""
import numpy as np

DIAGONALS = [(1, 1), (-1, 1), (-1, -1), (1, -1)]    # (sx, sy) of (sx, sy, 1)
RADII = {"H": 0.120, "C": 0.170, "N": 0.155, "O": 0.152}    # nm, float64 as the reference's


def radii_of(elements):
    return np.array([RADII[str(e)] for e in elements], dtype=np.float64)


def grid_of(xyz_frame, spacing):
    """origin float32 [3], dims [3] of the grid over xyz_frame [atoms, 3] float32"""
    assert xyz_frame.dtype == np.float32
    lo, hi = xyz_frame.min(axis=0), xyz_frame.max(axis=0)
    n = np.ceil((hi - lo) / np.float32(spacing))
    return lo, n.astype(np.int64)


def axes_of(origin, dims, spacing):
    return [np.float64(origin[k]) + np.arange(dims[k], dtype=np.float64) * spacing
            for k in range(3)]


def touches(xyz_frame, cutoff, spacing, origin=None, dims=None):
    """bool [nx, ny, nz]; every atom against every cell"""
    if origin is None:
        origin, dims = grid_of(xyz_frame, spacing)
    gx, gy, gz = axes_of(origin, dims, spacing)
    out = np.zeros(tuple(dims), dtype=bool)
    if out.size == 0:
        return out
    for p, c in zip(xyz_frame.astype(np.float64), np.asarray(cutoff, dtype=np.float64)):
        dx, dy, dz = gx - p[0], gy - p[1], gz - p[2]
        d2 = ((dx * dx)[:, None, None] + (dy * dy)[None, :, None]) + (dz * dz)[None, None, :]
        out |= d2 < c * c
    return out


def _between_axis(T, axis):
    """cells with a touching cell before and one after them along an axis"""
    before = np.logical_or.accumulate(T, axis=axis)
    after = np.flip(np.logical_or.accumulate(np.flip(T, axis), axis=axis), axis)
    return before & after & ~T


def _between_diagonal(T, quirk=True):
    """the same along (1, 1, 1)"""
    nx, ny, nz = T.shape
    before, after = np.zeros_like(T), np.zeros_like(T)
    for z in range(1, nz):
        before[1:, 1:, z] = (T[:, :, z - 1] | before[:, :, z - 1])[:-1, :-1]
    for z in range(nz - 2, -1, -1):
        after[:-1, :-1, z] = (T[:, :, z + 1] | after[:, :, z + 1])[1:, 1:]
    out = before & after & ~T
    if quirk:
        # lines whose first cell is (0, 0, z >= 1): the cells (t, t, z + t)
        x, y, z = np.ogrid[:nx, :ny, :nz]
        out &= ~((x == y) & (z > y))
    return out


def ranks(T, quirk=True):
    """uint8 [nx, ny, nz]"""
    T = np.asarray(T, dtype=bool)
    r = np.zeros(T.shape, dtype=np.uint8)
    if T.size == 0:
        return r
    for axis in range(3):
        r += _between_axis(T, axis)
    for sx, sy in DIAGONALS:
        view = (slice(None, None, sx), slice(None, None, sy), slice(None))
        r[view] += _between_diagonal(T[view], quirk)
    return r


def labels(mask):
    """int64 [nx, ny, nz]: the smallest flat index of every cell's 18-connected
    component of the mask, -1 outside"""
    mask = np.asarray(mask, dtype=bool)
    n = mask.size
    lab = np.where(mask, np.arange(n).reshape(mask.shape), n)
    if n == 0:
        return lab
    shifts = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
              if 1 <= abs(a) + abs(b) + abs(c) <= 2]
    assert len(shifts) == 18
    while True:
        pad = np.pad(lab, 1, constant_values=n)
        new = lab.copy()
        for a, b, c in shifts:
            nb = pad[1 + a:1 + a + mask.shape[0], 1 + b:1 + b + mask.shape[1],
                     1 + c:1 + c + mask.shape[2]]
            new = np.minimum(new, nb)
        new = np.where(mask, new, n)
        flat = np.append(new.ravel(), n)
        new = flat[new]                 # the label's own label
        if np.array_equal(new, lab):
            break
        lab = new
    return np.where(mask, lab, -1)


def pockets_of_labels(flat, lab, min_cluster_size=0):
    """flat indices (ascending) and their labels -> (cells, ids): the cells of the pockets
    of more than min_cluster_size cells, pocket after pocket, and the pockets' numbers"""
    uniq, sizes = np.unique(lab, return_counts=True)
    order = sorted(range(len(uniq)), key=lambda i: (-sizes[i], uniq[i]))
    cells, ids = [], []
    for i in order:
        if sizes[i] > min_cluster_size:
            members = flat[lab == uniq[i]]
            ids.append(np.full(len(members), len(ids), dtype=np.int64))
            cells.append(members)
    if not cells:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(cells), np.concatenate(ids)


def coordinates(flat, origin, dims, spacing):
    """float64 [n, 3] of flat indices"""
    flat = np.asarray(flat, dtype=np.int64)
    idx = np.stack(np.unravel_index(flat, tuple(int(d) for d in dims)), axis=1) \
        if flat.size else np.zeros((0, 3), dtype=np.int64)
    return np.asarray(origin, dtype=np.float32).astype(np.float64)[None, :] + idx * float(spacing)


def frame_pockets(xyz_frame, radii, spacing, probe, min_rank, min_cluster_size=0):
    """one frame, start to end -> dict(origin, dims, touches, ranks, flat, labels, cells,
    ids): flat/labels = every pocket cell in flat order with its component's label; cells/
    ids = the flat indices of the kept pockets in their order, and the pockets' numbers"""
    origin, dims = grid_of(xyz_frame, spacing)
    out = dict(origin=origin, dims=dims)
    if np.any(dims == 0):
        e = np.zeros(0, dtype=np.int64)
        out.update(touches=np.zeros(tuple(dims), bool), ranks=np.zeros(tuple(dims), np.uint8),
                   flat=e, labels=e, cells=e, ids=e)
        return out
    T = touches(xyz_frame, probe + np.asarray(radii, dtype=np.float64), spacing, origin, dims)
    R = ranks(T)
    out.update(touches=T, ranks=R)
    out.update(pockets_of_ranks(R, min_rank, min_cluster_size))
    return out


def pockets_of_ranks(R, min_rank, min_cluster_size=0):
    """dict(flat, labels, cells, ids) as frame_pockets gives them, from a grid of ranks"""
    mask = R >= min_rank
    flat = np.flatnonzero(mask)
    lab = labels(mask).ravel()[flat]
    cells, ids = pockets_of_labels(flat, lab, min_cluster_size)
    return dict(flat=flat, labels=lab, cells=cells, ids=ids)
