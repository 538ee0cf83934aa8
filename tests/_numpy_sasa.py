"""Brute-force Shrake-Rupley solvent-accessible surface area in numpy float32, the
expected values of tests/test_gpu_sasa.py.  It follows the contract of DESIGN.md 4h
operation for operation and tries every j != i: no neighbour list, no culling.

    R_i     = float32(radii_i) + float32(probe)
    p       = (R_i * s_k) + x_i                       per component
    blocked   iff for some j != i: (dx*dx + dy*dy) + dz*dz < R_j * R_j,  d = p - x_j
    count_i = the points that are not blocked
    area_i  = ((c * R_i) * R_i) * float32(count_i),   c = float32(4 pi / n)
    group   = 0.0f + the areas of its atoms in the order listed

numpy rounds every float32 operation on its own (it fuses nothing), which is the
contract.
"""
import numpy as np

F32 = np.float32


def sphere_points(n):
    """the golden-section spiral in float64, cast to float32 [n, 3]"""
    i = np.arange(n, dtype=np.float64)
    y = i * (2.0 / n) - 1.0 + 1.0 / n
    r = np.sqrt(1.0 - y * y)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([np.cos(phi) * r, y, np.sin(phi) * r], axis=1).astype(F32)


def counts(xyz, radii, probe, n, j_block=64):
    """accessible points [frames, atoms] int32; xyz [frames, atoms, 3] float32"""
    xyz = np.asarray(xyz)
    assert xyz.dtype == F32 and xyz.ndim == 3
    s = sphere_points(n)
    R = np.asarray(radii).astype(F32) + F32(probe)
    R2 = R * R
    A = xyz.shape[1]
    out = np.zeros(xyz.shape[:2], dtype=np.int32)
    atom = np.arange(A)
    for f, X in enumerate(xyz):
        p = (R[:, None, None] * s[None, :, :]) + X[:, None, :]       # [A, n, 3]
        blocked = np.zeros((A, n), dtype=bool)
        for j0 in range(0, A, j_block):
            Xj = X[j0:j0 + j_block]
            dx = p[:, :, None, 0] - Xj[None, None, :, 0]
            dy = p[:, :, None, 1] - Xj[None, None, :, 1]
            dz = p[:, :, None, 2] - Xj[None, None, :, 2]
            hit = ((dx * dx + dy * dy) + dz * dz) < R2[None, None, j0:j0 + j_block]
            hit &= (atom[:, None] != atom[None, j0:j0 + j_block])[:, None, :]
            blocked |= hit.any(axis=2)
        out[f] = n - blocked.sum(axis=1)
    return out


def areas(count, radii, probe, n):
    """[frames, atoms] float32 from the counts"""
    R = np.asarray(radii).astype(F32) + F32(probe)
    c = F32(4.0 * np.pi / n)
    return ((c * R) * R)[None, :] * np.asarray(count).astype(F32)


def group_sums(area, groups):
    """[frames, groups] float32: from 0, the atoms in the order listed"""
    area = np.asarray(area, dtype=F32)
    out = np.zeros((area.shape[0], len(groups)), dtype=F32)
    for g, ids in enumerate(groups):
        for a in ids:
            out[:, g] = out[:, g] + area[:, a]
    return out


def blob(rng, frames, atoms, side=None):
    """uniform random atoms at protein density (170 atoms in a 1.3 nm cube), radii
    drawn from H / C / N / O -> (xyz [frames, atoms, 3] float32, radii float32)"""
    if side is None:
        side = 1.3 * (atoms / 170.0) ** (1.0 / 3.0)
    xyz = (rng.rand(frames, atoms, 3) * side).astype(F32)
    radii = rng.choice(np.array([0.120, 0.170, 0.155, 0.152], dtype=F32), size=atoms)
    return xyz, radii
