"""Structure families for the RMSD kernels: frames (not hand-made 3x3 matrices,
those are tests/_qcp_cases.py) whose inner-product matrix against each other is
degenerate in every way a structure can make it -- rank one, rank two, det S < 0,
equal singular values, exactly equal traces -- or lies on either side of the
range of q = sum S_ij^2 the float32 certificate accepts.  numpy only, seeded.
Shared by tests/test_structure_families_host.py (oracle against a float64 Kabsch,
device header compiled with g++ against the oracle) and
tests/test_gpu_structure_families.py (the kernels against the oracle)."""
import zlib

import numpy as np

from enspara_amd import synth

NOISE_NM = 0.05
ATOM_COUNTS = (2, 3, 4, 7, 33)      # every remainder mod 4; 33: three groups of 16
FIXED_ATOMS = {"cube": 8, "two_atom_quantised": 2}
SCALES = {"scale_tiny": 1e-15, "scale_small": 1e-5, "scale_large": 1e4,
          "scale_huge": 1e9}
FAMILIES = ["generic", "collinear_exact", "collinear_rotated", "near_collinear",
            "planar", "mirror", "rotated_copies", "identical", "cube",
            "two_atom_quantised", "scale_tiny", "scale_small", "scale_large",
            "scale_huge", "far_offset"]


def family_cases():
    """every (family, A): A over ATOM_COUNTS, except where the family fixes it"""
    out = []
    for name in FAMILIES:
        for A in ((FIXED_ATOMS[name],) if name in FIXED_ATOMS else ATOM_COUNTS):
            out.append((name, A))
    return out


def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return synth._quat_to_rot(q)


def _rotate(rng, xyz):
    return np.einsum("nij,naj->nai", _rotations(rng, len(xyz)), xyz)


def _noisy_templates(rng, n, A, seed, noise=NOISE_NM):
    tmpl = synth.templates(4, A, seed)
    xyz = tmpl[rng.integers(0, 4, size=n)]
    if noise:
        xyz = xyz + rng.normal(scale=noise, size=xyz.shape)
    return xyz


def _far(rng, n):
    """a translation of +-10^4 along every axis"""
    return 1e4 * np.where(rng.random((n, 1, 3)) < 0.5, -1.0, 1.0)


def structure_family(name, n, A, seed=0):
    """float32 [n, A, 3] of the family named (all finite)"""
    if name not in FAMILIES:
        raise ValueError("unknown family %r" % (name,))
    if name in FIXED_ATOMS and A != FIXED_ATOMS[name]:
        raise ValueError("%s has %d atoms" % (name, FIXED_ATOMS[name]))
    seed = zlib.crc32(name.encode()) % 10**6 + 1000 * seed + A
    rng = np.random.default_rng(seed)
    near = rng.uniform(-5.0, 5.0, size=(n, 1, 3))
    if name == "cube":
        v = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)],
                     dtype=np.float64) - 0.5
        xyz = v[None] + rng.normal(scale=1e-3, size=(n, 8, 3))
        return (_rotate(rng, xyz) + near).astype(np.float32)
    if name == "two_atom_quantised":
        # float32 spacing at 10^4 is 2^-10: the two atoms land on a coarse grid
        xyz = _rotate(rng, _noisy_templates(rng, n, 2, seed))
        return (xyz + _far(rng, n)).astype(np.float32)
    if name == "rotated_copies":
        xyz = _noisy_templates(rng, n, A, seed, noise=0.0)
        return (_rotate(rng, xyz) + near).astype(np.float32)
    xyz = _noisy_templates(rng, n, A, seed)
    if name == "collinear_exact":
        # one coordinate axis per frame, coordinates k / 1024, offsets k / 64: the
        # other two centred coordinates are exactly zero, S has exactly rank one
        along = np.round(xyz[:, :, 0] * 1024.0) / 1024.0
        out = np.zeros((n, A, 3))
        out[np.arange(n), :, rng.integers(0, 3, size=n)] = along
        out += rng.integers(-320, 321, size=(n, 1, 3)) / 64.0
        return out.astype(np.float32)
    if name == "collinear_rotated":
        xyz[:, :, 1:] = 0.0
    elif name == "near_collinear":
        xyz[:, :, 1:] *= 1e-4
    elif name == "planar":
        xyz[:, :, 2] = 0.0
    elif name == "mirror":
        xyz[1::2, :, 0] *= -1.0
    elif name == "identical":
        one = (_rotate(rng, xyz[:1]) + near[:1]).astype(np.float32)
        return np.ascontiguousarray(np.repeat(one, n, axis=0))
    xyz = _rotate(rng, xyz)
    if name in SCALES:
        return ((xyz + near) * SCALES[name]).astype(np.float32)
    if name == "far_offset":
        return (xyz + _far(rng, n)).astype(np.float32)
    return (xyz + near).astype(np.float32)


def kabsch_msd(X, y):
    """float64 Kabsch: every frame of X [n, A, 3] superposed on y [A, 3] -- centre,
    SVD of the 3x3 inner-product matrix, third singular value signed like its
    determinant -> (msd [n], scale (Gx + Gy) / A [n])"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    A = X.shape[1]
    cx = X - X.mean(axis=1, keepdims=True)
    cy = y - y.mean(axis=0, keepdims=True)
    G = (cx * cx).sum(axis=(1, 2)) + (cy * cy).sum()
    H = np.einsum("nai,aj->nij", cx, cy)
    sv = np.linalg.svd(H, compute_uv=False)
    # the sign of det H from the matrix itself; an exactly singular H has s3 = 0
    with np.errstate(over="ignore", under="ignore"):
        top = np.abs(H).max(axis=(1, 2))
        det = np.linalg.det(H / np.where(top > 0, top, 1.0)[:, None, None])
    lam = sv[:, 0] + sv[:, 1] + np.where(det < 0, -sv[:, 2], sv[:, 2])
    return np.maximum(G - 2.0 * lam, 0.0) / A, G / A
