"""Two numpy models behind the tests of geometry.rmsf (numpy only).

1. ``kabsch_superpose`` / ``rmsf_reference``: the float64 yardstick.  mdtraj is
   not installed where these tests run, so the reference's ``rmsf_calc`` cannot
   be run and no golden output of it exists: a float64 Kabsch superposition
   (centre on the selection, SVD of H, third singular vector signed like det H,
   as tests/_structure_cases.kabsch_msd does) stands in for it.
2. ``accumulate``: the summation contract of csrc/ek_rmsf.hip step 3 restated
   operation for operation (float64, nothing fused).

``frame_bound`` is the per-frame bound on |aligned_device - aligned_model| of
DESIGN.md 4o, computed from the model's values alone.
"""
import numpy as np

TILE = 32       # RMSF_TILE of csrc/ek_rmsf.hip
C_BOUND = 8.0   # the constant c of DESIGN.md 4o


def kabsch_superpose(xyz, ref, sel=None):
    """Every frame of xyz [n, A, 3] on ref [A, 3] over the atoms sel, in float64.

    -> dict: R [n, 3, 3] (aligned = R (x - cx) + cref), aligned [n, A, 3], msd [n]
    over the selection, G = Gx + Gy [n], GxGy [n], g = lambda_1 - lambda_2 [n] of
    the 4x4 key matrix (eigvalsh), r_max [n] = the largest distance of any atom from
    the selection's centroid."""
    X = np.asarray(xyz, dtype=np.float64)
    y = np.asarray(ref, dtype=np.float64)
    n, A = X.shape[:2]
    sel = np.arange(A) if sel is None else np.asarray(sel)
    cx = X[:, sel].mean(axis=1, keepdims=True)
    cy = y[sel].mean(axis=0, keepdims=True)
    xs, ys = X[:, sel] - cx, y[sel] - cy
    Gx, Gy = (xs * xs).sum(axis=(1, 2)), (ys * ys).sum()
    H = np.einsum("nai,aj->nij", xs, ys)        # H_ij = sum_a x_ai y_aj
    R = np.empty((n, 3, 3))
    lam = np.empty(n)
    g = np.empty(n)
    for f in range(n):
        top = np.abs(H[f]).max()
        Hn = H[f] / (top if top > 0 else 1.0)
        U, s, Vt = np.linalg.svd(Hn)
        d = 1.0 if np.linalg.det(Hn) >= 0 else -1.0
        D = np.diag([1.0, 1.0, d])
        R[f] = Vt.T @ D @ U.T                   # maximises tr(R H)
        lam[f] = (s[0] + s[1] + d * s[2]) * top
        S = Hn
        K = np.array([
            [S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
            [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
            [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], S[1, 1] - S[0, 0] - S[2, 2], S[1, 2] + S[2, 1]],
            [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], S[2, 2] - S[0, 0] - S[1, 1]]])
        ev = np.linalg.eigvalsh(K)
        g[f] = (ev[3] - ev[2]) * top
    centred = X - cx
    aligned = np.einsum("nij,naj->nai", R, centred) + cy
    msd = np.maximum(Gx + Gy - 2.0 * lam, 0.0) / len(sel)
    r_max = np.sqrt((centred * centred).sum(axis=2)).max(axis=1)
    return {"R": R, "aligned": aligned, "msd": msd, "G": Gx + Gy, "GxGy": Gx * Gy, "g": g,
            "r_max": r_max, "n_sel": len(sel)}


def frame_bound(model):
    """bound_f = c (n_sel + 2) 2^-24 sqrt(Gx Gy) / g r_max + 2^-23 max|aligned| (inf
    where g = 0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        turn = np.where(model["g"] > 0, np.sqrt(model["GxGy"]) / model["g"], np.inf)
    return (C_BOUND * (model["n_sel"] + 2) * 2.0 ** -24 * turn * model["r_max"] +
            2.0 ** -23 * np.abs(model["aligned"]).max(axis=(1, 2)))


# g / (Gx + Gy) of every frame of a degenerate family of tests/_structure_cases.py (24
# frames, frame 0 the reference) stays below this in the model: the largest is 4.6e-7,
# near_collinear at A = 4 (its y and z are 1e-4 of x, so s2 / s1 ~ 1e-8 .. 1e-7); the exactly
# collinear ones and every two-atom case are below 1e-15.  The well-conditioned families
# have at least 2e-3.
DEGENERATE_RATIO = 5e-7


def assert_bound_is_tight(model, bound):
    """a loose bound cannot stand in for a check: what the bound allows the ROTATION to
    be off by is at most 1e-3 of the structure's extent.  (The other term, 2^-23
    max|aligned|, is the float32 grid the output lies on -- 1.2e-3 nm for far_offset's
    coordinates at 1e4, whatever the structure's size -- and no check can ask less.)"""
    turn = bound - 2.0 ** -23 * np.abs(model["aligned"]).max(axis=(1, 2))
    assert np.all(turn <= 1e-3 * model["r_max"]), float((turn / model["r_max"]).max())


def groups_of(residue_index):
    """residues = the distinct values in order of first appearance -> list of atom
    index arrays (ascending inside each)"""
    residue_index = np.asarray(residue_index)
    order = []
    for v in residue_index.tolist():
        if v not in order:
            order.append(v)
    return [np.flatnonzero(residue_index == v) for v in order]


def rmsf_reference(centers, populations=None, ref_frame=0, sel=None, groups=None):
    """float64 throughout: sqrt(sum_f w_f d^2_fa) per atom, or per group
    sqrt(sum_f w_f mean_{a in group} d^2_fa).  The reference frame is not moved and
    deviates by exactly 0."""
    X = np.asarray(centers, dtype=np.float64)
    n = len(X)
    w = np.full(n, 1.0 / n) if populations is None else np.asarray(populations, dtype=np.float64)
    al = kabsch_superpose(X, X[ref_frame], sel)["aligned"]
    al[ref_frame] = X[ref_frame]
    d2 = ((al - X[ref_frame][None]) ** 2).sum(axis=2)           # [n, A]
    if groups is None:
        return np.sqrt((w[:, None] * d2).sum(axis=0))
    return np.sqrt(np.array([(w * d2[:, np.asarray(g)].mean(axis=1)).sum() for g in groups]))


def accumulate(aligned_f32, ref_f32, weights, groups=None, tile=TILE):
    """csrc/ek_rmsf.hip step 3: per atom and tile of frames acc = 0.0, then for every
    frame of the tile in order acc = acc + w_f * ((dx * dx + dy * dy) + dz * dz), d =
    float64(aligned) - float64(reference); the total starts at 0.0 and adds the tiles'
    partials in order; a group is 0.0 plus its atoms' totals in listed order, divided
    by their count.  -> (atom sums [A], group sums [groups] or None)"""
    al = np.asarray(aligned_f32)
    assert al.dtype == np.float32 and np.asarray(ref_f32).dtype == np.float32
    d = al.astype(np.float64) - np.asarray(ref_f32).astype(np.float64)[None]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    w = np.asarray(weights, dtype=np.float64)
    total = np.zeros(al.shape[1])
    for t0 in range(0, len(al), tile):
        acc = np.zeros(al.shape[1])
        for f in range(t0, min(t0 + tile, len(al))):
            acc = acc + w[f] * d2[f]
        total = total + acc
    if groups is None:
        return total, None
    out = np.empty(len(groups))
    for k, g in enumerate(groups):
        s = 0.0
        for a in np.asarray(g).tolist():
            s = s + total[a]
        out[k] = s / len(g)
    return total, out
