"""A brute-force numpy model of the dye-labelling contract: float32
alignment in the contract's order, float64 distances, the reference's chunking, and bins
by the edge rule ``edge_k <= d < edge_{k+1}``.  It takes every square root and looks at
every pair: nothing of the device's thresholds on squared distances is in here.

The edge rule is not np.histogram called again: tests/golden/make_dyes_golden.py checks
that the two agree on every recorded case, so that the rule is what the reference does.
"""
import numpy as np

ONE_CHUNK_PAIRS = 5e7
CHUNK = 2048
F32 = np.float32


def align(dye, M, t):
    """p_j = ((x M[0][j] + y M[1][j]) + z M[2][j]) + t[j], float32, one rounding each"""
    d, M, t = np.asarray(dye, F32), np.asarray(M, F32), np.asarray(t, F32)
    out = np.empty((len(d), 3), dtype=F32)
    for j in range(3):
        out[:, j] = ((d[:, 0] * M[0, j] + d[:, 1] * M[1, j]) + d[:, 2] * M[2, j]) + t[j]
    return out


def norm_vec(v):
    return v / np.sqrt(np.einsum('...j,...j->...', v, v))[..., None]


def rot_mat(frame_xyz, backbone):
    """M [3, 3], t [3] of one frame, float32 (the reference's expressions)"""
    x = np.asarray(frame_xyz, F32)
    n, ca, c = (x[i] for i in backbone)
    normed = norm_vec(np.cross(norm_vec(ca - n), norm_vec(ca - c)))
    ca_vec = norm_vec(ca - ((n + c) / F32(2.)))
    theta = np.pi / 6.
    cb = ca + (F32(np.sin(theta) * 0.153) * ca_vec) + (F32(np.cos(theta) * 0.153) * normed)
    z = norm_vec(cb - ca)
    xv = norm_vec(np.cross(norm_vec(n - ca), z))
    yv = norm_vec(np.cross(z, xv))
    return np.array([xv, yv, z]), ca


def distances(a, b):
    """float64 [len(a), len(b)]: sqrt((dx dx + dy dy) + dz dz), d = a - b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def keep_mask(coords, frame_xyz, cutoff, rows=4096):
    """bool [n]: farther than the cutoff from every atom"""
    coords = np.asarray(coords)
    cutoff = np.asarray(cutoff, np.float64)
    keep = np.empty(len(coords), dtype=bool)
    for i in range(0, len(coords), rows):
        d = distances(frame_xyz, coords[i:i + rows])
        keep[i:i + rows] = np.all(d > cutoff[:, None], axis=0)
    return keep


def chunk_hist(d, bin_width):
    """counts int64 [nbins_c] of one chunk's distances by the edge rule"""
    d = np.asarray(d, np.float64).reshape(-1)
    nbins = int(d.max() / bin_width) + 2
    step = (nbins * bin_width) / nbins
    edges = np.arange(nbins + 1, dtype=np.float64) * step
    k = np.searchsorted(edges, d, side="right") - 1       # edges[k] <= d < edges[k + 1]
    assert k.min() >= 0 and k.max() < nbins, "a distance beyond the last edge"
    return np.bincount(k, minlength=nbins).astype(np.int64)


def chunks(coords1, coords2):
    """the (small, part of big) pairs of clouds the reference histograms one by one"""
    if len(coords1) * len(coords2) <= ONE_CHUNK_PAIRS:
        return [(coords1, coords2)]
    big, small = (coords1, coords2) if len(coords1) > len(coords2) else (coords2, coords1)
    return [(small, big[i:i + CHUNK]) for i in range(0, len(big), CHUNK)]


def pair_counts(coords1, coords2, bin_width, rows=1024):
    """counts int64 [nbins], and every chunk's nbins_c"""
    total, per_chunk = np.zeros(0, dtype=np.int64), []
    for a, b in chunks(coords1, coords2):
        # (a chunk's maximum first, then its histogram in slabs: the pairs of a chunk can
        # be 5e7 doubles, and the bins depend on the chunk's maximum alone)
        dmax = max(distances(a[i:i + rows], b).max() for i in range(0, len(a), rows))
        nbins = int(dmax / bin_width) + 2
        step = (nbins * bin_width) / nbins
        edges = np.arange(nbins + 1, dtype=np.float64) * step
        counts = np.zeros(nbins, dtype=np.int64)
        for i in range(0, len(a), rows):
            d = distances(a[i:i + rows], b).reshape(-1)
            k = np.searchsorted(edges, d, side="right") - 1
            assert k.min() >= 0 and k.max() < nbins
            counts += np.bincount(k, minlength=nbins)
        per_chunk.append(nbins)
        if nbins > len(total):
            total = np.concatenate([total, np.zeros(nbins - len(total), dtype=np.int64)])
        total[:nbins] += counts
    return total, per_chunk


def int_norm_hist(xs, ys):
    return ys / np.sum(ys * (xs[1:] - xs[:-1]))


def pair_distribution(coords1, coords2, bin_width):
    counts, _ = pair_counts(coords1, coords2, bin_width)
    edges = np.linspace(0, len(counts) * bin_width, len(counts) + 1)
    return int_norm_hist(edges, counts), edges


def frame_distribution(frame_xyz, cutoff, dye1, dye2, backbones, bin_width):
    """-> probs, edges, kept index sets of the four placements, counts of the two pairs"""
    placed, kept = [], []
    for dye in (dye1, dye2):
        for bb in backbones:
            M, t = rot_mat(frame_xyz, bb)
            p = align(dye, M, t)
            k = keep_mask(p, frame_xyz, cutoff)
            placed.append(p[k])
            kept.append(np.flatnonzero(k))
    pairs = [(placed[0], placed[3]), (placed[1], placed[2])]
    counts = [pair_counts(a, b, bin_width)[0] for a, b in pairs]
    probs, edges = [], []
    for c in counts:
        e = np.linspace(0, len(c) * bin_width, len(c) + 1)
        probs.append(int_norm_hist(e, c))
        edges.append(e)
    n = max(len(p) for p in probs)
    merged = sum(0.5 * np.concatenate([p, np.zeros(n - len(p))]) for p in probs)
    return merged, edges[int(np.argmax([len(p) for p in probs]))], kept, counts


def peptide(rng, residues, spacing=0.38):
    """A synthetic chain of N, CA, C, O, CB per residue along a noisy helix-free walk:
    -> xyz float32 [atoms, 3], atom names, residue numbers, radii (nm)"""
    names, seqs, xyz, radii = [], [], [], []
    pos = np.zeros(3)
    direction = np.array([1.0, 0.0, 0.0])
    vdw = {"N": 0.155, "CA": 0.17, "C": 0.17, "O": 0.152, "CB": 0.17}
    for r in range(residues):
        direction = direction + 0.6 * rng.randn(3)
        direction /= np.linalg.norm(direction)
        pos = pos + spacing * direction
        side = np.cross(direction, rng.randn(3))
        side /= np.linalg.norm(side)
        up = np.cross(direction, side)
        local = {"N": -0.12 * direction + 0.05 * side, "CA": 0 * side,
                 "C": 0.13 * direction + 0.06 * side, "O": 0.15 * direction + 0.17 * side,
                 "CB": -0.02 * direction - 0.08 * side + 0.12 * up}
        for a in ("N", "CA", "C", "O", "CB"):
            names.append(a)
            seqs.append(r + 1)
            xyz.append(pos + local[a] + 0.01 * rng.randn(3))
            radii.append(vdw[a])
    return (np.array(xyz, dtype=np.float32), np.array(names), np.array(seqs),
            np.array(radii, dtype=np.float64))


def ball(rng, n, radius, centre=(0, 0, 0)):
    """n points uniform in a ball, float32"""
    v = rng.randn(n, 3)
    v /= np.linalg.norm(v, axis=1)[:, None]
    return (np.asarray(centre) + v * (radius * rng.rand(n, 1) ** (1 / 3.))).astype(np.float32)


def chunk_clouds(seed, n1, n2):
    """Two clouds above the reference's threshold; the far points sit in the last chunk of
    the larger cloud only (the second on a tie), so that the chunks' numbers of bins
    differ.  The golden generator and the GPU test build the same clouds from the seed."""
    rng = np.random.RandomState(seed)
    a, b = ball(rng, n1, 1.0), ball(rng, n2, 1.5, centre=(2.0, 0.5, 0.0))
    big = a if n1 > n2 else b
    big[-3:] += np.float32(4.0)
    return a, b


def touch_cloud(seed, n, radius, centre):
    return ball(np.random.RandomState(seed), n, radius, centre=centre)
