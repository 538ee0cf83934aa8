"""A plain numpy restatement of the contracts of enspara_amd.cards and
enspara_amd.geometry.rotamer (reference enspara/cards/disorder.py, cards.py and
geometry/rotamer.py), the expected values of tests/test_gpu_cards.py and
tests/test_gpu_rotamer.py.  tests/test_cards_host.py holds it equal to the real
reference's outputs in tests/golden/cards_golden.npz.

Nothing here uses intervals or scans: transitions come from np.diff, the order /
disorder decision is the reference's likelihood-ratio expression evaluated per
span, the rotamer state machine walks the frames one by one (all columns of a
frame at once).
"""
import numpy as np

import _numpy_mi as nm

PHI, PSI, CHI = [0, 180, 360], [0, 160, 360], [0, 120, 240, 360]
ON_GATES = [0, 15, 105, 120, 165, 180, 195, 240, 255, 345, 359.5]


# ---- transitions, statistics, times ------------------------------------------------------
def transition_times(col):
    col = np.asarray(col)
    return np.where(col[1:] != col[:-1])[0]


def stats(X):
    """[frames, F] codes -> int64 [F, 4] = (n, first, last, s2); no transition: (0, -1, -1, 0)"""
    X = np.asarray(X)
    out = np.zeros((X.shape[1], 4), dtype=np.int64)
    for j in range(X.shape[1]):
        tt = transition_times(X[:, j]).astype(np.int64)
        if len(tt) == 0:
            out[j] = (0, -1, -1, 0)
            continue
        w = np.concatenate([tt[:1], np.diff(tt)])
        out[j] = (len(tt), tt[0], tt[-1], int((w * (w + 1) // 2).sum()))
    return out


def ord_disord_times(tt):
    """(ord_time, n_ord, disord_time, n_disord) of one list of transition times"""
    tt = np.asarray(tt, dtype=np.int64)
    if len(tt) == 0:
        return 0.0, 0.0, 0.0, 0.0
    if len(tt) == 1:
        return float(tt[0]) * (float(tt[0]) + 1.0) / 2, float(tt[0]), 0.0, 0.0
    gaps = np.diff(tt)
    w = np.concatenate([tt[:1], gaps]).astype(np.float64)
    return ((w * (w + 1.0) / 2).sum() / w.sum(), float(tt[-1]),
            float(gaps.sum()) / len(gaps), float(tt[-1] - tt[0]))


def mean_times(trajs):
    """-> (mean ordered, mean disordered) [F]: per-trajectory times weighted by length / total"""
    F = trajs[0].shape[1]
    o = np.zeros((len(trajs), F))
    d = np.zeros((len(trajs), F))
    for i, X in enumerate(trajs):
        for j in range(F):
            o[i, j], _, d[i, j], _ = ord_disord_times(transition_times(X[:, j]))
    wt = np.array([len(X) for X in trajs])
    wt = wt / np.sum(wt)
    return (np.array([(o[:, j] * wt).sum() for j in range(F)]),
            np.array([(d[:, j] * wt).sum() for j in range(F)]))


def likelihood(ord_time, disord_time, span):
    """the reference's expression (create_disorder_traj), span an int64"""
    with np.errstate(all="ignore"):
        return ord_time / disord_time * np.exp(-span * (1. / disord_time - 1. / ord_time))


def disorder_codes(X, ord_t, dis_t):
    """uint8 [frames, F]: 1 between neighbouring transitions whose likelihood ratio >= 3"""
    X = np.asarray(X)
    D = np.zeros(X.shape, dtype=np.uint8)
    for j in range(X.shape[1]):
        tt = transition_times(X[:, j])
        for a, b in zip(tt[:-1], tt[1:]):
            if likelihood(ord_t[j], dis_t[j], np.int64(b - a)) >= 3.0:
                D[a:b, j] = 1
    return D


def disorder_codes_from_interval(X, lo, hi):
    """the device's contract: 1 where a <= t < b neighbours and lo <= b - a <= hi"""
    X = np.asarray(X)
    D = np.zeros(X.shape, dtype=np.uint8)
    for j in range(X.shape[1]):
        tt = transition_times(X[:, j])
        for a, b in zip(tt[:-1], tt[1:]):
            if lo[j] <= b - a <= hi[j]:
                D[a:b, j] = 1
    return D


def cards_counts(trajs, Ds, n):
    S = np.concatenate(trajs)
    D = np.concatenate(Ds)
    return (nm.joint_counts(S, None, n), nm.joint_counts(D, None, 2),
            nm.joint_counts(S, D, n, 2), nm.joint_counts(D, S, 2, n))


def cards_matrices(trajs, n_states):
    """-> (four normalised matrices, four bounds on the device's deviation, Ds, counts)"""
    n_states = np.asarray(n_states)
    n = int(n_states.max())
    Ds = [disorder_codes(X, *mean_times(trajs)) for X in trajs]
    jcs = cards_counts(trajs, Ds, n)
    two = np.full(len(n_states), 2)
    caps = [(n_states, n_states), (two, two), (n_states, two), (two, n_states)]
    mats, bounds = [], []
    for jc, (a, b) in zip(jcs, caps):
        mi, S = nm.mutual_information(jc)
        cap = np.log(np.minimum(a[:, None], b[None, :]))
        mats.append(mi / cap)
        # (the quotient rounds once more on each side: half an ulp of at most S / cap each)
        bounds.append((nm.mi_bound(jc.shape[2], jc.shape[3], S) + 2 * nm.U * S) / cap)
    return mats, bounds, Ds, jcs


def dd_in_float64(ref_dd):
    """The reference's D-D matrix is divided by log(2) in float32 (np.log of its int16 state
    numbers); this is the same matrix divided by the float64 log(2), to two roundings."""
    return ref_dd * np.float64(np.log(np.int16(2))) / np.log(2.0)


# ---- rotamer states ------------------------------------------------------------------------------
def gates(hb, width):
    """get_gates of every basin -> (lower [nb], upper [nb]) float64"""
    hb = np.asarray(hb, dtype=np.float64)
    lower = np.where(hb[:-1] == 0, 360.0, hb[:-1]) - width
    upper = np.where(hb[1:] == 360, 0.0, hb[1:]) + width
    return lower, upper


def shifted(angles, shift):
    """a - shift, + 360 where negative: in float32, as the device and psi_rotamers do (in
    float64 for float64 angles, the expectation of the tests that start from coordinates)"""
    angles = np.asarray(angles)
    dt = np.float64 if angles.dtype == np.float64 else np.float32
    a = angles.astype(dt) - dt(shift)
    a[a < 0] += dt(360)
    return a


def rotamer_states(angles, kind, boundaries, shifts, width):
    """angles [frames, n] -> uint8 [frames, n]; column j of kind kind[j]"""
    angles = np.asarray(angles)
    T, n = angles.shape
    kind = np.asarray(kind)
    nb = np.array([len(boundaries[k]) - 1 for k in kind])
    hb = np.full((n, 9), np.inf)
    lower = np.zeros((n, 8))
    upper = np.zeros((n, 8))
    a = np.zeros((T, n), dtype=np.float64)
    for j in range(n):
        b = np.asarray(boundaries[kind[j]], dtype=np.float64)
        hb[j, :len(b)] = b
        lower[j, :nb[j]], upper[j, :nb[j]] = gates(b, width)
        a[:, j] = shifted(angles[:, j], shifts[kind[j]])      # (exactly widened)
    cols = np.arange(n)
    out = np.zeros((T, n), dtype=np.uint8)
    cur = np.zeros(n, dtype=np.int64)
    for t in range(T):
        # the basin the angle lies in: hb[i] <= a < hb[i + 1]; 360 counts as the last basin
        d = np.minimum((a[t][:, None] >= hb[:, 1:]).sum(axis=1), nb - 1)
        if t == 0:
            cur = d
        else:
            lo, up = lower[cols, cur], upper[cols, cur]
            inside = (lo <= a[t]) & (a[t] <= up)
            between = (up <= a[t]) & (a[t] <= lo)
            tr = np.where(up < lo, between, np.where(up > lo, ~inside, False))
            cur = np.where(tr, d, cur)
        out[t] = cur
    return out


# ---- dihedral angles -------------------------------------------------------------------------
def dihedral_deg(xyz, quads, dtype=np.float64):
    """atan2((b1 . c1) |b2|, c1 . c2) in `dtype`, degrees, < 0 -> + 360, > 359.5 -> 359.5"""
    x = np.asarray(xyz).astype(dtype)
    q = np.asarray(quads)
    p0, p1, p2, p3 = (x[:, q[:, k], :] for k in range(4))
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    c1, c2 = np.cross(b2, b3), np.cross(b1, b2)
    y = (b1 * c1).sum(axis=-1) * np.sqrt((b2 * b2).sum(axis=-1))
    xx = (c1 * c2).sum(axis=-1)
    deg = (np.arctan2(y, xx) * dtype(180.0 / np.pi)).astype(dtype)
    deg = np.where(deg < 0, deg + dtype(360), deg)
    return np.where(deg > 359.5, dtype(359.5), deg).astype(dtype)


def place_dihedrals(rng, target_deg, offset=5.0):
    """four atoms per target dihedral: bonds of 0.15, bond angles 100-125 degrees, a random
    rigid motion and an offset up to `offset` -> float32 [len(target), 4, 3]"""
    phi = np.deg2rad(np.asarray(target_deg, dtype=np.float64))
    m = len(phi)
    th1 = np.deg2rad(rng.uniform(100, 125, m))
    th2 = np.deg2rad(rng.uniform(100, 125, m))
    L = 0.15
    p1 = np.zeros((m, 3))
    p2 = np.stack([np.full(m, L), np.zeros(m), np.zeros(m)], axis=1)
    p0 = p1 + L * np.stack([np.cos(th1), np.sin(th1), np.zeros(m)], axis=1)
    # p3: bond angle th2 at p2, turned about the p1 - p2 axis by the dihedral
    p3 = p2 + L * np.stack([-np.cos(th2), np.sin(th2) * np.cos(phi),
                            np.sin(th2) * np.sin(phi)], axis=1)
    pts = np.stack([p0, p1, p2, p3], axis=1)
    # a random rotation (QR of a Gaussian matrix, made proper) and an offset per dihedral
    Q = np.linalg.qr(rng.normal(size=(m, 3, 3)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    pts = np.einsum("mab,mkb->mka", Q, pts) + rng.uniform(-offset, offset, (m, 1, 3))
    return pts.astype(np.float32)


def gate_distance(deg, kind, boundaries, shifts, width):
    """per angle (float64, [frames, n]) the distance in degrees to the nearest gate, boundary
    or the 359.5 clip of its column's kind, measured on the shifted angle"""
    deg = np.asarray(deg, dtype=np.float64)
    out = np.full(deg.shape, np.inf)
    for j in range(deg.shape[1]):
        k = kind[j]
        a = deg[:, j] - shifts[k]
        a = np.where(a < 0, a + 360, a)
        lo, up = gates(boundaries[k], width)
        marks = np.concatenate([np.asarray(boundaries[k], dtype=np.float64), lo, up])
        out[:, j] = np.abs(a[:, None] - marks[None, :]).min(axis=1)
        # the clip, the wrap of the raw angle and the sign change of the shift
        out[:, j] = np.minimum(out[:, j], np.abs(deg[:, j] - 359.5))
        out[:, j] = np.minimum(out[:, j], np.minimum(deg[:, j], 360 - deg[:, j]))
        out[:, j] = np.minimum(out[:, j], np.abs(deg[:, j] - shifts[k]))
    return out


def safe_trajectory(rng, frames, kind, boundaries, shifts, width, step=25.0, margin=0.01):
    """Coordinates whose dihedrals keep `margin` degrees from every gate, boundary and clip:
    dihedral j of kind kind[j] has the atoms 4 j .. 4 j + 3 and follows a random walk of
    steps `step` (a number, or an array [frames, 1]); where
    the angle computed in float64 from the float32 coordinates comes too close, the target is
    moved and the atoms placed again.  -> (xyz float32 [frames, 4 n, 3], quads [n, 4],
    angles float64 [frames, n])"""
    n = len(kind)
    target = np.mod(np.cumsum(rng.normal(0, step, (frames, n)), axis=0)
                    + rng.uniform(0, 360, n)[None, :], 360)
    quads = np.arange(4 * n).reshape(n, 4)
    xyz = place_dihedrals(rng, target.ravel()).reshape(frames, 4 * n, 3)
    for _ in range(50):
        deg = dihedral_deg(xyz, quads)
        bad = gate_distance(deg, kind, boundaries, shifts, width) < margin
        if not bad.any():
            break
        target[bad] = np.mod(target[bad] + 0.7, 360)
        xyz.reshape(frames, n, 4, 3)[bad] = place_dihedrals(rng, target[bad])
    deg = dihedral_deg(xyz, quads)
    assert gate_distance(deg, kind, boundaries, shifts, width).min() >= margin
    return xyz, quads, deg
