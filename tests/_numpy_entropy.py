"""A numpy restatement of the reference's enspara/info_theory/entropy.py and of the
arithmetic of enspara/apps/compute-shannon-entropy.py, the expected values of
tests/test_gpu_entropy.py, and the bound on what the device may differ by.  Nothing here
calls the device.

Every function that returns a sum of terms also returns S = the sum of the terms'
magnitudes, the scale of the bound: KL terms have both signs and cancel, so the error of
a row is relative to sum |t_j|, not to |sum t_j|.
"""
import warnings

import numpy as np

U = 2.0 ** -52
K = 4


def kl_terms(P, Q):
    """t = P log(P / Q) with NaN -> 0 (reference entropy.py:242-245), in nats"""
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", category=RuntimeWarning)
        t = P * np.log(P / Q)
    t[np.isnan(t)] = 0
    return t


def kl_divergence(P, Q, base=2):
    """-> (divergence per row (a scalar for 1-D input), S) in units of `base`"""
    t = kl_terms(P, Q)
    return t.sum(axis=-1) / np.log(base), np.abs(t).sum(axis=-1) / np.log(base)


def js_divergence(p, q):
    """-> (js, S_p, S_q), bits"""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    m = 0.5 * (p + q)
    a, Sa = kl_divergence(p, m)
    b, Sb = kl_divergence(q, m)
    return 0.5 * a + 0.5 * b, Sa, Sb


def shannon_rows(p, normalize=True):
    """-> (H per row, S per row), nats; elements <= 0 contribute 0"""
    p = np.asarray(p, dtype=np.float64)
    if normalize:
        p = np.copy(p) / np.sum(p, axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        t = np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0)
    return -t.sum(axis=-1), np.abs(t).sum(axis=-1)


def shannon_entropy(p, normalize=True):
    H, S = shannon_rows(np.asarray(p, dtype=np.float64).reshape(1, -1), normalize)
    return H[0], S[0]


def kl_bound(c, S, k=K):
    """|dev - numpy| <= (c + k) 2^-52 S for a row of c terms whose magnitudes sum to S
    (S already divided by ln(base), like the values).  k = 4:
    * P / Q is one correctly rounded division on both sides: the same bits.
    * each side's log is within one ulp of the true logarithm, so the two are at most 2
      ulps apart, and the multiply by P rounds once on each side, half an ulp each: a
      term differs by at most 3 * 2^-52 |t|.                                        (3)
    * c terms take c - 1 adds in either order; an add rounds by at most half an ulp of a
      partial sum, which is at most S in magnitude: (c - 1) / 2 * 2^-52 S on each side,
      (c - 1) * 2^-52 S between them.                                               (c - 1)
    * the division by ln(base) rounds once on each side, half an ulp each.           (1)
    That is c + 3; one more covers the second-order products of these.  The Shannon sum
    has the same terms (x log x: one log, one multiply) and no division: c + 2 <= c + 4.
    A row that is +inf has S = inf and is compared exactly, not by this bound."""
    return (c + k) * U * S


def js_bound(c, Sa, Sb):
    """0.5 * KL_p + 0.5 * KL_q: the halvings are exact, each KL within kl_bound, and the
    final add rounds once on each side (half an ulp of at most 0.5 (Sa + Sb) each):
    0.5 (c + 4) U (Sa + Sb) + U 0.5 (Sa + Sb) = 0.5 (c + 5) U (Sa + Sb)."""
    return 0.5 * (c + K + 1) * U * (Sa + Sb)


def shannon_norm_bound(c, S):
    """The row-normalised form, for rows that are not negative anywhere: the two row sums
    s differ by at most (c - 1) 2^-52 s (c - 1 adds of positive numbers, half an ulp a
    side each), x = p / s rounds once more on each side: x differs by d <= c 2^-52
    relative.  d/dx (x log x) = log x + 1, so a term moves by at most (|x log x| + x) d,
    and over the row, where the x sum to 1, by (S + 1) c 2^-52.  On top of kl_bound."""
    return kl_bound(c, S) + c * U * (S + 1.0)


# ---- Q from assignments ------------------------------------------------------------------
def dense_counts(assignments, n_states, lag_time=1):
    C = np.zeros((n_states, n_states), dtype=np.int64)
    for a in assignments:
        a = np.asarray(a)
        if len(a) > lag_time:
            np.add.at(C, (a[:-lag_time], a[lag_time:]), 1)
    return C


def default_prior(assignments):
    return 1 / np.sum([len(a) - 1 for a in assignments])


def Q_from_assignments(assignments, n_states=None, lag_time=1, builder="normalize",
                       prior_counts=None):
    """builders.normalize (rows over their sums) or builders.transpose (C + C.T first)
    of the dense counts + prior (reference entropy.py:16-41)"""
    if n_states is None:
        n_states = max(int(np.max(a)) for a in assignments) + 1
    if prior_counts is None:
        prior_counts = default_prior(assignments)
    C = dense_counts(assignments, n_states, lag_time) + prior_counts
    if builder == "transpose":
        C = C + C.T
    rs = C.sum(axis=1, keepdims=True)
    with np.errstate(all="ignore"):
        return np.where(rs > 0, C / np.where(rs > 0, rs, 1.0), 0.0)


def relative_entropy_per_state(P, Q, base=2.0):
    return kl_divergence(P, Q, base=base)


def relative_entropy_msm(P, Q, populations, state_subset=None, base=2.0):
    """the population-weighted sum of the per-state values on the subset"""
    if state_subset is None:
        state_subset = Ellipsis
    per, S = kl_divergence(P, Q, base=base)
    with np.errstate(invalid="ignore"):
        return np.sum(per[state_subset] * populations)


# ---- rotamer counts and entropies -------------------------------------------------------
def state_counts(trajs, n_max):
    """[F, n_max] int64: np.bincount per column, summed over the trajectories"""
    F = np.asarray(trajs[0]).reshape(len(trajs[0]), -1).shape[1]
    out = np.zeros((F, n_max), dtype=np.int64)
    for X in trajs:
        X = np.asarray(X).reshape(len(X), -1)
        for j in range(F):
            out[j] += np.bincount(X[:, j], minlength=n_max)[:n_max]
    return out


def dihedral_entropies(counts):
    """app :363-370: P_a = counts / counts.sum(-1), shannon_entropy of each row"""
    P_a = counts / counts.sum(axis=-1)[..., None]
    return shannon_rows(P_a, normalize=True)


def residue_entropies(H, n_states, residue_of, n_residues):
    """app :220-267, :310-319: sum per residue over the channel capacity sum(log n)"""
    H, n_states, residue_of = np.asarray(H), np.asarray(n_states), np.asarray(residue_of)
    total = np.array([H[residue_of == i].sum() for i in range(n_residues)])
    cap = np.array([np.log(n_states[residue_of == i]).sum() for i in range(n_residues)])
    with np.errstate(all="ignore"):
        return total / cap


# ---- inputs ------------------------------------------------------------------------------
def metastable_chain(rng, n, n_basins=3, leak=0.02):
    """a row-stochastic matrix of n states in n_basins basins that leak into each other,
    with some exact zeros"""
    T = rng.rand(n, n) * (rng.rand(n, n) < 0.6)
    basin = np.arange(n) * n_basins // n
    T = np.where(basin[:, None] == basin[None, :], T, T * leak)
    T[np.arange(n), (np.arange(n) + 1) % n] += 0.05    # a ring: every state is left and entered
    T[np.arange(n), np.arange(n)] += 0.5
    return T / T.sum(axis=1, keepdims=True)


def sample_chain(rng, T, n_trj, length):
    """assignments [n_trj, length] drawn from T"""
    cum = np.cumsum(T, axis=1)
    out = np.zeros((n_trj, length), dtype=np.int64)
    out[:, 0] = rng.randint(0, len(T), size=n_trj)
    for t in range(1, length):
        u = rng.rand(n_trj)
        out[:, t] = np.minimum((u[:, None] > cum[out[:, t - 1]]).sum(axis=1), len(T) - 1)
    return out


def random_rows(rng, rows, cols):
    """positive rows that sum to 1"""
    M = rng.rand(rows, cols) + 1e-3
    return M / M.sum(axis=1, keepdims=True)
