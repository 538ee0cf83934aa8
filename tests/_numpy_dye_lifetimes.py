"""The plain model of enspara_amd.geometry.dye_lifetimes and of the pair table of
enspara_amd.geometry.explicit_r0_calc, in numpy: the pair function in the
device's operation order (float64) and in np.longdouble, the decay CDF, and the samplers
``resolve``, ``static`` and ``isotropic``.  As in _numpy_kmc.py every sampler takes its
uniforms as ``uniform(stream, chain, index)``: ``PhiloxUniforms(seed)`` is the device's,
``RecordedUniforms`` replays the reference's generator.

tests/test_dye_lifetimes_host.py holds this model to the real reference's recorded outputs;
the GPU tests take every expected value from here.  Every sampler also returns, per chain,
how close a draw came to a value it was compared with: the smallest ``|u - cdf_k|`` over the
chain's decay draws, ``|coin - FE|`` for a static sample.  A device whose CDFs are within
half that margin of the model's makes the same decisions.

The bounds, device (float64, every operation rounded once, sqrt and exp within one ulp)
against the exact value of the same float64 inputs.  u = 2^-53; "k u" stands for a relative
(or, where said, absolute) error of k u to first order, the constants rounded up to absorb
the higher orders.
  r      c = centre_D - centre_A has 1 u a component; r2 = cx cx + cy cy + cz cz is a sum of
         three non-negative products: 2 + 1 + 2 = 5 u; the root halves that and adds 2 u:
         |r - r_exact| <= 5 u r (``R_REL``).
  k2     |D|, |A|: 3 u for the sum of squares, the root gives 3.5 u, say 4 u.  rvec has 1 u a
         component, |rvec| as r: 5 u.  A.D has the absolute error 3 u |A||D| (three products,
         two additions, Cauchy-Schwarz), its denominator 4 + 4 + 1 = 9 u and the division 1 u:
         cosT is within 13 u absolutely.  rvec.D and A.rvec carry rvec's rounding too: 4 u
         |rvec||D|, denominator 5 + 4 + 1 = 10 u, division 1 u: cosD, cosA within 15 u.  3 cosD
         cosA: 3 (15 + 15) u and two roundings of a value <= 3: 96 u.  k = cosT - that: 13 + 96
         u and the rounding of |k| <= 4: 113 u.  k2 = k k: 2 |k| 113 u + 16 u <= 920 u.
         |k2 - k2_exact| <= 1024 u (``K2_ABS``, absolute: the subtraction cancels).
  FE     FE = f(k2) = s k2 / (1 + s k2) with s = c6 / r^6.  f' = s / (1 + s k2)^2 falls in k2,
         so the error of k2 moves FE by at most s K2_ABS / (1 + s max(k2 - K2_ABS, 0))^2.  The
         rest is relative: r6 = r2 r2 r2 has 3 * 5 + 2 = 17 u, c6 k2 1 u: 18 u on the ratio
         r6 / R0^6, which moves FE = 1 / (1 + ratio) by FE (1 - FE) 18 u <= 4.5 u; the addition
         and the division add 2 u: |FE - FE_exact| <= that first term + 8 u (``fe_bound``).
  cdf    y = kRET dt = (1 / Td) dt s k2 has the absolute error A = (dt / Td) s K2_ABS from k2
         and 17 + 4 = 21 u relatively.  p_RET = 1 - exp(-y): exp(-y) (A + 21 u y) + 2 u + 1 u
         <= A + 11 u (y exp(-y) <= 1 / e).  Without renormalisation the entries are p_rad,
         p_rad + p_nonrad, and that + p_RET, over c3 = their sum + (1 - p_rad - p_nonrad -
         p_RET), in which p_RET's error cancels: c3 is within 6 u of 1.  So an entry is within
         A + 11 u + 10 u.  Renormalised, every p is divided by sum >= 1 whose error is A + 14
         u: within 2 A + 34 u.  Where the exact remainder is within its error of 0 the two
         sides may take different branches; the two forms differ there by the remainder
         itself.  |cdf - cdf_exact| <= 2 A + 48 u (``cdf_bound``), absolute.
These are derived from the operation count, not tuned to any output; the GPU test prints the
largest observed ratio to them."""
import numpy as np

from _numpy_kmc import PhiloxUniforms, RecordedUniforms, row_cdf, compressed, EmptyRow  # noqa: F401

DECAY, DONOR, ACCEPTOR, FRET_COIN = 5, 6, 7, 8
RADIATIVE, NON_RADIATIVE, ENERGY_TRANSFER, EXCITED = 0, 1, 2, 3
OUTCOMES = ("radiative", "non_radiative", "energy_transfer")

U = 2.0 ** -53
R_REL = 5 * U
K2_ABS = 1024 * U


def consts(dye_params, dt, n=1.333):
    """the per-problem constants as the host makes them: p_rad, p_nonrad, dt, c6, 1 / Td, 0"""
    J, Qd, Td = dye_params
    krad = Qd / Td
    k_non_rad = (1 / Td) - krad
    return np.array([1 - np.exp(-krad * dt), 1 - np.exp(-k_non_rad * dt), dt,
                     0.02108**6 * Qd * J / n**4, 1 / Td, 0.0])


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def pair(d, a, K, dtype=np.float64):
    """(k2, r, FE, cdf [..., 3]) of donor and acceptor conformations [..., 9] (broadcast), in
    the device's order of operations, in ``dtype``"""
    d, a, K = (np.asarray(x, dtype=np.float64).astype(dtype) for x in (d, a, K))
    p_rad, p_nonrad, dt, c6, inv_td = (K[i] for i in range(5))
    one, three = dtype(1), dtype(3)
    c = d[..., 0:3] - a[..., 0:3]
    r2 = _dot(c, c)
    v = d[..., 3:6] - a[..., 3:6]
    D, A = d[..., 6:9], a[..., 6:9]
    D, A, v = np.broadcast_arrays(D, A, v)
    nD, nA, nR = np.sqrt(_dot(D, D)), np.sqrt(_dot(A, A)), np.sqrt(_dot(v, v))
    cosT = _dot(A, D) / (nA * nD)
    cosD = _dot(v, D) / (nR * nD)
    cosA = _dot(A, v) / (nA * nR)
    k = cosT - three * cosD * cosA
    k2 = k * k
    r = np.sqrt(r2)
    r06 = c6 * k2
    r6 = r2 * r2 * r2
    FE = r06 / (r06 + r6)
    kret = inv_td * r06 / r6
    p_ret = one - np.exp(-kret * dt)
    p0 = p_rad + np.zeros_like(p_ret)
    p1 = p_nonrad + np.zeros_like(p_ret)
    p2 = p_ret
    p3 = one - p_rad - p_nonrad - p_ret
    neg = p3 < 0
    total = np.where(neg, p0 + p1 + p2 + dtype(0), one)
    p0, p1, p2 = (np.where(neg, p / total, p) for p in (p0, p1, p2))
    p3 = np.where(neg, dtype(0), p3)
    c1 = p0 + p1
    c2 = c1 + p2
    c3 = c2 + p3
    return k2, r, FE, np.stack([p0 / c3, c1 / c3, c2 / c3], axis=-1)


def pair_exact(d, a, K):
    """``pair`` in np.longdouble (2^-64 where the platform has the x87 format)"""
    return pair(d, a, K, dtype=np.longdouble)


def fe_bound(k2_exact, r_exact, K):
    s = np.asarray(K[3] / np.asarray(r_exact, dtype=np.float64) ** 6)
    k2 = np.maximum(np.asarray(k2_exact, dtype=np.float64) - K2_ABS, 0.0)
    return s * K2_ABS / (1 + s * k2) ** 2 + 8 * U


def cdf_bound(r_exact, K):
    s = np.asarray(K[3] / np.asarray(r_exact, dtype=np.float64) ** 6)
    return 2 * (K[2] * K[4]) * s * K2_ABS + 48 * U


def table(d_coords, a_coords, K, dtype=np.float64):
    """the pair function over every (donor state, acceptor state): [nd, na] each"""
    d = np.asarray(d_coords, dtype=np.float64)[:, None, :]
    a = np.asarray(a_coords, dtype=np.float64)[None, :, :]
    return pair(d, a, K, dtype=dtype)


def init_cdf(eqs):
    c = np.cumsum(np.asarray(eqs, dtype=np.float64))
    return c / c[-1]


def _initial(cdf, u):
    return int(min(np.searchsorted(cdf, u, side="right"), len(cdf) - 1))


def _hop(rows, s, u):
    if rows[s] is None:
        raise EmptyRow(s)
    cols, cdf = rows[s]
    return int(cols[np.searchsorted(cdf, u, side="right")])


class StillExcited(Exception):
    pass


def resolve(d_coords, d_T, d_eqs, a_coords, a_T, a_eqs, K, n_samples, uniform, first_chain=0,
            max_steps=1 << 20, block=64):
    """-> (steps int64 [n], outcomes int8 [n], donor trajectories, acceptor trajectories
    (lists of int64 arrays, steps + 1 long), margins [n])"""
    d_rows, a_rows = compressed(d_T), compressed(a_T)
    d_init, a_init = init_cdf(d_eqs), init_cdf(a_eqs)
    d_coords, a_coords = np.asarray(d_coords, dtype=np.float64), np.asarray(a_coords, np.float64)
    _, _, _, cdfs = table(d_coords, a_coords, K)
    steps, outcomes, margins = (np.zeros(n_samples, dtype=np.int64),
                                np.zeros(n_samples, dtype=np.int8), np.full(n_samples, np.inf))
    dtrajs, atrajs = [], []
    for j in range(n_samples):
        c = first_chain + j
        sd = _initial(d_init, float(uniform(DONOR, c, np.array(0))))
        sa = _initial(a_init, float(uniform(ACCEPTOR, c, np.array(0))))
        dtrj, atrj, t, ch = [sd], [sa], 0, EXCITED
        while ch == EXCITED:
            if t >= max_steps:
                raise StillExcited(c)
            if t % block == 0:          # the doubles of the next ``block`` steps
                idx = np.arange(t, t + block)
                ue, ud, ua = uniform(DECAY, c, idx), uniform(DONOR, c, idx + 1), \
                    uniform(ACCEPTOR, c, idx + 1)
            u = ue[t % block]
            cdf = cdfs[sd, sa]
            margins[j] = min(margins[j], np.abs(cdf - u).min())
            ch = int(np.searchsorted(cdf, u, side="right"))
            sd, sa = _hop(d_rows, sd, ud[t % block]), _hop(a_rows, sa, ua[t % block])
            dtrj.append(sd)
            atrj.append(sa)
            t += 1
        steps[j], outcomes[j] = t, ch
        dtrajs.append(np.array(dtrj, dtype=np.int64))
        atrajs.append(np.array(atrj, dtype=np.int64))
    return steps, outcomes, dtrajs, atrajs, margins


def static(d_coords, d_eqs, a_coords, a_eqs, K, n_samples, uniform, first_chain=0):
    """-> (acceptor flags bool [n], donor states, acceptor states, |coin - FE| [n])"""
    d_init, a_init = init_cdf(d_eqs), init_cdf(a_eqs)
    _, _, FE, _ = table(d_coords, a_coords, K)
    c = first_chain + np.arange(n_samples)
    zero = np.zeros(n_samples, dtype=np.int64)
    ds = np.minimum(np.searchsorted(d_init, uniform(DONOR, c, zero), side="right"),
                    len(d_init) - 1)
    as_ = np.minimum(np.searchsorted(a_init, uniform(ACCEPTOR, c, zero), side="right"),
                     len(a_init) - 1)
    coin = uniform(FRET_COIN, c, zero)
    fe = FE[ds, as_]
    return coin <= fe, ds, as_, np.abs(coin - fe)


def isotropic(d_coords, d_eqs, a_coords, a_eqs, K, n_samples, uniform, first_chain=0):
    """-> (acceptor flags bool [n], k2s, FEs, eqs, avg_FE, |coin - avg_FE| [n]) over the states
    with nonzero eq prob, donor-major"""
    d_eqs, a_eqs = np.asarray(d_eqs, dtype=np.float64), np.asarray(a_eqs, dtype=np.float64)
    ds, as_ = np.where(d_eqs != 0)[0], np.where(a_eqs != 0)[0]
    k2, _, FE, _ = table(np.asarray(d_coords)[ds], np.asarray(a_coords)[as_], K)
    eqs = (d_eqs[ds][:, None] * a_eqs[as_][None, :]).reshape(-1)
    avg = float(np.average(FE.reshape(-1), weights=eqs))
    c = first_chain + np.arange(n_samples)
    coin = uniform(FRET_COIN, c, np.zeros(n_samples, dtype=np.int64))
    return coin <= avg, k2.reshape(-1), FE.reshape(-1), eqs, avg, np.abs(coin - avg)


# ---- inputs --------------------------------------------------------------------------------
def random_coords(rng, n, centre, spread=0.8):
    """[n, 9]: emission centres and dipole origins scattered round ``centre``, random dipoles"""
    c = np.asarray(centre, dtype=np.float64) + spread * rng.randn(n, 3)
    return np.hstack([c, c + 0.1 * rng.randn(n, 3), 0.3 * rng.randn(n, 3)])


def random_msm(rng, n, nnz, empty=()):
    """(T [n, n] row-stochastic with ``nnz`` nonzeros a row, eqs [n]); the states ``empty``
    have empty rows, nothing enters them and their eq prob is 0"""
    live = np.array([i for i in range(n) if i not in set(empty)])
    T = np.zeros((n, n))
    for i in live:
        cols = rng.choice(live, size=min(nnz, len(live)), replace=False)
        T[i, cols] = rng.dirichlet(np.ones(len(cols)))
        T[i] /= T[i].sum()
    eqs = np.zeros(n)
    eqs[live] = rng.dirichlet(np.ones(len(live)))
    return T, eqs
