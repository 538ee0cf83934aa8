"""Explicit dye geometry: kappa squared, distance and Forster radius of a donor and
an acceptor conformation (the array-only part of the reference's
enspara/geometry/explicit_r0_calc.py).

A dye conformation is 9 doubles, as ``assemble_dye_r_mu`` of the reference lays them
out: the emission centre, the origin of the transition dipole and the dipole vector
(not normalised), in nm.  ``dye_r_mu`` makes them from atom coordinates and atom
indices; there is no topology reader here, so where the reference takes an mdtraj
trajectory and a dye name these functions take ``coords [n_states, 9]``.

Host (numpy, the reference's expressions): ``calc_R0``, ``calc_k2_r`` (vectorised over
leading axes), ``dye_r_mu``, ``find_dyeless_states``, ``remove_bad_states``.
Device: ``pair_table``, every (donor state, acceptor state) of a pair of dye MSMs at
once (csrc/ek_dye_pair.hip); ``geometry.dye_lifetimes`` runs the
excitations on the same function.

Bursts (csrc/ek_dye_bursts.hip): ``simulate_burst_k2`` (and
``sample_k2_bursts``, the same photon by photon) runs a chain of the protein MSM per
burst and, at every photon, draws one of the donor's and one of the acceptor's
conformations of the state the chain is in; ``sample_dye_coords`` is that draw on a list
of states; ``remove_dyeless_msm_states`` the reference's host step before it.  Burst
``b`` is chain ``b`` of the seed: the chain of
``dyes_from_expt_dist.sample_FRET_histograms`` and of
``dye_lifetimes.sample_lifetime_bursts``.  On purpose different from the reference:

* *seeding and chains*: one seed reproduces a run and every burst has its own chain; the
  reference seeds only the initial state and lets ``synthetic_trajectory`` and
  ``sample_dye_coords`` use the global generator;
* *one uniform pick*: row ``min(m - 1, int(u m))`` of the state's ``m`` conformations
  (the clamp because ``u m`` can round up to ``m``); a state one of whose dyes has no
  conformation raises ``DataInvalid`` naming it when a photon is emitted there;
* *``FE`` from ``c6`` without roots*: ``FE = c6 k2 / (c6 k2 + r^6)`` with ``c6 =
  0.02108^6 Qd J / n^4`` and ``r^6 = (r^2)^3``, the bits of ``pair_table``, not via
  ``calc_R0``'s sixth root; it differs from the reference's by rounding;
* ``dye_params = (J, Qd, Td)`` stands for the two dye names; ``n_procs`` is ignored;
  messages go to ``logging``; a removed state's equilibrium probability is exactly 0.

Labelling (csrc/ek_dye_map.hip): ``map_dye_on_protein`` superposes every
conformation of a dye library on the labelled residue of every protein centre
(``geometry.rmsf``'s superposition, one fit per (centre, conformation)), counts the dye
atoms that touch no protein atom (the float64 test of
``dyes_from_expt_dist.remove_touches_protein``), keeps the conformations with at most
``atom_tol`` touching atoms and returns their ``dye_r_mu`` rows;
``align_full_dye_to_res`` and ``remove_touches_protein_dye_traj`` are its two steps alone.
There is no topology: the residue's and the dye's fit atoms (``prot_sel``, ``dye_sel``),
the residue's own atoms (``exclude_atoms``), the radii and the dye's ``r_atom`` and
``mu_atoms`` are arrays and indices.  On purpose different from the reference: a (centre,
conformation) whose optimal rotation is not determined raises ``DataInvalid`` (as
``rmsf.superpose``); nothing is written to disk (``save_aligned_dyes``: ask for
``return_aligned``); ``n_procs`` does not exist.

Not ported: ``load_dye``, ``load_library``, ``get_dye_overlap`` (files, yaml, pandas: the
caller passes ``dye_params = (J, Qd, Td)`` and the dye library as an array);
``map_dye_on_protein``'s ``save_aligned_dyes`` and ``weight_dyes`` (a file output, and an
option the reference itself raises on).
"""
import ctypes
import logging

import numpy as np

from .. import _lib, exception

__all__ = ["calc_R0", "calc_k2_r", "dye_r_mu", "find_dyeless_states", "remove_bad_states",
           "pair_table", "R0_CONSTANT", "sample_dye_coords", "remove_dyeless_msm_states",
           "sample_k2_bursts", "simulate_burst_k2", "DyeMap", "map_dye_on_protein",
           "align_full_dye_to_res", "remove_touches_protein_dye_traj", "dye_reach",
           "cull_radius"]

_log = logging.getLogger(__name__)

R0_CONSTANT = 0.02108       # for R0 in nm


def calc_R0(k2, QD, J, n=1.333):
    """Forster radius in nm: ``0.02108 (k2 QD J / n^4)^(1/6)`` (the reference's
    expression; ``k2`` may be an array)."""
    n4 = n**4
    return R0_CONSTANT * np.power(np.asarray(k2, dtype=np.float64) * QD * J / n4, 1 / 6)


def calc_k2_r(Donor_coords, Acceptor_coords):
    """``(k2, r)`` of donor and acceptor conformations ``[..., 9]`` (leading axes
    broadcast): ``r`` between the emission centres, the angles between the dipole
    vectors and the vector joining the dipole origins,
    ``k2 = (cosT - 3 cosD cosA)^2``."""
    D = np.asarray(Donor_coords, dtype=np.float64)
    A = np.asarray(Acceptor_coords, dtype=np.float64)
    if D.shape[-1:] != (9,) or A.shape[-1:] != (9,):
        raise exception.DataInvalid(
            "dye coordinates are [..., 9], got %s and %s" % (D.shape, A.shape))
    dot = lambda a, b: (a * b).sum(axis=-1)                 # noqa: E731
    norm = lambda a: np.sqrt(dot(a, a))                     # noqa: E731
    c = D[..., 0:3] - A[..., 0:3]
    r = norm(c)
    rvec = D[..., 3:6] - A[..., 3:6]
    D_vec, A_vec = D[..., 6:9], A[..., 6:9]
    cos_theta_T = dot(A_vec, D_vec) / (norm(A_vec) * norm(D_vec))
    cos_theta_D = dot(rvec, D_vec) / (norm(rvec) * norm(D_vec))
    cos_theta_A = dot(A_vec, rvec) / (norm(A_vec) * norm(rvec))
    k2 = (cos_theta_T - (3 * cos_theta_D * cos_theta_A))**2
    return k2, r


def dye_r_mu(xyz, r_atom, mu_atoms):
    """The array form of the reference's ``assemble_dye_r_mu``: ``xyz [n_frames,
    n_atoms, 3]`` (nm), the index ``r_atom`` of the emission centre's atom and the two
    indices ``mu_atoms`` of the dipole's -> ``[n_frames, 9]``: centre, dipole origin
    (the first dipole atom), ``mu0 - mu1``."""
    xyz = np.asarray(xyz)
    if xyz.ndim != 3 or xyz.shape[2] != 3:
        raise exception.DataInvalid("xyz is [n_frames, n_atoms, 3], got %s" % (xyz.shape,))
    idx = [int(r_atom), int(mu_atoms[0]), int(mu_atoms[1])]
    if min(idx) < 0 or max(idx) >= xyz.shape[1]:
        raise exception.DataInvalid("atom indices %s do not fit %d atoms" % (idx, xyz.shape[1]))
    mu0, mu1 = xyz[:, idx[1], :], xyz[:, idx[2], :]
    return np.hstack((xyz[:, idx[0], :], mu0, np.subtract(mu0, mu1)))


def find_dyeless_states(dye_coords):
    """Indices of the entries of ``dye_coords`` (a ragged array or a list) that hold
    no dye position."""
    return np.array([i for i in range(len(dye_coords)) if len(dye_coords[i]) == 0])


def remove_bad_states(bad_states, t_counts):
    """A copy of ``t_counts`` with the rows and columns of ``bad_states`` zeroed."""
    t_counts = np.copy(t_counts)
    if len(bad_states) == 0:
        return t_counts
    bad_states = np.asarray(bad_states, dtype=np.int64)
    t_counts[:, bad_states] = 0
    t_counts[bad_states, :] = 0
    return t_counts


def pair_table(d_coords, a_coords, dye_params, dye_lagtime=None, n=1.333, device=0):
    """Every pair of a donor and an acceptor conformation on the device.

    Parameters
    ----------
    d_coords, a_coords : array, shape=(nd, 9) and (na, 9)
    dye_params : (J, Qd, Td)
        Spectral overlap, donor quantum yield, donor lifetime without acceptor (ns).
    dye_lagtime : float, optional
        The lag time of the dye MSMs in ns; with it the decay CDFs are returned too.

    Returns
    -------
    k2, r, FE : arrays, shape=(nd, na); with a lag time also the decay CDF
    ``[nd, na, 3]``: radiative, non-radiative, energy transfer (the fourth entry,
    still excited, is 1).
    """
    from . import dye_lifetimes
    with dye_lifetimes.DyePair(
            dye_lifetimes.geometry_problem(d_coords, a_coords, dye_params,
                                           1.0 if dye_lagtime is None else dye_lagtime, n=n),
            device=device) as pair:
        k2, r, FE, cdf = pair.pair_table(0)
    return (k2, r, FE) if dye_lagtime is None else (k2, r, FE, cdf)


# ---- bursts with explicit dyes (csrc/ek_dye_bursts.hip) ------------------------
def _conformations(coords, what, n_states=None):
    """per-state conformations (a ragged array or a list of ``[m, 9]`` arrays, ``[]`` for
    a dyeless state) -> (off int64 [n + 1], xyz float64 [total, 9])"""
    try:
        rows = [np.asarray(coords[i], dtype=np.float64) for i in range(len(coords))]
    except (TypeError, ValueError):
        raise exception.DataInvalid(
            "%s coordinates are a list over the protein states of [m, 9] arrays." % what)
    if not rows or (n_states is not None and len(rows) != n_states):
        raise exception.DataInvalid(
            "%s coordinates of %d states do not fit %s protein states."
            % (what, len(rows), "any" if n_states is None else n_states))
    for s, c in enumerate(rows):
        if c.size == 0:
            rows[s] = np.zeros((0, 9))
        elif c.ndim != 2 or c.shape[1] != 9:
            raise exception.DataInvalid(
                "The %s conformations of state %d are [m, 9], got %s." % (what, s, c.shape))
        elif not np.all(np.isfinite(c)):
            raise exception.DataInvalid(
                "The %s conformations of state %d are not finite." % (what, s))
        if len(rows[s]) >= 2 ** 31:
            raise exception.DataInvalid("State %d has 2^31 %s conformations or more." % (s, what))
    off = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    return off, np.ascontiguousarray(np.concatenate(rows), dtype=np.float64)


def _raise_no_conformation(d_off, a_off, state):
    if state >= 0:
        lacks = [w for w, off in (("donor", d_off), ("acceptor", a_off))
                 if off[state + 1] == off[state]]
        raise exception.DataInvalid(
            "A photon was emitted in state %d, which has no %s conformation."
            % (state, " and no ".join(lacks)))


def _c6(dye_params, n):
    from . import dye_lifetimes
    try:
        J, Qd, Td = (float(v) for v in dye_params)
        n = float(n)
    except (TypeError, ValueError):
        raise exception.DataInvalid("dye_params is (J, Qd, Td), n a number")
    if not (J >= 0 and np.isfinite(J) and n > 0 and np.isfinite(n)):
        raise exception.DataInvalid("J >= 0 and n > 0, got %r, %r" % (J, n))
    if not 0 < Qd <= 1:
        raise exception.DataInvalid("Qd in (0, 1], got %r" % Qd)
    return dye_lifetimes.R0_6_constant(Qd, J, n)


def sample_dye_coords(donor_coords, acceptor_coords, states, random_state=None, chain=0,
                      device=0, return_conformations=False):
    """A donor and an acceptor conformation for every entry of ``states``, drawn uniformly
    from the state's own, and their ``(k2s, rs)``; with ``return_conformations`` also
    the two row indices.  Entry *k* draws what photon *k* of burst ``chain`` draws in
    ``simulate_burst_k2``.

    donor_coords, acceptor_coords : per protein state ``[m, 9]`` (``dye_r_mu``'s layout)
    """
    from . import dye_lifetimes as dl
    d_off, d_xyz = _conformations(donor_coords, "donor")
    a_off, a_xyz = _conformations(acceptor_coords, "acceptor", len(d_off) - 1)
    n_states = len(d_off) - 1
    s = dl.sd._states(states, n_states, "states")
    chain = dl._chain(chain)
    dl.last_seed = seed = dl.sd._seed(random_state)
    flags = np.empty(len(s), dtype=np.uint8)
    k2s, rs = np.empty(len(s)), np.empty(len(s))
    rows = [np.empty(len(s), dtype=np.int32) for _ in range(2)] if return_conformations else None
    bad = ctypes.c_int64(-1)
    _lib.check(_lib.load().ek_dye_photons_k2(
        int(device), seed, chain, len(s), _lib.i32p(s), n_states, _lib.i64p(d_off),
        _lib.f64p(d_xyz), _lib.i64p(a_off), _lib.f64p(a_xyz), 0.0, _lib.u8p(flags),
        _lib.f64p(k2s), _lib.f64p(rs),
        _lib.i32p(rows[0]) if rows else dl._null(ctypes.c_int32),
        _lib.i32p(rows[1]) if rows else dl._null(ctypes.c_int32), ctypes.byref(bad)))
    _raise_no_conformation(d_off, a_off, bad.value)
    return (k2s, rs, rows[0], rows[1]) if rows else (k2s, rs)


def remove_dyeless_msm_states(dye_coords1, dye_coords2, eq_probs, t_counts, device=0):
    """The MSM without the states one of whose dyes has no conformation: their rows and
    columns of the counts zeroed, row-normalised, with its equilibrium probabilities
    (exactly 0 for a removed state).  -> ``(eqs, tprobs, dye_coords1, dye_coords2)``,
    the coordinates as lists in which, as in the reference, a removed state holds one row
    of zeros as a mark.  Messages go to ``logging``."""
    from ..msm import builders
    t_counts = np.asarray(t_counts)
    if t_counts.ndim != 2 or t_counts.shape[0] != t_counts.shape[1]:
        raise exception.DataInvalid("t_counts is square, not %s" % (t_counts.shape,))
    n = len(t_counts)
    eq_probs = np.asarray(eq_probs, dtype=np.float64)
    if eq_probs.shape != (n,):
        raise exception.DataInvalid(
            "eq_probs of shape %s do not fit %d states." % (eq_probs.shape, n))
    _conformations(dye_coords1, "dye 1", n)
    _conformations(dye_coords2, "dye 2", n)
    bad1, bad2 = find_dyeless_states(dye_coords1), find_dyeless_states(dye_coords2)
    bad = np.unique(np.concatenate((bad1, bad2))).astype(np.int64)
    if len(bad) == n:
        raise exception.DataInvalid("No protein state could be labelled.")
    _log.info("%d and %d states had no available dye configuration.", len(bad1), len(bad2))
    counts, tprobs, eqs = builders.normalize(remove_bad_states(bad, t_counts),
                                             calculate_eq_probs=True, device=device)
    lost = float(eq_probs[bad].sum())
    _log.info("Total states removed: %d/%d; lost %.3f%% of the original eq probs.",
              len(bad), n, 100 * lost)
    if len(bad) / n > 0.2:
        _log.warning("Labeling resulted in lots of states lost from the MSM.")
    if lost > 0.2:
        _log.warning("Labeling at this position resulted in major probability loss.")
    eqs = np.array(eqs, dtype=np.float64)
    eqs[bad] = 0.0      # (nothing enters a removed state: exactly 0, not the solver's rounding)
    c1 = [np.asarray(dye_coords1[i]) for i in range(n)]
    c2 = [np.asarray(dye_coords2[i]) for i in range(n)]
    for i in bad:
        c1[i] = np.zeros((1, 9))
        c2[i] = np.zeros((1, 9))
    return eqs, tprobs, c1, c2


def sample_k2_bursts(T, populations, dye_coords1, dye_coords2, MSM_frames, dye_params, n=1.333,
                     random_state=None, return_trajectories=False, return_conformations=False,
                     device=0, step_cap=None):
    """Bursts of photons with explicit dye geometry, photon by photon: every burst runs a
    chain of the protein MSM and, at every frame of ``MSM_frames``, draws a donor and an
    acceptor conformation of the state the chain is in; the photon is the acceptor's iff
    its coin is ``<= FE = c6 k2 / (c6 k2 + r^6)`` of the pair.

    Returns ``(photons uint8, k2s, rs, states int32)``, RaggedArrays of a row per burst;
    with ``return_conformations`` also the donor's and the acceptor's row indices
    (int32); with ``return_trajectories`` last the chains, an object array of int32
    arrays.  ``simulate_burst_k2`` is this with the reference's return values."""
    from . import dye_lifetimes as dl
    c6 = _c6(dye_params, n)
    sampler, own = dl.sd._sampler(T, device)
    try:
        d_off, d_xyz = _conformations(dye_coords1, "donor", sampler.n_states)
        a_off, a_xyz = _conformations(dye_coords2, "acceptor", sampler.n_states)

        def call(L, h, seed, b0, nb, sub_off, sub_frames, pop, cap, subs, traj):
            bad_row, bad_state = ctypes.c_int64(-1), ctypes.c_int64(-1)
            null = dl._null(ctypes.c_int32)
            _lib.check(L.ek_dye_bursts_k2(
                h, seed, b0, nb, _lib.i64p(sub_off), _lib.i64p(sub_frames), _lib.f64p(pop),
                _lib.i64p(d_off), _lib.f64p(d_xyz), _lib.i64p(a_off), _lib.f64p(a_xyz), c6, cap,
                _lib.u8p(subs[0]), _lib.f64p(subs[1]), _lib.f64p(subs[2]), _lib.i32p(subs[3]),
                _lib.i32p(subs[4]) if return_conformations else null,
                _lib.i32p(subs[5]) if return_conformations else null, traj,
                ctypes.byref(bad_row), ctypes.byref(bad_state)))
            dl.sd._raise_bad_row(bad_row.value)
            _raise_no_conformation(d_off, a_off, bad_state.value)

        outputs = [np.float64, np.float64, np.int32] + \
            ([np.int32, np.int32] if return_conformations else [])
        foff, flat, trajs = dl._run_bursts(sampler, populations, MSM_frames, random_state,
                                           return_trajectories, step_cap, outputs, call)
    finally:
        if own:
            sampler.close()
    out = tuple(dl._ragged(a, foff) for a in flat)
    return out + (trajs,) if return_trajectories else out


def simulate_burst_k2(MSM_frames, T, populations, dye_coords1, dye_coords2, dye_params, n=1.333,
                      random_state=None, return_trajectories=True, return_conformations=False,
                      device=0, step_cap=None, n_procs=1):
    """The reference's ``simulate_burst_k2`` -> ``(FEs, trajs, k2s, rs)``: per burst the
    share of acceptor photons, the chain (``None`` without ``return_trajectories``), and
    the kappa squared and distance behind every photon (RaggedArrays); with
    ``return_conformations`` also the donor's and the acceptor's row indices.
    ``dye_params = (J, Qd, Td)`` stands for the reference's two dye names; ``n_procs`` is
    accepted and ignored."""
    out = sample_k2_bursts(T, populations, dye_coords1, dye_coords2, MSM_frames, dye_params, n=n,
                           random_state=random_state, return_trajectories=return_trajectories,
                           return_conformations=return_conformations, device=device,
                           step_cap=step_cap)
    FEs = np.array([np.mean(p) for p in out[0]])
    trajs = out[-1] if return_trajectories else None
    extra = tuple(out[4:6]) if return_conformations else ()
    return (FEs, trajs, out[1], out[2]) + extra


# ---- labelling: a dye library on a residue of every centre (csrc/ek_dye_map.hip; 4q) ---------
MAX_SEL = 16                # DM_MAX_SEL
MAX_CENTRES = 32768         # DM_MAX_CENTRES: centres of one device run
MAX_COORD = 2.0 ** 20       # DM_MAX_COORD, nm


class DyeMap(object):
    """What ``map_dye_on_protein`` returns.

    coords : list over the centres of float64 ``[kept_p, 9]``, the ``dye_r_mu`` rows of the
        kept conformations (what ``sample_dye_coords``, ``remove_dyeless_msm_states``,
        ``simulate_burst_k2`` and ``find_dyeless_states`` take)
    kept : list over the centres of int64 arrays, the kept conformations, ascending
    counts : int32 ``[P, D]``, the dye atoms of every conformation that touch no atom
    coords_all : float64 ``[P, D, 9]``, every conformation (``dye_lifetimes.problem`` and
        ``calc_lifetimes`` take this together with ``kept``)
    aligned : float32 ``[P, D, A, 3]`` or None
    list_len : int32 ``[P]``, the protein atoms that passed the cull
    timing : ms between device events, summed over the chunks: upload, fit, cull, touch,
        download
    """

    def __init__(self, coords, kept, counts, coords_all, aligned, list_len, timing):
        self.coords, self.kept, self.counts = coords, kept, counts
        self.coords_all, self.aligned = coords_all, aligned
        self.list_len, self.timing = list_len, timing

    def __len__(self):
        return len(self.coords)


def _real_array(a, name, shape_text, ndim, dtype=None):
    a = np.asarray(a)
    if a.ndim != ndim or (ndim == 3 and a.shape[2] != 3) or 0 in a.shape:
        raise exception.DataInvalid("%s is %s, not %s" % (name, shape_text, a.shape))
    if dtype is not None and a.dtype != dtype:
        raise exception.DataInvalid("%s is %s, not %s" % (name, np.dtype(dtype), a.dtype))
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
        raise exception.DataInvalid("%s is a real array, not %s" % (name, a.dtype))
    if not np.isfinite(a).all():
        raise exception.DataInvalid("%s holds values that are not finite." % name)
    return a


def _coordinates(a, name, shape_text):
    """float32 [.., .., 3], finite and within 2^20 nm: one pass (a NaN or an infinity fails the
    comparison too); the library does not look at a run's coordinates again"""
    a = np.asarray(a)
    if a.ndim != 3 or a.shape[2] != 3 or 0 in a.shape:
        raise exception.DataInvalid("%s is %s, not %s" % (name, shape_text, a.shape))
    if a.dtype != np.float32:
        raise exception.DataInvalid("%s is float32, not %s" % (name, a.dtype))
    if not (float(a.min()) >= -MAX_COORD and float(a.max()) <= MAX_COORD):
        raise exception.DataInvalid(
            "%s holds coordinates that are not finite or lie beyond 2^20 nm." % name)
    return np.ascontiguousarray(a)


def _indices(idx, n, name, lo=0, hi=None):
    """a list of distinct atom indices in [0, n), its length in [lo, hi] -> int32"""
    try:
        a = np.asarray(idx)
    except (TypeError, ValueError):
        raise exception.DataInvalid("%s is a list of atom indices." % name)
    if a.size == 0:
        a = a.astype(np.int64)
    if a.ndim != 1 or a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise exception.DataInvalid("%s is a 1-D list of integer atom indices." % name)
    if a.size < lo or (hi is not None and a.size > hi):
        raise exception.DataInvalid(
            "%s holds %d atoms, not %d to %s." % (name, a.size, lo, "any" if hi is None else hi))
    if a.size and (a.min() < 0 or a.max() >= n):
        raise exception.DataInvalid(
            "%s indexes atoms %d .. %d; there are %d atoms." % (name, a.min(), a.max(), n))
    if np.unique(a).size != a.size:
        raise exception.DataInvalid("%s repeats an atom." % name)
    return np.ascontiguousarray(a, dtype=np.int32)


def _selections(prot_sel, dye_sel, atoms, A):
    p = _indices(prot_sel, atoms, "prot_sel", 3, MAX_SEL)
    d = _indices(dye_sel, A, "dye_sel", 3, MAX_SEL)
    if len(p) != len(d):
        raise exception.DataInvalid(
            "prot_sel and dye_sel pair atoms: %d and %d were given." % (len(p), len(d)))
    return p, d


def _cutoffs(radii, probe_radius, atoms):
    radii = _real_array(radii, "radii", "[atoms]", 1)
    if radii.shape != (atoms,):
        raise exception.DataInvalid("radii is [%d], not %s" % (atoms, radii.shape))
    try:
        probe = float(probe_radius)
    except (TypeError, ValueError):
        raise exception.DataInvalid("probe_radius is a number, not %r" % (probe_radius,))
    # (the float64 sum made on the host, as the reference's atomic_radii + probe_radius)
    cutoff = np.ascontiguousarray(radii.astype(np.float64) + probe)
    if not (np.isfinite(probe) and (cutoff > 0).all() and (cutoff <= MAX_COORD).all()):
        raise exception.DataInvalid("radius + probe_radius must lie in (0, 2^20] nm for every atom.")
    return cutoff


def _atom_tol(atom_tol, A):
    if isinstance(atom_tol, bool) or not isinstance(atom_tol, (int, np.integer)) \
            or not 0 <= atom_tol <= A:
        raise exception.DataInvalid("atom_tol = %r is not an integer in [0, %d]" % (atom_tol, A))
    return int(atom_tol)


def _chunk_centres(chunk_centres):
    if chunk_centres is None:
        return None
    if isinstance(chunk_centres, bool) or not isinstance(chunk_centres, (int, np.integer)) \
            or chunk_centres < 1:
        raise exception.DataInvalid(
            "chunk_centres = %r is not a positive integer" % (chunk_centres,))
    return min(int(chunk_centres), MAX_CENTRES)


def dye_reach(dye_xyz, dye_sel=None):
    """The largest distance (float64) of any dye atom from its conformation's selection
    centroid (from the mean of all atoms of the library with ``dye_sel=None``, the form
    without a fit): no aligned dye atom is farther from the residue's centroid."""
    x = np.asarray(dye_xyz, dtype=np.float64)
    if dye_sel is None:
        c = x.reshape(-1, 3).mean(axis=0)[None, None, :]
    else:
        sel = np.asarray(dye_sel)
        c = np.zeros((len(x), 3))
        for k in sel:                       # (the float64 sum in selection order of 4q)
            c = c + x[:, k, :]
        c = (c / float(len(sel)))[:, None, :]
    d = x - c
    return float(np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
                         + d[..., 2] * d[..., 2]).max())


def cull_radius(reach, c_ref, cutoff, fit=True):
    """The distance from ``c_ref`` (the centroid of the residue's fit atoms) beyond which
    an atom of cut-off ``cutoff`` can touch no aligned dye atom: ``reach + cutoff + margin``,
    ``margin = 2^-22 (max|c_ref| + reach) + 2^-40 reach`` ("Margin"), times the
    ``1 + 2^-40`` that covers the cull's own roundings.  What csrc/ek_dye_map.hip computes."""
    margin = (float(np.abs(c_ref).max()) + reach) * 2.0 ** -22 + reach * 2.0 ** -40 if fit else 0.0
    return ((reach + margin) + np.asarray(cutoff, dtype=np.float64)) * (1.0 + 2.0 ** -40)


def _assemble(counts, coords_all, n_dye_atoms, atom_tol):
    """the reference's ``counts >= len(dye.xyz[0]) - atom_tol`` per centre -> (coords, kept)"""
    kept = [np.flatnonzero(c >= n_dye_atoms - atom_tol).astype(np.int64) for c in counts]
    coords = [np.ascontiguousarray(coords_all[p][k]) for p, k in enumerate(kept)]
    return coords, kept


def _run_map(xyz, cutoff, exclude, dye_xyz, prot_sel, dye_sel, r_atom, mu0, mu1, want_aligned,
             chunk, device):
    """the validated device calls -> counts, coords_all, aligned, list_len, timing"""
    P, atoms = xyz.shape[:2]
    D, A = dye_xyz.shape[:2]
    L = _lib.load()
    counts = np.empty((P, D), dtype=np.int32)
    coords_all = np.empty((P, D, 9), dtype=np.float64)
    flags = np.empty((P, D), dtype=np.uint8)
    aligned = np.empty((P, D, A, 3), dtype=np.float32) if want_aligned else None
    list_len = np.empty(P, dtype=np.int32)
    timing, ms = np.zeros(5), np.zeros(5)
    null32 = ctypes.POINTER(ctypes.c_int32)()
    h = ctypes.c_void_p()
    _check_map(L.ek_dye_map_open(
        int(device), atoms, _lib.f64p(cutoff), len(exclude),
        _lib.i32p(exclude) if len(exclude) else null32, D, A, _lib.f32p(dye_xyz),
        0 if prot_sel is None else len(prot_sel),
        null32 if prot_sel is None else _lib.i32p(prot_sel),
        null32 if dye_sel is None else _lib.i32p(dye_sel), r_atom, mu0, mu1, ctypes.byref(h)))
    try:
        if chunk is None:
            fits = ctypes.c_int64(0)
            _check_map(L.ek_dye_map_max_centres(h, int(want_aligned), ctypes.byref(fits)))
            chunk = int(fits.value)
        for p0 in range(0, P, chunk):
            n = min(chunk, P - p0)
            _check_map(L.ek_dye_map_run(h, _lib.f32p(xyz[p0:p0 + n]), n, int(want_aligned)))
            _check_map(L.ek_dye_map_fetch(
                h, n, _lib.i32p(counts[p0:p0 + n]), _lib.f64p(coords_all[p0:p0 + n]),
                _lib.u8p(flags[p0:p0 + n]),
                _lib.f32p(aligned[p0:p0 + n]) if want_aligned
                else ctypes.POINTER(ctypes.c_float)()))
            _check_map(L.ek_dye_map_stats(h, n, _lib.i32p(list_len[p0:p0 + n]),
                                          ctypes.POINTER(ctypes.c_double)()))
            _check_map(L.ek_dye_map_last_timing(h, _lib.f64p(ms)))
            timing += ms
    finally:
        L.ek_dye_map_close(h)
    bad = np.argwhere(flags != 0)
    if len(bad):
        raise exception.DataInvalid(
            "The optimal rotation of conformation %d on centre %d is not determined (collinear "
            "fit atoms, or s2 + s3 ~ 0); %d such (centre, conformation) pairs."
            % (bad[0][1], bad[0][0], len(bad)))
    return counts, coords_all, aligned, list_len, timing


def _check_map(rc):
    if rc == _lib.EK_ENOMEM:
        msg = _lib.load().ek_last_error().decode("utf-8", "replace")
        raise exception.InsufficientResourceError(msg)
    _lib.check(rc)


def _map_inputs(xyz, radii, dye_xyz, prot_sel, dye_sel, exclude_atoms, r_atom, mu_atoms,
                probe_radius, atom_tol, chunk_centres):
    xyz = _coordinates(xyz, "xyz", "[centres, atoms, 3]")
    dye_xyz = _coordinates(dye_xyz, "dye_xyz", "[conformations, dye atoms, 3]")
    atoms, (D, A) = xyz.shape[1], dye_xyz.shape[:2]
    if D * A >= 2 ** 31 - 256:
        raise exception.DataInvalid("dye_xyz holds 2^31 atoms or more.")
    cutoff = _cutoffs(radii, probe_radius, atoms)
    psel, dsel = _selections(prot_sel, dye_sel, atoms, A)
    exclude = _indices(exclude_atoms, atoms, "exclude_atoms")
    idx = _indices([r_atom] if np.ndim(r_atom) == 0 else r_atom, A, "r_atom", 1, 1)
    mu = _indices(mu_atoms, A, "mu_atoms", 2, 2)
    return (xyz, cutoff, dye_xyz, psel, dsel, exclude, int(idx[0]), int(mu[0]), int(mu[1]),
            _atom_tol(atom_tol, A), _chunk_centres(chunk_centres))


def map_dye_on_protein(xyz, radii, dye_xyz, prot_sel, dye_sel, exclude_atoms, r_atom, mu_atoms,
                       probe_radius=0.04, atom_tol=6, return_aligned=False, chunk_centres=None,
                       device=0):
    """The reference's ``map_dye_on_protein`` on arrays: every conformation of a dye library
    superposed on the labelled residue of every protein centre, the conformations that clash
    with the protein removed.

    Parameters
    ----------
    xyz : float32 ``[P, atoms, 3]``, the protein centres (nm)
    radii : ``[atoms]``, the atoms' radii (nm)
    dye_xyz : float32 ``[D, A, 3]``, the dye's conformations as they come
    prot_sel, dye_sel : equally long lists of 3 to 16 atom indices, paired: the residue's and
        the dye's N, CA, CB, C, O in the reference (N, CA, C, O for GLY and PRO)
    exclude_atoms : the labelled residue's atoms, which the touch test skips (the
        reference's ``atom_slice('not resSeq ...')``)
    r_atom : the dye atom at the emission centre
    mu_atoms : the two dye atoms of the transition dipole; the origin is the first, the
        vector ``mu_atoms[0] - mu_atoms[1]``.  The reference gets them from mdtraj's
        ``select('(name X) or (name Y)')``, which returns ASCENDING indices whatever the
        order of the names: its origin is the lower-indexed of the two atoms.  Pass
        ``sorted(...)`` to reproduce it.
    probe_radius : a dye atom touches an atom within ``radius + probe_radius`` (float64,
        ``sqrt((dx dx + dy dy) + dz dz) > cutoff`` is free).  No dye radius is added, as in
        the reference (its comment says otherwise).
    atom_tol : a conformation is kept iff at most ``atom_tol`` of its atoms touch
    return_aligned : also return the aligned coordinates ``[P, D, A, 3]``
    chunk_centres : centres of one device run; by default what fits half of the free
        device memory.  The result's bits do not depend on it.

    Returns
    -------
    DyeMap
    """
    (xyz, cutoff, dye_xyz, psel, dsel, exclude, r, mu0, mu1, tol, chunk) = _map_inputs(
        xyz, radii, dye_xyz, prot_sel, dye_sel, exclude_atoms, r_atom, mu_atoms, probe_radius,
        atom_tol, chunk_centres)
    counts, coords_all, aligned, list_len, timing = _run_map(
        xyz, cutoff, exclude, dye_xyz, psel, dsel, r, mu0, mu1, bool(return_aligned), chunk, device)
    coords, kept = _assemble(counts, coords_all, dye_xyz.shape[1], tol)
    return DyeMap(coords, kept, counts, coords_all, aligned, list_len, timing)


def align_full_dye_to_res(frame_xyz, dye_xyz, prot_sel, dye_sel, device=0):
    """Every conformation of ``dye_xyz [D, A, 3]`` superposed on the atoms ``prot_sel`` of
    ``frame_xyz [atoms, 3]`` over its atoms ``dye_sel`` -> float32 ``[D, A, 3]`` (the
    alignment of ``map_dye_on_protein``, bit for bit)."""
    frame = np.asarray(frame_xyz)
    if frame.ndim != 2:
        raise exception.DataInvalid("frame_xyz is [atoms, 3], not %s" % (frame.shape,))
    xyz = _coordinates(frame[None], "frame_xyz", "[atoms, 3]")
    dye_xyz = _coordinates(dye_xyz, "dye_xyz", "[conformations, dye atoms, 3]")
    atoms, A = xyz.shape[1], dye_xyz.shape[1]
    psel, dsel = _selections(prot_sel, dye_sel, atoms, A)
    # (every atom excluded: nothing to test)
    _, _, aligned, _, _ = _run_map(xyz, np.ones(atoms), np.arange(atoms, dtype=np.int32), dye_xyz,
                                   psel, dsel, 0, 0, 0, True, None, device)
    return aligned[0]


def remove_touches_protein_dye_traj(frame_xyz, radii, aligned_dye_xyz, exclude_atoms,
                                    probe_radius=0.04, atom_tol=6, device=0):
    """The reference's function on arrays: the indices (int64, ascending) of the
    conformations of ``aligned_dye_xyz [D, A, 3]`` at most ``atom_tol`` of whose atoms lie
    within ``radius + probe_radius`` of an atom of ``frame_xyz [atoms, 3]`` outside
    ``exclude_atoms``.  The coordinates are taken as they are."""
    frame = np.asarray(frame_xyz)
    if frame.ndim != 2:
        raise exception.DataInvalid("frame_xyz is [atoms, 3], not %s" % (frame.shape,))
    xyz = _coordinates(frame[None], "frame_xyz", "[atoms, 3]")
    dye_xyz = _coordinates(aligned_dye_xyz, "aligned_dye_xyz", "[conformations, dye atoms, 3]")
    atoms, A = xyz.shape[1], dye_xyz.shape[1]
    cutoff = _cutoffs(radii, probe_radius, atoms)
    exclude = _indices(exclude_atoms, atoms, "exclude_atoms")
    tol = _atom_tol(atom_tol, A)
    counts, _, _, _, _ = _run_map(xyz, cutoff, exclude, dye_xyz, None, None, 0, 0, 0, False, None,
                                  device)
    return np.flatnonzero(counts[0] >= A - tol).astype(np.int64)
