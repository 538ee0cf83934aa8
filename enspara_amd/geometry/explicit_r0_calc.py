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

Not ported: ``load_dye``, ``load_library``, ``get_dye_overlap`` (files, yaml, pandas: the
caller passes ``dye_params = (J, Qd, Td)``); ``align_full_dye_to_res``,
``remove_touches_protein_dye_traj``, ``map_dye_on_protein`` (mdtraj superposition and
selection: the caller passes aligned coordinates and the states to keep; the per-frame
touch test itself is ``dyes_from_expt_dist.remove_touches_protein``).
"""
import ctypes
import logging

import numpy as np

from .. import _lib, exception

__all__ = ["calc_R0", "calc_k2_r", "dye_r_mu", "find_dyeless_states", "remove_bad_states",
           "pair_table", "R0_CONSTANT", "sample_dye_coords", "remove_dyeless_msm_states",
           "sample_k2_bursts", "simulate_burst_k2"]

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
