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

Not ported: ``load_dye``, ``load_library``, ``get_dye_overlap`` (files, yaml, pandas: the
caller passes ``dye_params = (J, Qd, Td)``); ``align_full_dye_to_res``,
``remove_touches_protein_dye_traj``, ``map_dye_on_protein`` (mdtraj superposition and
selection: the caller passes aligned coordinates and the states to keep; the per-frame
touch test itself is ``dyes_from_expt_dist.remove_touches_protein``);
``sample_dye_coords`` and ``simulate_burst_k2`` (burst-level resampling).
"""
import numpy as np

from .. import exception

__all__ = ["calc_R0", "calc_k2_r", "dye_r_mu", "find_dyeless_states", "remove_bad_states",
           "pair_table", "R0_CONSTANT"]

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
