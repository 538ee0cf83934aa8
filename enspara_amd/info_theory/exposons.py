"""Exposons (Porter et al, Biophys. J. 116, 2019; reference
enspara/info_theory/exposons.py): groups of residues whose sidechains' solvent
exposure changes together.  Sidechain solvent-accessible surface areas
(``geometry.sasa``, on the device) are made binary at a threshold, their
pairwise mutual information is taken with frame weights (``weighted_mi``, on
the device) and clustered by affinity propagation (``_affinity``, on the host:
``[n_res, n_res]`` work).

Where this differs from the reference, on purpose: there is no topology
reader, so coordinates, radii, atom names and residue indices are passed
instead of an ``md.Trajectory``; ``exposons`` does not run the reference's
first, discarded clustering; an empty sidechain is ``DataInvalid`` where the
reference asserts.
"""
import logging

import numpy as np

from .. import exception
from ..geometry import sasa as _sasa
from . import _affinity
from .mutual_info import weighted_mi

logger = logging.getLogger(__name__)

__all__ = ["exposons", "exposons_from_sasas", "get_sidechain_atom_ids",
           "condense_sidechain_sasas", "BACKBONE_NAMES"]

BACKBONE_NAMES = frozenset(["N", "C", "CA", "O", "HA", "H", "H1", "H2", "H3", "OXT"])


def get_sidechain_atom_ids(atom_names, residue_index):
    """Discover the atom IDs for atoms that are in sidechains: atoms that are
    NOT named N, C, CA, O, HA, H, H1, H2, H3 or OXT.

    Parameters
    ----------
    atom_names : sequence of str, length n_atoms
    residue_index : sequence of int, length n_atoms
        The residue (0 .. n_residues - 1) each atom belongs to.

    Returns
    -------
    sc_ids : list of np.ndarray
        The atom ids of each residue's sidechain, ascending (possibly empty).
    """
    residue_index = np.asarray(residue_index)
    if residue_index.ndim != 1 or len(atom_names) != len(residue_index):
        raise exception.DataInvalid(
            "%d atom names for %s residue indices" % (len(atom_names), residue_index.shape,))
    if not np.issubdtype(residue_index.dtype, np.integer) or (
            residue_index.size and residue_index.min() < 0):
        raise exception.DataInvalid("Residue indices are integers from 0.")
    side = np.array([str(a).strip() not in BACKBONE_NAMES for a in atom_names], dtype=bool)
    n_res = int(residue_index.max()) + 1 if residue_index.size else 0
    return [np.flatnonzero(side & (residue_index == r)) for r in range(n_res)]


def condense_sidechain_sasas(sasas, sidechain_ids):
    """Condense atomic SASAs into sidechain SASAs.

    Parameters
    ----------
    sasas : np.ndarray, shape=(n_confs, n_atoms)
        Atomic solvent accessibilities.
    sidechain_ids : list of index arrays
        The atoms of each sidechain (``get_sidechain_atom_ids``).

    Returns
    -------
    rsd_sasas : np.ndarray, shape=(n_confs, n_sidechains), float32
        The float32 sum of each sidechain's atoms, added in the order listed
        from 0 (what ``geometry.sasa.shrake_rupley(atom_groups=...)`` returns).
    """
    sasas = np.asarray(sasas, dtype=np.float32)
    if sasas.ndim != 2:
        raise exception.DataInvalid("sasas is [n_confs, n_atoms], not %s" % (sasas.shape,))
    out = np.zeros((sasas.shape[0], len(sidechain_ids)), dtype=np.float32)
    for i, ids in enumerate(sidechain_ids):
        ids = np.asarray(ids)
        if ids.ndim != 1 or ids.size == 0:
            raise exception.DataInvalid("Found 0 atoms for sidechain %d." % i)
        if ids.min() < 0 or ids.max() >= sasas.shape[1]:
            raise exception.DataInvalid(
                "Sidechain %d names atoms %d .. %d, which didn't match the number of "
                "SASAs provided (%d). Make sure you computed atom-level SASAs."
                % (i, ids.min(), ids.max(), sasas.shape[1]))
        for a in ids:
            out[:, i] = out[:, i] + sasas[:, a]
    return out


def exposons_from_sasas(sasas, damping, weights, threshold, device=0):
    """Compute exposons from sidechain SASAs.

    Parameters
    ----------
    sasas : np.ndarray, shape=(n_conformations, n_sidechains)
        SASAs to use in the calculations.
    damping : float
        Damping parameter to use for affinity propagation. Goes from 0.5
        to <1.0. Empirically, values between 0.85 and 0.95 tend to work best.
    weights : ndarray, shape=(n_conformations,)
        Weight of each frame for the mutual information calculation.
    threshold : float
        Sidechains with greater than this amount of total SASA count as
        exposed for the exposed/buried dichotomy.

    Returns
    -------
    sasa_mi : np.ndarray, shape=(n_res, n_res)
        Mutual information of each sidechain with each other sidechain.
    exposons : np.ndarray, shape=(n_res,)
        Assignment of residues to exposons.
    """
    sasa_mi = weighted_mi(np.asarray(sasas) > threshold, weights, device=device)
    labels = _affinity.affinity_propagation(sasa_mi, damping=damping, preference=0,
                                            max_iter=10000)
    return sasa_mi, labels


def exposons(xyz, radii, sidechain_ids, damping, weights=None, probe_radius=0.28,
             threshold=0.02, n_sphere_points=960, device=0):
    """Compute exposons for a trajectory (or, with `weights`, for the centers
    of an MSM).

    Parameters
    ----------
    xyz : np.ndarray, shape=(frames, atoms, 3), float32
        Coordinates in nm.
    radii : array, shape=(atoms,)
        van der Waals radii in nm (``geometry.sasa.radii_from_elements``).
    sidechain_ids : list of index arrays
        The atoms of each residue's sidechain (``get_sidechain_atom_ids``).
    damping : float
        Damping parameter of affinity propagation, in [0.5, 1).
    weights : ndarray, shape=(frames,), default=None
        Weight of each frame; None weights all frames equally.
    probe_radius : float, default=0.28
        Size of the solvent probe in nm (the exposons paper used 0.28, the
        radius of two water molecules).
    threshold : float, default=0.02
        Sidechains with more than this total SASA count as exposed.
    n_sphere_points : int, default=960

    Returns
    -------
    sasa_mi, exposons : as ``exposons_from_sasas``
    """
    n = len(xyz)
    if weights is None:
        weights = np.full((n,), 1 / n) if n else np.zeros(0)
    else:
        weights = np.array(weights) / sum(weights)
    sasas = _sasa.shrake_rupley(xyz, radii, probe_radius=probe_radius,
                                n_sphere_points=n_sphere_points,
                                atom_groups=sidechain_ids, device=device)
    return exposons_from_sasas(sasas, damping, weights, threshold, device=device)
