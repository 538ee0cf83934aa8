"""Shannon entropies of rotamer states per dihedral and per residue (the
arithmetic of the reference's enspara/apps/compute-shannon-entropy.py: rotamer
counts :155-195, the entropy per dihedral :197-217, the per-residue sum and the
channel capacity :220-329)."""
import numpy as np

from .. import exception
from ..info_theory import entropy

__all__ = ["shannon_entropies", "residue_shannon_entropies"]


def shannon_entropies(feature_trajs, n_feature_states, device=0):
    """The Shannon entropy of every dihedral's rotamer distribution, in nats.

    Parameters
    ----------
    feature_trajs : list of arrays [frames, n_dihedrals]
        Rotamer states (``RotamerFeaturizer.feature_trajectories_``).
    n_feature_states : array, shape=(n_dihedrals,)
        Number of rotamer states of each dihedral
        (``RotamerFeaturizer.n_feature_states_``).

    Returns
    -------
    entropies : np.ndarray, shape=(n_dihedrals,)
        From ``counts = state_counts(...)``, each row over its number of frames,
        and ``shannon_entropy`` (with its normalisation) of every row.
    """
    counts = entropy.state_counts(feature_trajs, n_feature_states, device=device)
    frames = counts.sum(axis=1, keepdims=True)
    return entropy.shannon_entropy_rows(counts / frames, normalize=True, device=device)


def residue_shannon_entropies(dihedral_entropies, n_feature_states, residue_of_feature,
                              n_residues):
    """Per residue, the sum of its dihedrals' entropies over its channel
    capacity ``sum(log(n_states))`` -- the most its dihedrals could carry.  A
    residue without dihedrals gives NaN (0 / 0, as in the reference).

    ``residue_of_feature`` : integer array, shape=(n_dihedrals,)
        The residue index of every dihedral.  The reference's app takes the
        residue of atom 1 of each quad; there is no topology reader here, so
        with ``atom_residue`` [n_atoms] (the residue index of every atom, from
        whatever read the topology) that rule is
        ``atom_residue[featurizer.atom_indices_[:, 1]]``.
    """
    H = np.asarray(dihedral_entropies, dtype=np.float64)
    n = np.asarray(n_feature_states)
    res = np.asarray(residue_of_feature)
    if not np.issubdtype(res.dtype, np.integer):
        raise exception.DataInvalid(
            "residue_of_feature holds residue indices, not %s" % res.dtype)
    if not (H.ndim == 1 and H.shape == n.shape == res.shape):
        raise exception.DataInvalid(
            "one entropy, number of states and residue per dihedral: got shapes %s, %s, %s"
            % (H.shape, n.shape, res.shape))
    n_residues = int(n_residues)
    if res.size and (res.min() < 0 or res.max() >= n_residues):
        raise exception.DataInvalid(
            "residue indices must lie in [0, %d); found %d .. %d"
            % (n_residues, res.min(), res.max()))
    # one pass per quantity: entropies and log-capacities summed into their residues
    log_n = np.log(n.astype(np.float64))
    entropy_sum = np.bincount(res, weights=H, minlength=n_residues)
    capacity = np.bincount(res, weights=log_n, minlength=n_residues)
    with np.errstate(divide="ignore", invalid="ignore"):
        return entropy_sum / capacity
