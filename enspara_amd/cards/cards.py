"""High-level routines for Correlation of All Rotameric and Dynamical States
(reference enspara/cards/cards.py)."""
import logging

import numpy as np

from ..info_theory import mutual_info
from . import disorder
from .featurizers import RotamerFeaturizer

logger = logging.getLogger(__name__)

__all__ = ["cards", "cards_matrices"]


def cards(trajectories, dihedrals=None, buffer_width=15, n_procs=None, device=0):
    """Compute ordered, disordered and ordered-disordered mutual information
    matrices for the correlation between rotameric states across a set of
    trajectories.

    Parameters
    ----------
    trajectories : iterable of coordinates
        ``[frames, atoms, 3]`` arrays or objects with such an ``.xyz``
        (generators are accepted).
    dihedrals : mapping {"phi": [n, 4], "psi": [n, 4], "chi": [n, 4]}
        The atom indices of the dihedrals (required: nothing here derives them
        from a topology).
    buffer_width : number, default=15
        The width of the no-man's land between rotameric bins.
    n_procs : accepted and ignored.

    Returns
    -------
    structural_mi, disorder_mi, struct_to_disorder_mi, disorder_to_struct_mi :
        ``[n_dihedrals, n_dihedrals]`` float64, normalised by channel capacity
    atom_inds : ``[n_dihedrals, 4]``
    """
    r = RotamerFeaturizer(dihedrals, buffer_width=buffer_width, n_procs=n_procs)
    r.fit(trajectories, device=device)
    return cards_matrices(r.feature_trajectories_, r.n_feature_states_, n_procs,
                          device=device) + (r.atom_indices_,)


def cards_matrices(feature_trajs, n_feature_states, n_procs=None, device=0):
    """Compute the structural, disorder, structure-to-disorder and
    disorder-to-structure mutual information matrices of a set of trajectories
    of state assignments, each ``[F, F]`` float64 and normalised by channel
    capacity.  Every trajectory is uploaded once; the statistics, the disorder
    states and the counts stay on the device; four matrices are downloaded.

    The capacities are float64 logarithms.  (The reference's disorder-disorder
    matrix is divided by ``log(2)`` in float32, because its state numbers of
    the disorder trajectories are int16: 2.7e-9 of each entry.)"""
    trajs, n = disorder.check_feature_trajs(feature_trajs, n_feature_states)
    with disorder.CardsStates(trajs[0].shape[1], int(n.max()), device=device) as d:
        for t in trajs:
            d.add(t)
        d.disorder(*disorder.disorder_interval(*d.mean_times()))
        ss, dd, sd, ds = d.matrices()
    two = 2 * np.ones(len(n), dtype=n.dtype)
    norm = mutual_info.channel_capacity_normalization
    return norm(ss, n, n), norm(dd, two, two), norm(sd, n, two), norm(ds, two, n)
