"""Featurizer that converts atomic position trajectories into rotamer
trajectories, by the CARDS definition of rotamer states (reference
enspara/cards/featurizers.py)."""
import logging

from ..geometry import rotamer

logger = logging.getLogger(__name__)

__all__ = ["RotamerFeaturizer"]


class RotamerFeaturizer(object):
    """Convert coordinates into rotamer trajectories.  ``dihedrals`` maps
    "phi" / "psi" / "chi" to ``[n, 4]`` atom indices; ``n_procs`` is accepted
    and ignored."""

    __slots__ = ['dihedrals', 'buffer_width', 'n_procs', 'feature_trajectories_',
                 'n_feature_states_', 'atom_indices_']

    def __init__(self, dihedrals, buffer_width=15, n_procs=1):
        self.dihedrals = dihedrals
        self.buffer_width = buffer_width
        self.n_procs = n_procs

    def fit(self, trajectories, device=0):
        """Assign rotameric states to a set of trajectories (lists and
        generators alike).  Makes available ``feature_trajectories_``,
        ``n_feature_states_`` and ``atom_indices_``."""
        quads, _, n_states = rotamer.check_dihedrals(self.dihedrals)
        self.feature_trajectories_ = [
            rotamer.all_rotamers(t, self.dihedrals, buffer_width=self.buffer_width,
                                 device=device)[0]
            for t in trajectories]
        self.n_feature_states_ = n_states
        self.atom_indices_ = quads
        return self
