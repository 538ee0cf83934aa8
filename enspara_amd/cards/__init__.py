"""Correlation of All Rotameric and Dynamical States (reference enspara/cards) on
the device: rotamer states from coordinates (csrc/ek_rotamer.hip), transition
statistics, order / disorder states and the four mutual-information matrices
(csrc/ek_cards.hip, on the count and information kernels of csrc/ek_mi.hip), and
the Shannon entropies of the rotamer states per dihedral and per residue
(``entropy``; csrc/ek_entropy.hip).
"""
from . import disorder, entropy, featurizers  # noqa: F401
from .cards import cards, cards_matrices  # noqa: F401
from .disorder import (  # noqa: F401
    transitions, traj_ord_disord_times, create_disorder_traj, assign_order_disorder,
    transition_stats, aggregate_mean_times, disorder_interval, times_from_stats,
    CardsStates, SCAN_CHUNK, MAX_FRAMES)
from .entropy import shannon_entropies, residue_shannon_entropies  # noqa: F401
from .featurizers import RotamerFeaturizer  # noqa: F401

__all__ = ["cards", "cards_matrices", "RotamerFeaturizer", "disorder", "featurizers",
           "SCAN_CHUNK", "entropy", "shannon_entropies", "residue_shannon_entropies"
           ] + list(disorder.__all__)
