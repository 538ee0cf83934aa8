"""Information theory on the device (reference enspara/info_theory): joint
counts of discrete features on the int8 matrix cores and the mutual
information matrices built on them (``mutual_info``; csrc/ek_mi.hip), the
mutual information of weighted observations on the float64 matrix cores
(``weighted_mi``; csrc/ek_wmi.hip) and exposons (``exposons``: solvent
accessibility from ``geometry.sasa``, ``weighted_mi``, affinity propagation on
the host), and the relative entropy of Markov state models, Jensen-Shannon
divergence, Shannon entropy and per-feature state counts (``entropy``;
csrc/ek_entropy.hip).
"""
from . import mutual_info  # noqa: F401
from . import entropy  # noqa: F401
from . import exposons  # noqa: F401
from .mutual_info import (  # noqa: F401
    mi_matrix, mi_matrix_serial, joint_counts, mutual_information, mi_to_nmi_apc,
    deconvolute_network, mi_to_nmi, mi_to_apc, channel_capacity_normalization,
    check_features_states, JointCounts, MI_CHUNK, MAX_STATES, WMI_CHUNK,
    weighted_joint_probabilities, weighted_mi, weighted_mi_last_timing)

__all__ = ["mutual_info", "exposons", "entropy"] + list(mutual_info.__all__)
