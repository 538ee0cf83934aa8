"""Information theory on the device (reference enspara/info_theory): joint
counts of discrete features on the int8 matrix cores and the mutual
information matrices built on them (``mutual_info``; csrc/ek_mi.hip).

Absent: ``weighted_mi`` (float-weighted sums are a different kernel),
``entropy`` and ``exposons``.
"""
from . import mutual_info  # noqa: F401
from .mutual_info import (  # noqa: F401
    mi_matrix, mi_matrix_serial, joint_counts, mutual_information, mi_to_nmi_apc,
    deconvolute_network, mi_to_nmi, mi_to_apc, channel_capacity_normalization,
    check_features_states, JointCounts, MI_CHUNK, MAX_STATES)

__all__ = ["mutual_info"] + list(mutual_info.__all__)
