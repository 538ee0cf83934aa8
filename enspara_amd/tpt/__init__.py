"""Transition path theory on the device (reference enspara/tpt): committors and
mean first passage times (``core``), reactive fluxes, net fluxes and reactive
populations (``tpt``) of a transition probability matrix.

The linear algebra -- assembling ``I - Q`` or ``I - T + W``, a float64 LU with
partial pivoting whose trailing update runs on the matrix cores, the
substitutions and the element-wise epilogues -- is csrc/ek_tpt.hip and
csrc/ek_lu.hip; a call uploads ``tprob`` once and downloads its result once.

Absent from this namespace, present in a module of their own: the reference's
``paths`` and ``top_path`` (enspara/tpt/path.py) are
``enspara_amd.tpt.path.paths`` and ``enspara_amd.tpt.path.top_path``, the
widest-path searches on the device (csrc/ek_tpt_path.hip); write
``from enspara_amd.tpt.path import paths`` and hand it ``net_fluxes``' output.
"""
from .core import committors, mfpts  # noqa: F401
from .tpt import reactive_fluxes, net_fluxes, reactive_populations  # noqa: F401

__all__ = ["committors", "mfpts", "reactive_fluxes", "net_fluxes",
           "reactive_populations"]
