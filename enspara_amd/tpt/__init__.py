"""Transition path theory on the device (reference enspara/tpt): committors and
mean first passage times (``core``), reactive fluxes, net fluxes and reactive
populations (``tpt``) of a transition probability matrix.

The linear algebra -- assembling ``I - Q`` or ``I - T + W``, a float64 LU with
partial pivoting whose trailing update runs on the matrix cores, the
substitutions and the element-wise epilogues -- is csrc/ek_tpt.hip and
csrc/ek_lu.hip; a call uploads ``tprob`` once and downloads its result once.

Absent: the reference's ``paths`` and ``top_path`` (enspara/tpt/path.py).  They
are graph searches on the host with no device work in them; run them on
``net_fluxes``' output with the reference or with networkx.
"""
from .core import committors, mfpts  # noqa: F401
from .tpt import reactive_fluxes, net_fluxes, reactive_populations  # noqa: F401

__all__ = ["committors", "mfpts", "reactive_fluxes", "net_fluxes",
           "reactive_populations"]
