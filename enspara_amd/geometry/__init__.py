"""Geometry helpers on the hot path: point-vs-set distances in feature space
(reference enspara/geometry/libdist.pyx), dihedral angles and buffered rotamer
states (reference enspara/geometry/rotamer.py), Shrake-Rupley solvent-accessible
surface areas (``sasa``; what the reference takes from mdtraj)."""
from . import libdist  # noqa: F401
from . import rotamer  # noqa: F401
from . import sasa  # noqa: F401
from .rotamer import all_rotamers  # noqa: F401
