"""Geometry helpers on the hot path: point-vs-set distances in feature space
(reference enspara/geometry/libdist.pyx), dihedral angles and buffered rotamer
states (reference enspara/geometry/rotamer.py), Shrake-Rupley solvent-accessible
surface areas (``sasa``; what the reference takes from mdtraj), LIGSITE pocket
detection (``pockets``; reference enspara/geometry/pockets.py), smFRET burst
sampling on a Markov state model (``dyes_from_expt_dist``; the array-only part
of the reference's module of that name), explicit dye geometry and the
donor-excitation Monte Carlo on dye MSMs (``explicit_r0_calc``, ``dye_lifetimes``;
reference modules of those names), superposition on a reference structure and
population-weighted RMSF (``rmsf``; reference enspara/geometry/rmsf.py)."""
from . import libdist  # noqa: F401
from . import rotamer  # noqa: F401
from . import sasa  # noqa: F401
from . import pockets  # noqa: F401
from . import dyes_from_expt_dist  # noqa: F401
from . import explicit_r0_calc  # noqa: F401
from . import dye_lifetimes  # noqa: F401
from . import rmsf  # noqa: F401
from .rotamer import all_rotamers  # noqa: F401
from .pockets import get_pockets, get_pocket_cells, cluster_pocket_cells  # noqa: F401
