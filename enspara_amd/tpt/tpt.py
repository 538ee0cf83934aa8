"""Reactive fluxes, net fluxes and reactive populations between a set of
sources and a set of sinks (reference enspara/tpt/tpt.py; Metzner, Schuette and
Vanden-Eijnden, Multiscale Model. Simul. 7, 1192 (2009)).

The flux functions upload ``tprob`` once: the committors are solved on the
device (see ``core.committors``) and the fluxes formed there from them, in the
reference's order of operations, ``(T_ij * (pi_i * (1 - q_i))) * q_j``.

Where this differs from the reference: sparse ``tprob`` is densified for the
work, and the flux functions then return a ``scipy.sparse.lil_matrix`` as the
reference does (an ndarray for dense input); argument errors and singular
systems raise ``DataInvalid`` (see ``core``).
"""
import numpy as np
import scipy.sparse

from .. import _lib
from .core import (_check_info, _dense_tprob, _populations, _source_sink_states,
                   committors)

__all__ = ["reactive_fluxes", "net_fluxes", "reactive_populations"]


def _fluxes(tprob, sources, sinks, populations, net, device):
    T = _dense_tprob(tprob)
    n = T.shape[0]
    sources, sinks = _source_sink_states(sources, sinks, n)
    pops = _populations(T, populations, device)
    q = np.zeros(n)
    out = np.zeros((n, n))
    info = np.zeros(1, dtype=np.int32)
    L = _lib.load()
    _lib.check(L.ek_tpt_fluxes(int(device), n, _lib.f64p(T), _lib.i32p(sources),
                               len(sources), _lib.i32p(sinks), len(sinks),
                               _lib.f64p(pops), 1 if net else 0, _lib.f64p(q),
                               _lib.f64p(out), _lib.i32p(info)))
    _check_info(int(info[0]), "net_fluxes" if net else "reactive_fluxes")
    if scipy.sparse.issparse(tprob):
        return scipy.sparse.lil_matrix(out)
    return out


def reactive_fluxes(tprob, sources, sinks, populations=None, device=0):
    """The flux of reactive trajectories along every edge of an MSM from a set
    of sources to a set of sinks (reference tpt.py:48-91):
    ``f_ij = pi_i (1 - q_i) T_ij q_j`` with the forward committors ``q`` and a
    zero diagonal.

    Parameters
    ----------
    tprob : array-like or scipy sparse matrix, shape=(n_states, n_states)
    sources, sinks : int or array-like of int
    populations : array-like, shape=(n_states,), optional
        Equilibrium populations; computed with ``enspara_amd.msm.eq_probs`` if
        None.
    device : int
        The HIP device.

    Returns
    -------
    fluxes : np.ndarray (float64), or scipy.sparse.lil_matrix for sparse input
    """
    return _fluxes(tprob, sources, sinks, populations, False, device)


def net_fluxes(tprob, sources, sinks, populations=None, device=0):
    """The net flux along every edge, ``max(f_ij - f_ji, 0)`` of
    ``reactive_fluxes`` (reference tpt.py:94-125); arguments and return type
    as there."""
    return _fluxes(tprob, sources, sinks, populations, True, device)


def reactive_populations(tprob, sources, sinks, populations=None, device=0):
    """The probability that a state is observed on a reactive trajectory,
    ``pi_i q_i (1 - q_i)`` normalised to sum 1 (reference tpt.py:128-160).
    The committors are solved on the device; the O(n) rest runs on the host."""
    T = _dense_tprob(tprob)
    pops = _populations(T, populations, device)
    q = committors(T, sources, sinks, device=device)
    densities = pops * q * (1 - q)
    return densities / np.sum(densities)
