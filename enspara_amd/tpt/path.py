"""The highest-flux pathways from a set of sources to a set of sinks through a
net-flux matrix (reference enspara/tpt/path.py; Dijkstra, Numer. Math. 1, 269
(1959); Metzner, Schuette and Vanden-Eijnden, Multiscale Model. Simul. 7, 1192
(2009)): ``top_path`` finds the path whose least edge is largest, ``paths``
finds one path after another, removing each from the matrix before the next.

The matrix goes to the device once per call, as a CSR of its entries (a dense
matrix is compacted there, a scipy sparse matrix is uploaded as it is and never
densified); the searches run in one resident workgroup, a batch of paths per
launch, and removing a path edits the CSR in place (csrc/ek_tpt_path.hip, which
also states the rule by which the reference's queue picks its next node).
Paths and fluxes are the reference's bit for bit: the paths are integers, the
fluxes entries of the matrix or single IEEE differences of them, and the
explained flux is added up in the reference's order.

Where this differs from the reference: argument errors raise ``DataInvalid``
before any device call (a matrix that is not square or not finite, empty or
out-of-range sources or sinks); a sparse matrix is accepted and treated as its
dense equivalent.  The reference's quirks are kept: the stopping test runs
after a path is appended (``num_paths=0`` yields one path), a state that is
both source and sink yields no path, and ``total_flux`` is
``net_flux[sources, :].sum()`` as numpy computes it.
"""
import ctypes
import math

import numpy as np
import scipy.sparse

from .. import _lib
from ..exception import DataInvalid
from .core import _states

__all__ = ['paths', 'top_path']

# states up to which a search keeps its per-state arrays in the LDS
# (TPT_PATH_LDS_STATES of csrc/ek_tpt_path.hip; above, in global memory through the
# same code), the bytes it keeps per state, and the width of the search workgroup:
# nothing here computes with them, the tests place their shapes around them
LDS_STATES = 7680       # TPT_PATH_LDS_STATES
STATE_BYTES = 21        # TPT_PATH_STATE_BYTES
SEARCH_WG = 256         # TPT_PATH_WG
MAX_STATES = 65535      # TPT_PATH_MAX_N

_KEEP, _SUBTRACT, _BOTTLENECK = 0, 1, 2
_NEVER = 2 ** 62        # a number of paths no run reaches


def _flux_matrix(net_flux):
    """``net_flux`` as a checked C-contiguous float64 array, or as a checked
    canonical CSR matrix (duplicates summed, columns ascending) if it is sparse."""
    if scipy.sparse.issparse(net_flux):
        F = scipy.sparse.csr_matrix(net_flux, dtype=np.float64, copy=True)
        F.sum_duplicates()
        F.sort_indices()
        data = F.data
    else:
        try:
            F = np.ascontiguousarray(np.asarray(net_flux), dtype=np.float64)
        except (TypeError, ValueError):
            raise DataInvalid("the net fluxes are a matrix of numbers")
        data = F
    if F.ndim != 2 or F.shape[0] != F.shape[1] or F.shape[0] < 1:
        raise DataInvalid("a net-flux matrix is square, not %s" % (F.shape,))
    if F.shape[0] > MAX_STATES:
        raise DataInvalid("%d states: the searches take at most %d" % (F.shape[0], MAX_STATES))
    if not np.all(np.isfinite(data)):
        raise DataInvalid("the net-flux matrix has entries that are not finite")
    return F


def _total_flux(F, sources):
    """the reference's ``net_flux[sources, :].sum()``: for a sparse matrix, of the
    dense equivalent of those rows"""
    rows = F[sources, :]
    if scipy.sparse.issparse(rows):
        rows = rows.toarray()
    return float(rows.sum())


class _Search:
    """A handle of ek_tpt_paths_open: the matrix on the device and what was
    explained so far."""

    def __init__(self, F, sources, sinks, mode, num_paths, total_flux, flux_cutoff, device,
                 batch_paths=0, batch_nodes=0):
        self._L = _lib.load()
        self._h = ctypes.c_void_p()
        n = F.shape[0]
        if scipy.sparse.issparse(F):
            dense = None
            indptr = np.ascontiguousarray(F.indptr, dtype=np.int64)
            cols = np.ascontiguousarray(F.indices, dtype=np.int32)
            vals = np.ascontiguousarray(F.data, dtype=np.float64)
            if cols.size == 0:      # (something to point at)
                cols, vals = np.zeros(1, dtype=np.int32), np.zeros(1)
            csr = (_lib.i64p(indptr), _lib.i32p(cols), _lib.f64p(vals))
        else:
            dense, csr = _lib.f64p(F), (None, None, None)
        caps = np.zeros(2, dtype=np.int32)
        _lib.check(self._L.ek_tpt_paths_open(
            int(device), n, dense, csr[0], csr[1], csr[2], _lib.i32p(sources), len(sources),
            _lib.i32p(sinks), len(sinks), mode, num_paths, float(total_flux),
            float(flux_cutoff), int(batch_paths), int(batch_nodes), _lib.i32p(caps),
            ctypes.byref(self._h)))
        self._nodes = np.zeros(int(caps[1]), dtype=np.int32)
        self._offsets = np.zeros(int(caps[0]) + 1, dtype=np.int32)
        self._fluxes = np.zeros(int(caps[0]))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._h:
            h, self._h = self._h, ctypes.c_void_p()
            _lib.check(self._L.ek_tpt_paths_close(h))

    def next(self):
        """-> (paths, fluxes, done) of the next batch"""
        count, done, info = (np.zeros(1, dtype=np.int32) for _ in range(3))
        _lib.check(self._L.ek_tpt_paths_next(
            self._h, _lib.i32p(self._nodes), _lib.i32p(self._offsets),
            _lib.f64p(self._fluxes), _lib.i32p(count), _lib.i32p(done), _lib.i32p(info)))
        if info[0]:
            raise RuntimeError("the path search ran past its own bound (code %d): %s"
                               % (info[0], "a search popped more nodes than there are states"
                                  if info[0] == 1 else "a path is longer than the states"))
        c = int(count[0])
        off = self._offsets
        found = [self._nodes[off[p]:off[p + 1]].astype(np.int64) for p in range(c)]
        return found, self._fluxes[:c].copy(), bool(done[0])

    def stats(self):
        """-> (entries of the CSR, pops, paths, in LDS), (ms compaction, ms searches)"""
        counts, ms = np.zeros(4, dtype=np.int64), np.zeros(2)
        _lib.check(self._L.ek_tpt_paths_stats(self._h, _lib.i64p(counts), _lib.f64p(ms)))
        return tuple(int(c) for c in counts), tuple(float(m) for m in ms)


def _checked(sources, sinks, net_flux):
    F = _flux_matrix(net_flux)
    n = F.shape[0]
    return _states(sources, n, "sources"), _states(sinks, n, "sinks"), F


def top_path(sources, sinks, net_flux, device=0):
    """The path from a source to a sink whose smallest net flux along an edge is
    largest (reference path.py:46-160).

    Parameters
    ----------
    sources, sinks : int or array-like of int
        The source and the sink states.
    net_flux : array-like or scipy sparse matrix, shape=(n_states, n_states)
        Net fluxes, as ``enspara_amd.tpt.net_fluxes`` returns them.
    device : int
        The HIP device.

    Returns
    -------
    path : np.ndarray, int64
        The states of the path, from a source to a sink.  If no sink can be reached
        it is the first sink alone.
    flux : float
        The smallest flux along the path: ``-inf`` if no sink can be reached,
        ``inf`` if a sink is itself a source.
    """
    sources, sinks, F = _checked(sources, sinks, net_flux)
    with _Search(F, sources, sinks, _KEEP, 1, 1.0, 1.0, device) as search:
        found, fluxes, _ = search.next()
    return found[0], float(fluxes[0])


def paths(sources, sinks, net_flux, remove_path='subtract', num_paths=np.inf,
          flux_cutoff=(1 - 1E-10), device=0, _batch_paths=0, _batch_nodes=0):
    """The top paths from the sources to the sinks: find the top path, remove it
    from the net fluxes, repeat (reference path.py:197-320).

    Parameters
    ----------
    sources, sinks : int or array-like of int
        The source and the sink states.
    net_flux : array-like or scipy sparse matrix, shape=(n_states, n_states)
        Net fluxes, as ``enspara_amd.tpt.net_fluxes`` returns them.
    remove_path : {'subtract', 'bottleneck'} or callable
        'subtract' takes the path's flux off every edge of the path (Metzner et
        al.), 'bottleneck' only removes the edge with the least flux.  A callable
        ``f(net_flux, path) -> net_flux`` runs on the host between one device
        ``top_path`` and the next.
    num_paths : number
        Stop after this many paths (the test follows the path: at least one).
    flux_cutoff : float
        Stop once the paths found explain this fraction of
        ``net_flux[sources, :].sum()``.
    device : int
        The HIP device.

    Returns
    -------
    paths : list of np.ndarray (int64)
    fluxes : np.ndarray, float64, shape=(n_paths,)
    """
    if not callable(remove_path) and remove_path not in ('subtract', 'bottleneck'):
        raise ValueError("remove_path (%s) must be a callable or one of "
                         "['subtract', 'bottleneck']" % str(remove_path))
    sources, sinks, F = _checked(sources, sinks, net_flux)
    total_flux = _total_flux(F, sources)
    found, fluxes = [], []

    if callable(remove_path):
        # the reference's loop, a device search per path; the callable sees the
        # matrix in the caller's own form
        net_flux = net_flux.copy() if hasattr(net_flux, "copy") else np.array(net_flux)
        counter, expl_flux = 0, 0.0
        while True:
            path, flux = top_path(sources, sinks, net_flux, device=device)
            if np.isinf(flux):
                break
            found.append(path)
            fluxes.append(flux)
            with np.errstate(all="ignore"):
                expl_flux += np.float64(flux) / np.float64(total_flux)
            counter += 1
            if counter >= num_paths or expl_flux >= flux_cutoff:
                break
            net_flux = remove_path(net_flux, path)
        return found, np.array(fluxes, dtype=np.float64)

    # counter >= num_paths, for a counter that is an integer
    limit = _NEVER if (num_paths != num_paths or num_paths >= _NEVER) else \
        max(int(math.ceil(num_paths)), 0)
    mode = _SUBTRACT if remove_path == 'subtract' else _BOTTLENECK
    with _Search(F, sources, sinks, mode, limit, total_flux, float(flux_cutoff), device,
                 _batch_paths, _batch_nodes) as search:
        done = False
        while not done:
            batch, batch_fluxes, done = search.next()
            found.extend(batch)
            fluxes.extend(batch_fluxes.tolist())
    return found, np.array(fluxes, dtype=np.float64)
