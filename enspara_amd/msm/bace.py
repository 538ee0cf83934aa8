"""BACE, the Bayesian agglomerative clustering engine (reference
enspara/msm/bace.py; Bowman, J. Chem. Phys. 137, 134111 (2012)): coarse-grain
the states of a count matrix into macrostates by merging, again and again, the
pair of states whose transition statistics are the least distinguishable.

The Bayes factors run on the device (csrc/ek_msm_bace.hip): those of the prune
step, one workgroup per state, and the whole merge loop -- the initial pair
matrix, every merge, the row of factors it invalidates and the arg-max of the
matrix -- without a host round trip between merges.  The host keeps what is
O(n) bookkeeping: ``absorb`` and the relabelling after each merge, rebuilt from
the merge records the device returns.

Types are the reference's, because they decide the merges: counts, weights and
every sum float64; the sum rounded to float32; its inverse taken in float32;
the reported factor ``float32(1) / dMat[minX, minY]``.  The float64 sum's order
is the device's own (the reference's is a BLAS dot of unspecified order), so a
result can differ from the reference's where two candidate pairs lie within a
float32 ulp of each other or a sum straddles a float32 rounding boundary, and
nowhere else.
"""
import numpy as np
import scipy.sparse

from .. import _lib
from ..exception import DataInvalid

__all__ = ["bace", "baysean_prune", "absorb"]

# one step of ek_msm_bace_run (include/enspara_hip.h)
_RECORD = np.dtype([("x", np.int32), ("y", np.int32), ("bf", np.float32),
                    ("status", np.int32)])


def _dense_counts(c):
    """``c`` as a new, checked float64 array."""
    if scipy.sparse.issparse(c):
        c = c.toarray()
    c = np.array(c, dtype=np.float64, order="C")
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise DataInvalid("a count matrix is square, not %s" % (c.shape,))
    if c.shape[0] < 2:
        raise DataInvalid("BACE needs at least 2 states, not %d" % c.shape[0])
    if not np.all(np.isfinite(c)) or np.any(c < 0):
        raise DataInvalid("counts are finite and not negative")
    return c


def absorb(c, absorb_states):
    """Absorb each of ``absorb_states``, in the order given, into its
    kinetically nearest neighbour: the state it has the most counts to (the
    first of them on ties), its own self-counts aside (reference
    bace.py:255-307).  Host only.

    Returns ``(c, labels)``: the counts with the absorbed states' rows and
    columns added to their destinations' and zeroed (the shape stays), and for
    every state the index of the state it now belongs to among those that are
    left, renumbered as the reference does: every absorption moves the labels
    above the absorbed state's down by one.  A state whose row is all zeros
    gets label -1 and is skipped -- nothing is renumbered for it, so the labels
    above it keep a gap, in ``bace``'s labels as well; one with self-counts only
    cannot be absorbed and raises ``DataInvalid``.

    Differs from the reference: sparse input is densified for the work and
    comes back in the type it came in (the reference returns ``lil``)."""
    kind = type(c) if scipy.sparse.issparse(c) else None
    c = c.toarray() if kind is not None else np.array(c)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise DataInvalid("a count matrix is square, not %s" % (c.shape,))
    labels = np.arange(c.shape[0])
    for s in absorb_states:
        own = c[s, s]
        c[s, s] = 0
        if c[s].sum() == 0:
            if own:
                raise DataInvalid("State %s can't be absorbed into a neighbor "
                                  "because it is disconnected." % s)
            labels[s] = -1
            continue
        dest = int(np.argmax(c[s]))
        c[dest, :] += c[s, :]
        c[:, dest] += c[:, s]
        c[dest, dest] += own
        c[s, :] = 0
        c[:, s] = 0
        labels[labels >= labels[s]] -= 1
        labels[s] = labels[dest]
    return (c if kind is None else kind(c)), labels


def _prune_factors(dense, device=0):
    """float32 Bayes factor of every state against the pseudo-state, on the
    device (reference bace.py:341-369)."""
    n = dense.shape[0]
    w = np.ascontiguousarray(dense.sum(axis=1) + 1)
    d = np.zeros(n, dtype=np.float32)
    L = _lib.load()
    _lib.check(L.ek_msm_bace_prune(int(device), n, _lib.f64p(dense), _lib.f64p(w),
                                   _lib.f32p(d)))
    return d


def baysean_prune(c, n_procs=1, factor=np.log(3), device=0):
    """Prune the states whose Bayes factor against a state of pseudo-counts
    only is below ``factor``, absorbing them into their kinetically nearest
    neighbour (reference bace.py:310-377) -> ``(c_pruned, labels,
    kept_states)``.

    The factors are computed on the device, one workgroup per state, in the
    reference's types: weights = row sums + 1, the pseudo-state
    ``float32(1) / float32(n)``, a float64 sum rounded to float32, which is
    compared with the float64 ``factor`` (``<`` prunes, ``>=`` keeps).
    ``absorb`` runs on the host.  Sparse input is densified for the work and
    the counts come back in the type they came in.  ``n_procs`` is accepted and
    has no effect on the result."""
    dense = _dense_counts(c)
    d = _prune_factors(dense, device=device)
    prune = np.where(d < factor)[0]
    keep = np.where(d >= factor)[0]
    c_pruned, labels = absorb(c if hasattr(c, "shape") else np.array(c), prune)
    return c_pruned, labels, keep


def _results_from_records(state_map, m, n_macrostates, records):
    """The device's merge records -> ``(bayes_factors, labels)``.  ``state_map``:
    the prune's labels; ``m``: states kept; ``records[i]``: the pair and factor
    the matrix showed after i merges.  Merge i (1-based) joins the pair of
    record i - 1 and gives ``labels[m - i]``; record i gives
    ``bayes_factors[m - 1 - i]``."""
    state_map = np.array(state_map, dtype=int)
    bayes_factors, labels = {}, {}
    for i in range(len(records)):
        if i > 0:
            prev = records[i - 1]
            if prev["status"] != 0:
                raise DataInvalid(
                    "no pair of states with more than one count between them is "
                    "left at %d macrostates: the counts are disconnected and "
                    "%d macrostates cannot be reached" % (m - i + 1, n_macrostates))
            x, y = int(prev["x"]), int(prev["y"])
            # reference bace.py:155-157: the merged state's label goes, the labels
            # above it move down, its members take minX's
            drop = state_map[y]
            members = state_map == drop
            state_map[state_map >= drop] -= 1
            state_map[members] = state_map[x]
            labels[m - i] = state_map.copy()
        bayes_factors[m - 1 - i] = records["bf"][i]
    return bayes_factors, labels


def _bace_full(c, n_macrostates, device=0, dmat_steps=0):
    """``bace`` -> ``(bayes_factors, labels, records, dmats)``: what ``bace``
    returns, the device's merge records (``x``, ``y``, ``bf``, ``status`` per
    step) and, for the first ``dmat_steps`` steps (the initial matrix is step
    0), the whole float32 matrix of inverse Bayes factors as the step left
    it."""
    dense = _dense_counts(c)
    n = dense.shape[0]
    n_macrostates = int(n_macrostates)
    if n_macrostates < 1:
        raise DataInvalid("n_macrostates must be at least 1, not %d" % n_macrostates)
    pruned, state_map, kept = baysean_prune(dense, device=device)
    state_map = state_map.astype(int)
    m = len(kept)
    if m < 1:
        raise DataInvalid("no state has enough counts to survive the prune")
    pruned = np.ascontiguousarray(pruned, dtype=np.float64)
    w = np.ascontiguousarray(pruned.sum(axis=1))
    w[kept] += 1
    n_merges = max(m - n_macrostates, 0)
    dmat_steps = min(int(dmat_steps), n_merges + 1)
    records = np.zeros(n_merges + 1, dtype=_RECORD)
    dmats = np.zeros((max(dmat_steps, 1), n, n), dtype=np.float32)
    kept32 = np.ascontiguousarray(kept, dtype=np.int32)
    L = _lib.load()
    _lib.check(L.ek_msm_bace_run(
        int(device), n, _lib.f64p(pruned), _lib.f64p(w), _lib.i32p(kept32), m,
        n_macrostates, n_merges, records.ctypes.data, dmat_steps, _lib.f32p(dmats)))

    bayes_factors, labels = _results_from_records(state_map, m, n_macrostates, records)
    return bayes_factors, labels, records, dmats[:dmat_steps]


def bace(c, n_macrostates, chunk_size=100, n_procs=1, device=0):
    """Bayesian agglomerative coarse-graining (reference bace.py:45-119; if you
    use it, read and cite Bowman, J. Chem. Phys. 137, 134111 (2012)).

    Parameters
    ----------
    c : array-like or scipy sparse matrix, shape=(n_states, n_states)
        Transition counts.  Sparse input is densified on the host; the result
        is the dense path's.
    n_macrostates : int
        Number of macrostates to coarse-grain into.
    chunk_size, n_procs :
        Accepted for the reference's signature; no effect on the result (they
        have none in the reference either).
    device : int
        The HIP device.

    Returns
    -------
    bayes_factors : dict
        Number of macrostates -> the (float32) Bayes factor of the merge that
        leads to it.
    labels : dict
        Number of macrostates -> the labelling of the microstates into that
        many macrostates (-1: a state without counts).

    States are first pruned (``baysean_prune``); with m the number of states
    kept, the device then computes the inverse Bayes factor of every pair
    ``s < d`` with ``c[s, d] > 1`` and performs the merges: the pair with the
    largest entry (the first in row-major order on ties) is merged, the row of
    the merged state is recomputed, and so on.

    Where this differs from the reference, on purpose:

    * Number of merges and keys.  With p = n - m states pruned the reference
      still runs ``n - n_macrostates`` merges -- p too many, which take the
      arg-max of an all-zero matrix, merge state 0 with itself and report
      ``inf`` -- and keys ``labels`` by ``n - cycle - 1``, shifted by p.  Here
      ``m - n_macrostates`` merges run, ``labels`` has the keys
      ``m - 1 .. n_macrostates`` and ``bayes_factors`` the keys
      ``m - 1 .. n_macrostates - 1``.  With p = 0 that is the reference exactly;
      with p > 0 ``labels[k]`` here is the reference's ``labels[k + p]``.
    * No eligible pair left.  If no pair with ``c > 1`` remains before
      ``n_macrostates`` is reached (disconnected counts: the matrix's largest
      entry is 0), ``DataInvalid`` is raised and names the number of
      macrostates reached.
    * ``n_macrostates >= m`` performs no merge: ``labels == {}`` and
      ``bayes_factors`` holds the one factor of the initial matrix.
    * ``c`` must be square, finite, not negative, with at least 2 states;
      otherwise ``DataInvalid``.
    * The order of the float64 sums (see the module's docstring)."""
    return _bace_full(c, n_macrostates, device=device)[:2]
