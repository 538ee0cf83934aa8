"""smFRET burst simulation on a Markov state model: the array-only subset of the
reference's enspara/geometry/dyes_from_expt_dist.py, the chains and photons on
the device (csrc/ek_kmc.hip).

Ported: ``FRET_efficiency``, ``make_distribution``, ``convert_photon_times``
(numpy, the reference's arithmetic), ``sample_FE_probs`` and
``sample_FRET_histograms`` (device).

Not ported, and why: everything that needs a topology -- ``load_dye``,
``determine_rot_mat``, ``find_atom_index``, ``calc_cb_coords``,
``remove_touches_protein``, ``align_dye_to_res``, ``dye_distance_distribution``
and their helpers place dye point clouds on residues of an mdtraj trajectory,
and this package reads no topologies -- and the histogram post-processing
(``histogram_to_match_expt``, the moment helpers), which is a few numpy lines on
the result with nothing to run on a device.

A burst is one chain of ``msm.synthetic_data`` (chain index = burst index, the
same transition doubles) started from the inverse CDF of ``populations`` and run
to the burst's last frame.  For photon *k* at frame *f* the distance is the
centre of the bin picked by inverse CDF of ``dist_distribution[trj[f]][:, 1]``
plus ``u * bin_width - bin_width / 2`` (``bin_width`` from state 0's first two
centres, as in the reference), ``E = r0^6 / (r0^6 + d^6)`` and the photon is an
acceptor photon iff a further double is ``<= E``.  The device returns one byte
per photon; means and the ``np.std`` of chunk means are the reference's numpy
expressions on the host.

Where this differs from the reference, on purpose:

* ``random_state`` reproduces a run (the reference seeds from the OS in every
  burst and photon); ``n_procs`` is accepted and ignored;
* ``d^6`` is ``(d d)(d d)(d d)`` in float64, not ``d ** 6``: ``E`` can differ
  from the reference's by rounding;
* ``FEs`` is a float64 array, the intraburst deviation NaN when
  ``n_photon_std`` is None (the reference returns an object array holding
  None); ``trajs`` is None when ``return_trajectories`` is off;
* invalid input raises ``DataInvalid`` before any device call.
"""
import ctypes

import numpy as np

from .. import _lib, exception, ra
from ..msm import synthetic_data as _sd

__all__ = ["FRET_efficiency", "make_distribution", "convert_photon_times",
           "divide_chunks", "sample_FE_probs", "sample_FRET_histograms", "last_timing"]

# Bounds on one device call's buffers.  A call lasts as long as its longest burst, however
# few bursts it holds, so the bounds are generous: 4 GiB of trajectories, 2^27 photons.
_TRAJ_CELLS = 1 << 30
_PHOTONS = 1 << 27
_last_ms = np.zeros(3)


def FRET_efficiency(dists, r0, offset=0):
    """Convert distance into FRET efficiency given a Forster radius ``r0`` and
    a distance offset."""
    r06 = r0**6
    return r06 / (r06 + ((dists + offset)**6))


def make_distribution(probs, bin_edges):
    """Per state, ``[bins, 2]``: bin centres and probabilities scaled to sum to
    one.  ``probs`` [n_states][bins], ``bin_edges`` [n_states][bins + 1], ragged."""
    probs_norm = ra.RaggedArray([l / l.sum() for l in probs])
    bin_edges = bin_edges if isinstance(bin_edges, ra.RaggedArray) \
        else ra.RaggedArray(bin_edges)
    dist_vals = (bin_edges[:, 1:] + bin_edges[:, :-1]) / 2.
    return ra.RaggedArray(
        np.vstack([dist_vals._data, probs_norm._data]).T, lengths=probs_norm.lengths)


def divide_chunks(l, n):
    """Yields ``n``-sized chunks from ``l`` (the last may be shorter)."""
    for i in range(0, len(l), n):
        yield l[i:i + n]


def convert_photon_times(inter_photon_times, lagtime, slowing_factor):
    """Inter-photon times (in us) -> MSM frames, for a lag time in ns and a
    factor by which the model is slower than the experiment."""
    conversion_factor = 1000 / (lagtime * slowing_factor)
    return np.array(
        [np.cumsum(np.multiply(inter_photon_times[i], conversion_factor), dtype=int)
         for i in range(len(inter_photon_times))], dtype='O')


def _dist_tables(dist_distribution, n_states):
    """-> (off int64 [n_states + 1], centres, cdf, bin_width): per state the
    bin centres and ``cumsum(p) / last``, as ``np.random.choice`` builds it"""
    try:
        n_rows = len(dist_distribution)
    except TypeError:
        raise exception.DataInvalid("dist_distribution is a sequence of [bins, 2] arrays.")
    if n_rows < n_states:
        raise exception.DataInvalid(
            "dist_distribution has %d rows for %d states." % (n_rows, n_states))
    centres, cdfs, off = [], [], [0]
    for s in range(n_states):
        d = np.asarray(dist_distribution[s], dtype=np.float64)
        if d.ndim != 2 or d.shape[1] != 2 or d.shape[0] < 1:
            raise exception.DataInvalid(
                "dist_distribution[%d] is [bins, 2] (centre, probability), not of shape %s."
                % (s, d.shape))
        p = d[:, 1]
        if not np.all(p >= 0):
            raise exception.DataInvalid(
                "dist_distribution[%d] has negative or NaN probabilities." % s)
        c = np.cumsum(p)
        if not abs(c[-1] - 1.0) <= _sd._ATOL:
            raise exception.DataInvalid(
                "The probabilities of dist_distribution[%d] sum to %r, not 1." % (s, c[-1]))
        c /= c[-1]
        centres.append(d[:, 0])
        cdfs.append(c)
        off.append(off[-1] + len(c))
    d0 = np.asarray(dist_distribution[0], dtype=np.float64)
    if d0.shape[0] < 2:
        raise exception.DataInvalid(
            "dist_distribution[0] needs two bins: the bin width is read off its centres.")
    bin_width = float(d0[1, 0] - d0[0, 0])
    return (np.asarray(off, dtype=np.int64), np.ascontiguousarray(np.concatenate(centres)),
            np.ascontiguousarray(np.concatenate(cdfs)), bin_width)


def sample_FE_probs(dist_distribution, states, R0, random_state=None, chain=0, device=0):
    """A FRET efficiency for every entry of ``states``: a distance drawn from
    the state's distribution (bin by inverse CDF, uniform within the bin),
    converted with the Forster radius ``R0``.  Entry *k* uses the bin and jitter
    doubles (``chain``, *k*) of the seed: what photon *k* of burst ``chain``
    draws in ``sample_FRET_histograms``."""
    states = np.asarray(states)
    n_states = len(dist_distribution)
    s = _sd._states(states, n_states, "states")
    off, centres, cdf, bw = _dist_tables(dist_distribution, n_states)
    chain = int(chain)
    if not 0 <= chain < 2 ** 60:
        raise exception.DataInvalid("chain in [0, 2^60)")
    seed = _sd._seed(random_state)
    E = np.empty(len(s))
    _lib.check(_lib.load().ek_kmc_fret_probs(
        int(device), seed, chain, len(s), _lib.i32p(s), n_states, _lib.i64p(off),
        _lib.f64p(centres), _lib.f64p(cdf), bw, float(R0)**6, _lib.f64p(E)))
    return E


def _frames(MSM_frames):
    """-> (offsets int64 [n_bursts + 1], flat int64 frames), validated"""
    try:
        rows = [np.asarray(f) for f in MSM_frames]
    except TypeError:
        raise exception.DataInvalid("MSM_frames is a list of lists of frames.")
    if not rows:
        raise exception.DataInvalid("No bursts were given.")
    for b, f in enumerate(rows):
        if f.ndim != 1 or f.size == 0 or not (np.issubdtype(f.dtype, np.integer)):
            raise exception.DataInvalid(
                "Burst %d is a non-empty 1-D list of integer frames." % b)
        f = f.astype(np.int64)
        if f[0] < 0 or np.any(np.diff(f) < 0) or f[-1] >= 2 ** 40:
            raise exception.DataInvalid(
                "The frames of burst %d are negative, decrease or exceed 2^40." % b)
        rows[b] = f
    off = np.concatenate([[0], np.cumsum([len(f) for f in rows])]).astype(np.int64)
    return off, np.ascontiguousarray(np.concatenate(rows))


def _pop_cdf(populations, n):
    p = np.asarray(populations, dtype=np.float64)
    if p.shape != (n,):
        raise exception.DataInvalid(
            "populations of shape %s do not fit %d states." % (p.shape, n))
    if not np.all(p >= 0):
        raise exception.DataInvalid("populations has negative or NaN entries.")
    c = np.cumsum(p)
    if not abs(c[-1] - 1.0) <= _sd._ATOL:
        raise exception.DataInvalid("populations sum to %r, not 1." % c[-1])
    c /= c[-1]
    return np.ascontiguousarray(c)


def sample_FRET_histograms(
        T, populations, dist_distribution, MSM_frames, R0, n_procs=1, n_photon_std=None,
        random_state=None, return_trajectories=True, device=0, step_cap=None):
    """Samples a MSM to regenerate experimental FRET distributions.

    Parameters
    ----------
    T : array or scipy sparse matrix, shape=(n_states, n_states), or a Sampler
        Transition probability matrix.
    populations : array, shape=(n_states, )
        State populations; every burst's chain starts from a draw of them.
    dist_distribution : ra.RaggedArray, shape=(n_states, None, 2)
        Per state, bin centres and probabilities of the dye-dye distance.
    MSM_frames : list of lists
        Per burst, the frames at which its photons are emitted (not negative,
        not decreasing; ``convert_photon_times`` makes them).
    R0 : float
        Forster radius of the dyes.
    n_procs : ignored (the bursts run as lanes of one device call).
    n_photon_std : int, optional
        The number of photons to chunk for assessing variation within a burst
        (the last chunk may be shorter).
    random_state : int, optional
        The seed; ``None`` draws one from the OS (``msm.synthetic_data.last_seed``).
    return_trajectories : bool
        Download every burst's chain.  Off, nothing of them is written: for
        10^4 bursts of 10^5 frames they are 4 GB.

    Returns
    -------
    FEs : np.ndarray, shape=(n_bursts, 2)
        The FRET efficiency of every burst (the mean of its acceptor flags) and
        the standard deviation of its chunk means (NaN without ``n_photon_std``).
    trajs : object array of int32 arrays, shape=(n_bursts,), or None
        The states every burst's chain visited, ``last frame + 1`` each.
    """
    sampler, own = _sd._sampler(T, device)
    try:
        n = sampler.n_states
        pop = _pop_cdf(populations, n)
        off, centres, cdf, bw = _dist_tables(dist_distribution, n)
        foff, frames = _frames(MSM_frames)
        if n_photon_std is not None and (
                not isinstance(n_photon_std, (int, np.integer)) or n_photon_std < 1):
            raise exception.DataInvalid("n_photon_std is None or an integer >= 1")
        cap = int(step_cap or 0)
        if cap < 0:
            raise exception.DataInvalid("step_cap > 0")
        seed = _sd._seed(random_state)
        sampler.last_seed = seed
        n_bursts = len(foff) - 1
        lasts = frames[foff[1:] - 1]
        photons = np.empty(len(frames), dtype=np.uint8)
        trajs = np.empty(n_bursts, dtype=object) if return_trajectories else None
        r06 = float(R0)**6
        h = sampler._handle()
        L = sampler._L
        b0 = 0
        _last_ms[:] = 0
        while b0 < n_bursts:
            # as many bursts as stay within the bounds on one call's buffers
            cells = np.cumsum(lasts[b0:] + 1) if return_trajectories else np.zeros(1)
            n_ph = foff[b0 + 1:] - foff[b0]
            fit = int(np.searchsorted(n_ph, _PHOTONS, side="right"))
            if return_trajectories:
                fit = min(fit, int(np.searchsorted(cells, _TRAJ_CELLS, side="right")))
            b1 = min(n_bursts, b0 + max(1, fit))
            sub_off = np.ascontiguousarray(foff[b0:b1 + 1] - foff[b0])
            sub_frames = frames[foff[b0]:foff[b1]]
            sub_ph = photons[foff[b0]:foff[b1]]
            flat = np.empty(int(cells[b1 - b0 - 1]), dtype=np.int32) \
                if return_trajectories else None
            bad = ctypes.c_int64(-1)
            _lib.check(L.ek_kmc_fret_bursts(
                h, seed, b0, b1 - b0, _lib.i64p(sub_off), _lib.i64p(sub_frames),
                _lib.f64p(pop), _lib.i64p(off), _lib.f64p(centres), _lib.f64p(cdf), bw, r06,
                cap, _lib.u8p(sub_ph),
                _lib.i32p(flat) if flat is not None
                else ctypes.cast(None, ctypes.POINTER(ctypes.c_int32)),
                ctypes.byref(bad)))
            _sd._raise_bad_row(bad.value)
            _last_ms[:] += _sd.last_timing()
            if return_trajectories:
                ends = cells[:b1 - b0]
                for i in range(b1 - b0):
                    trajs[b0 + i] = flat[ends[i] - lasts[b0 + i] - 1:ends[i]]
            b0 = b1
    finally:
        if own:
            sampler.close()
    FEs = np.full((n_bursts, 2), np.nan)
    for b in range(n_bursts):
        acceptor_emissions = photons[foff[b]:foff[b + 1]].view(np.bool_)
        FEs[b, 0] = np.mean(acceptor_emissions)
        if n_photon_std is not None:
            FRET_chunks = [np.mean(subset)
                           for subset in divide_chunks(acceptor_emissions, int(n_photon_std))]
            FEs[b, 1] = np.std(FRET_chunks)
    return FEs, trajs


def last_timing():
    """Milliseconds between device events of the last ``sample_FRET_histograms``, summed
    over its device calls: upload, kernels, download."""
    return _last_ms.copy()
