"""smFRET on a Markov state model: the array-only subset of the reference's
enspara/geometry/dyes_from_expt_dist.py.  Dye labelling (point clouds placed on
residues, pairwise distance histograms: csrc/ek_dyes.hip) and burst
simulation (chains and photons: csrc/ek_kmc.hip) run on the device.

Ported: ``FRET_efficiency``, ``make_distribution``, ``convert_photon_times``,
``norm_vec``, ``calc_cb_coords``, ``determine_rot_mat``, ``align_dye_to_res``,
``find_atom_index``, ``load_dye``, ``int_norm_hist``, ``bincount_dists``,
``_merge_histograms`` (numpy, the reference's arithmetic), ``sample_FE_probs``,
``sample_FRET_histograms``, ``remove_touches_protein``,
``pairwise_distance_distribution`` and ``dye_distance_distribution`` (device).

Not ported, and why: ``cluster_grids`` (``cluster_grid_points=True`` raises
``NotImplementedError``: the reference orders clusters by an ``argsort`` that is
not stable for ties, so there is nothing exact to hold a port to),
``rodrigues_rotation``, and the histogram post-processing
(``histogram_to_match_expt``, the moment helpers), which is a few numpy lines on the
result with nothing to run on a device.  The explicit treatment of the dyes that later
versions of the reference build next to this module is ``geometry.explicit_r0_calc`` and
``geometry.dye_lifetimes``.

There is no topology reader here.  Where the reference takes an mdtraj trajectory
and residue numbers, these functions take ``xyz`` ([frames, atoms, 3] float32, nm),
per-atom ``radii`` (nm; ``geometry.sasa.radii_from_elements`` makes them) and a
*backbone*: the three atom indices ``(n, ca, c)`` of a labelled residue
(``backbone_indices`` finds them in per-atom name and residue-number arrays).
The rotation ``M`` and translation ``t`` of a placement are float32 numpy on the
host, the reference's expressions vectorised over frames; the alignment itself is
``p_j = ((x*M[0][j] + y*M[1][j]) + z*M[2][j]) + t[j]`` in float32 (the reference's
``np.matmul`` has no defined order), the touch test and the distances are float64
(DESIGN.md 4l has the whole contract).  ``load_dye`` reads ``.npy`` ([n, 3], nm) or
the coordinate columns of a PDB's ATOM / HETATM records (``/ 10`` to nm, float32):
it is for a user's own copies of the reference's cloud files and is not pinned to
mdtraj's bits.  A frame one of whose placements keeps no point raises
``DataInvalid`` (the reference dies in ``max()`` of an empty array).

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
           "divide_chunks", "sample_FE_probs", "sample_FRET_histograms", "last_timing",
           "norm_vec", "calc_cb_coords", "determine_rot_mat", "align_dye_to_res",
           "find_atom_index", "backbone_indices", "load_dye", "int_norm_hist",
           "bincount_dists", "remove_touches_protein", "pairwise_distance_distribution",
           "dye_distance_distribution", "last_labelling_timing", "MAX_BINS", "MAX_POINTS",
           "MAX_COORD", "MAX_CHUNK_FRAMES"]

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


# ---- dye labelling -------------------------------------------------------------------------
# DY_MAX_BINS, DY_MAX_POINTS, DY_MAX_COORD, DY_MAX_FRAMES of csrc/ek_dyes.hip
MAX_BINS = 4096
MAX_POINTS = 1 << 20
MAX_COORD = 2.0 ** 20
MAX_CHUNK_FRAMES = 4096
_MIN_WIDTH, _MAX_WIDTH = 2.0 ** -40, 2.0 ** 40
_F32 = np.float32
_label_ms = np.zeros(4)


def norm_vec(vec):
    """Divides vectors (the last axis) by their magnitude."""
    vec = np.asarray(vec)
    return vec / np.sqrt(np.einsum('...j,...j->...', vec, vec))[..., None]


def _frames_xyz(xyz, what="xyz"):
    """-> float32 [frames, atoms, 3] and whether a frames axis was added"""
    xyz = np.asarray(xyz)
    if xyz.ndim not in (2, 3) or xyz.shape[-1] != 3 or xyz.shape[-2] < 1:
        raise exception.DataInvalid(
            "%s is [frames, atoms, 3] or [atoms, 3], not %s" % (what, xyz.shape))
    if xyz.dtype != np.float32:
        raise exception.DataInvalid("%s is float32 (nm), not %s" % (what, xyz.dtype))
    if not np.all(np.abs(xyz) <= MAX_COORD):        # (NaN fails this too)
        raise exception.DataInvalid(
            "%s must be finite and within %g nm." % (what, MAX_COORD))
    return (xyz[None] if xyz.ndim == 2 else xyz), xyz.ndim == 2


def _backbones(backbones, atoms, rows=None):
    b = np.asarray(backbones)
    if b.ndim == 1:
        b = b[None]
    if b.ndim != 2 or b.shape[1] != 3 or (rows is not None and b.shape[0] != rows) \
            or not np.issubdtype(b.dtype, np.integer):
        raise exception.DataInvalid(
            "backbones holds %sthe atom indices (n, ca, c) of a residue per row, not %s %s"
            % ("%d rows of " % rows if rows else "", b.dtype, b.shape))
    if b.size and (b.min() < 0 or b.max() >= atoms):
        raise exception.DataInvalid("A backbone index is not in [0, %d)." % atoms)
    return b.astype(np.int64)


def calc_cb_coords(xyz, backbones):
    """Where the CB of each residue belongs, from its N, CA and C.

    ``xyz`` [frames, atoms, 3] (or one frame [atoms, 3]) float32, ``backbones``
    [k, 3] atom indices (n, ca, c) -> float32 [frames, k, 3] (or [k, 3])."""
    x, single = _frames_xyz(xyz)
    b = _backbones(backbones, x.shape[1])
    l = 0.153       # average CA-CB distance
    n_coords, ca_coords, c_coords = x[:, b[:, 0]], x[:, b[:, 1]], x[:, b[:, 2]]
    normed_vec = norm_vec(np.cross(norm_vec(ca_coords - n_coords),
                                   norm_vec(ca_coords - c_coords)))
    ca_vec = norm_vec(ca_coords - ((n_coords + c_coords) / _F32(2.)))
    theta = np.pi / 6.
    ca_dist, norm_dist = _F32(np.sin(theta) * l), _F32(np.cos(theta) * l)
    cb = ca_coords + (ca_dist * ca_vec) + (norm_dist * normed_vec)
    return cb[0] if single else cb


def determine_rot_mat(xyz, backbone):
    """The rotation that puts a residue's CA at the origin, its CB on the z axis
    and its N in the z-y plane, per frame: ``M`` float32 [frames, 3, 3] (rows x, y,
    z) and ``t`` [frames, 3], the CA ([3, 3] and [3] for one frame [atoms, 3])."""
    x, single = _frames_xyz(xyz)
    b = _backbones(backbone, x.shape[1], rows=1)
    cb_coord = calc_cb_coords(x, b)[:, 0]
    n_coord, ca_coord = x[:, b[0, 0]], x[:, b[0, 1]]
    z_vec = norm_vec(cb_coord - ca_coord)
    x_vec = norm_vec(np.cross(norm_vec(n_coord - ca_coord), z_vec))
    y_vec = norm_vec(np.cross(z_vec, x_vec))
    M = np.stack([x_vec, y_vec, z_vec], axis=1)
    return (M[0], ca_coord[0]) if single else (M, ca_coord)


def _align(d, M, t):
    """the contract's order, float32: ((x M0j + y M1j) + z M2j) + tj"""
    return ((d[:, 0:1] * M[0][None, :] + d[:, 1:2] * M[1][None, :])
            + d[:, 2:3] * M[2][None, :]) + t[None, :]


def _cloud(coords, what):
    c = np.asarray(coords)
    if c.ndim != 2 or c.shape[1] != 3 or not 1 <= c.shape[0] <= MAX_POINTS:
        raise exception.DataInvalid(
            "%s is [n, 3] with 1 <= n <= %d, not %s" % (what, MAX_POINTS, c.shape))
    if c.dtype != np.float32:
        raise exception.DataInvalid("%s is float32 (nm), not %s" % (what, c.dtype))
    if not np.all(np.abs(c) <= MAX_COORD):
        raise exception.DataInvalid("%s must be finite and within %g nm." % (what, MAX_COORD))
    return np.ascontiguousarray(c)


def align_dye_to_res(frame_xyz, dye_coords, backbone):
    """A point cloud [n, 3] float32 placed on the residue with the given backbone
    in one frame [atoms, 3]: float32 [n, 3] (host numpy, the device's arithmetic)."""
    x, single = _frames_xyz(frame_xyz, "frame_xyz")
    if not single:
        raise exception.DataInvalid("frame_xyz is one frame, [atoms, 3].")
    M, t = determine_rot_mat(x[0], backbone)
    return _align(_cloud(dye_coords, "dye_coords"), M, t)


def find_atom_index(atom_names, res_seqs, resSeq, atom_name):
    """The index of the first atom called ``atom_name`` in a residue numbered
    ``resSeq``, given every atom's name and residue number; None if there is none."""
    names, seqs = np.asarray(atom_names), np.asarray(res_seqs)
    if names.ndim != 1 or names.shape != seqs.shape:
        raise exception.DataInvalid(
            "atom_names %s and res_seqs %s are one entry per atom." % (names.shape, seqs.shape))
    hit = np.flatnonzero((seqs == resSeq) & (names == atom_name))
    return int(hit[0]) if hit.size else None


def backbone_indices(atom_names, res_seqs, resSeq):
    """The atom indices (N, CA, C) of residue ``resSeq``: int64 [3]."""
    found = [find_atom_index(atom_names, res_seqs, resSeq, a) for a in ("N", "CA", "C")]
    if None in found:
        raise exception.DataInvalid(
            "Residue %r has no %s atom." % (resSeq, ("N", "CA", "C")[found.index(None)]))
    return np.array(found, dtype=np.int64)


def load_dye(path):
    """A dye point cloud, float32 [n, 3] in nm: a ``.npy`` file that holds just
    that, or the coordinate columns of the ATOM / HETATM records of a PDB file
    (Angstrom, divided by 10).  Not pinned to what mdtraj makes of the same file."""
    path = str(path)
    if path.lower().endswith(".npy"):
        cloud = np.asarray(np.load(path))
        if cloud.ndim != 2 or cloud.shape[1] != 3 or not np.issubdtype(cloud.dtype, np.floating):
            raise exception.DataInvalid("%s does not hold an [n, 3] float array." % path)
        cloud = cloud.astype(np.float32)
    else:
        rows = []
        try:
            with open(path) as f:
                for line in f:
                    if line.startswith(("ATOM", "HETATM")):
                        rows.append([float(line[30:38]), float(line[38:46]), float(line[46:54])])
        except (OSError, ValueError) as e:
            raise exception.DataInvalid("%s is not a readable PDB file: %s" % (path, e))
        cloud = np.array(rows, dtype=np.float32).reshape(-1, 3) / _F32(10)
    if len(cloud) == 0 or not np.all(np.isfinite(cloud)):
        raise exception.DataInvalid("%s holds no points, or points that are not finite." % path)
    return cloud


def int_norm_hist(xs, ys):
    """``ys`` scaled so that its integral over the edges (or points) ``xs`` is one."""
    if ys.shape[0] == xs.shape[0] - 1:
        heights = ys
    elif ys.shape[0] == xs.shape[0]:
        heights = (ys[1:] + ys[:-1]) / 2.
    dx = xs[1:] - xs[:-1]
    return ys / np.sum(heights * dx)


def bincount_dists(dists, bin_width=0.1):
    """A histogram of ``dists`` from zero in bins of ``bin_width``, with room for
    the largest: ``counts, bin_edges``."""
    nbins = int(dists.max() / bin_width) + 2
    return np.histogram(dists, bins=nbins, range=[0, nbins * bin_width])


def _merge_histograms(counts, bin_edges, weights=None):
    """Histograms over uniform bins from zero, added (weighted) bin by bin: the
    sum and the edges of the first histogram with the most bins."""
    weights = np.ones(len(counts)) if weights is None else np.array(weights).reshape(-1)
    lens = [c.shape[0] for c in counts]
    n_pads = np.max(lens) - lens
    padded = np.array([np.hstack([counts[n], np.zeros(n_pads[n], dtype=int)])
                       for n in range(len(counts))])
    return np.sum(padded * weights[:, None], axis=0), bin_edges[np.argmax(lens)]


def _width(bin_width):
    try:
        w = float(bin_width)
    except (TypeError, ValueError):
        raise exception.DataInvalid("bin_width is a number, not %r" % (bin_width,))
    if not w > 0:
        raise exception.DataInvalid("bin_width = %r must be positive." % (w,))
    if not _MIN_WIDTH <= w <= _MAX_WIDTH:
        raise exception.DataInvalid("bin_width = %r is not in [2^-40, 2^40] nm." % (w,))
    return w


def _cutoffs(radii, probe_radius, atoms):
    radii = np.asarray(radii)
    if radii.shape != (atoms,):
        raise exception.DataInvalid("radii has shape %s for %d atoms" % (radii.shape, atoms))
    try:
        cutoff = radii.astype(np.float64) + float(probe_radius)
    except (TypeError, ValueError):
        raise exception.DataInvalid("probe_radius and radii are numbers.")
    if not np.all((cutoff > 0) & (cutoff <= MAX_COORD)):
        raise exception.DataInvalid(
            "radius + probe_radius must be positive and finite for every atom.")
    return np.ascontiguousarray(cutoff)


def _check(rc):
    if rc == _lib.EK_ENOMEM:
        msg = _lib.load().ek_last_error().decode("utf-8", "replace")
        raise exception.InsufficientResourceError(msg)
    _lib.check(rc)


def _span_check(diag, w, what):
    """the bound of csrc/ek_dyes.hip: at most MAX_BINS bins per chunk"""
    if not diag < (MAX_BINS - 3) * w:
        raise exception.DataInvalid(
            "%s span %g nm, not below %d bin widths of %g nm." % (what, diag, MAX_BINS - 3, w))


def remove_touches_protein(coords, frame_xyz, radii, probe_radius=0.17, device=0):
    """The points of ``coords`` [n, 3] float32 farther than ``radius +
    probe_radius`` from every atom of ``frame_xyz`` [atoms, 3], in their order."""
    c = _cloud(coords, "coords")
    x, single = _frames_xyz(frame_xyz, "frame_xyz")
    if not single:
        raise exception.DataInvalid("frame_xyz is one frame, [atoms, 3].")
    x = np.ascontiguousarray(x[0])
    cutoff = _cutoffs(radii, probe_radius, len(x))
    keep = np.zeros(len(c), dtype=np.uint8)
    _check(_lib.load().ek_dyes_touches(int(device), _lib.f32p(x), len(x), _lib.f64p(cutoff),
                                       _lib.f32p(c), len(c), _lib.u8p(keep)))
    return c[keep.view(np.bool_)]


def _edges_probs(counts, w):
    nbins = len(counts)
    bin_edges = np.linspace(0, nbins * w, nbins + 1)
    return int_norm_hist(bin_edges, counts), bin_edges


def pairwise_distance_distribution(coords1, coords2, bin_width=0.1, device=0):
    """The distribution of all distances between two clouds [n, 3] float32:
    ``probs`` [bins] (integral one) and ``bin_edges`` [bins + 1]."""
    c1, c2 = _cloud(coords1, "coords1"), _cloud(coords2, "coords2")
    w = _width(bin_width)
    both = np.concatenate([c1, c2]).astype(np.float64)
    ext = both.max(axis=0) - both.min(axis=0)
    _span_check(np.sqrt(np.sum(ext * ext)) * (1 + 2.0 ** -16), w, "The clouds")
    nbins = ctypes.c_int32(0)
    counts = np.zeros(MAX_BINS, dtype=np.int64)
    _check(_lib.load().ek_dyes_pair_hist(int(device), _lib.f32p(c1), len(c1), _lib.f32p(c2),
                                         len(c2), w, ctypes.byref(nbins), _lib.i64p(counts)))
    return _edges_probs(counts[:nbins.value], w)


def _placement_span(Mt, rho):
    """per frame, the diagonal of the box that holds its four placements
    (dy_frame_diag of csrc/ek_dyes.hip)"""
    m = Mt.astype(np.float64)
    reach = rho * np.sqrt((m[..., 0:3] ** 2 + m[..., 3:6] ** 2) + m[..., 6:9] ** 2)
    t = m[..., 9:12]
    r = (reach + (np.abs(t) + reach) * 2.0 ** -20) * (1 + 2.0 ** -16)
    ext = (t + r).max(axis=1) - (t - r).min(axis=1)
    return np.sqrt(np.sum(ext * ext, axis=1))


_PLACEMENTS = ("dye1 on residue 0", "dye1 on residue 1", "dye2 on residue 0",
               "dye2 on residue 1")


def dye_distance_distribution(xyz, radii, dye1, dye2, backbones, probe_radius=0.2,
                              bin_width=0.1, n_procs=1, device=0, chunk_frames=None,
                              cluster_grid_points=False):
    """The distribution of distances between two dyes on two residues, per frame.

    Each cloud is placed on each residue, the points within ``radius +
    probe_radius`` of an atom are removed, and the distances dye1 on the first
    residue -- dye2 on the second and dye1 on the second -- dye2 on the first are
    histogrammed and averaged.

    Parameters
    ----------
    xyz : np.ndarray, shape=(frames, atoms, 3), float32
        Coordinates in nm.
    radii : array, shape=(atoms,)
        van der Waals radii in nm.
    dye1, dye2 : np.ndarray, shape=(n, 3), float32
        The dyes' point clouds (``load_dye``).
    backbones : int array, shape=(2, 3)
        The atom indices (n, ca, c) of the two labelled residues.
    probe_radius : float, default=0.2
    bin_width : float, default=0.1
    n_procs : ignored (the frames run as one device call per chunk).
    chunk_frames : int, default=None
        Frames of one upload; by default what fits the device.
    cluster_grid_points : bool
        Not available: True raises NotImplementedError.

    Returns
    -------
    probs, bin_edges : ra.RaggedArray, one row per frame
        What ``make_distribution`` takes.
    """
    global _label_ms
    if cluster_grid_points:
        raise NotImplementedError(
            "cluster_grid_points is not ported: the reference's choice among equally large "
            "clusters is not defined.")
    x, single = _frames_xyz(xyz)
    if single:
        raise exception.DataInvalid("xyz is [frames, atoms, 3].")
    x = np.ascontiguousarray(x)
    frames, atoms = x.shape[:2]
    if frames < 1:
        raise exception.DataInvalid("xyz holds no frames.")
    cutoff = _cutoffs(radii, probe_radius, atoms)
    d1, d2 = _cloud(dye1, "dye1"), _cloud(dye2, "dye2")
    b = _backbones(backbones, atoms, rows=2)
    w = _width(bin_width)
    if chunk_frames is None:
        chunk_frames = 0
    elif (isinstance(chunk_frames, bool) or not isinstance(chunk_frames, (int, np.integer))
          or not 1 <= chunk_frames <= MAX_CHUNK_FRAMES):
        raise exception.DataInvalid(
            "chunk_frames = %r is not in [1, %d]" % (chunk_frames, MAX_CHUNK_FRAMES))
    Mt = np.empty((frames, 2, 12), dtype=np.float32)
    for r in range(2):
        with np.errstate(invalid="ignore", divide="ignore"):
            M, t = determine_rot_mat(x, b[r])
        Mt[:, r, :9], Mt[:, r, 9:] = M.reshape(frames, 9), t
    bad = np.flatnonzero(~np.all(np.isfinite(Mt), axis=(1, 2)))
    if bad.size:
        raise exception.DataInvalid(
            "Frame %d: the N, CA and C of a labelled residue do not span a plane." % bad[0])
    rho = max(np.sqrt((c[:, 0] ** 2 + c[:, 1] ** 2) + c[:, 2] ** 2).max()
              for c in (d1.astype(np.float64), d2.astype(np.float64)))
    if frames:
        _span_check(_placement_span(Mt, rho).max(), w, "The placements of a frame")
    L = _lib.load()
    kept = np.zeros((frames, 4), dtype=np.int32)
    nbins = np.zeros((frames, 2), dtype=np.int32)
    h = ctypes.c_void_p()
    _check(L.ek_dyes_open(int(device), atoms, _lib.f64p(cutoff), len(d1), _lib.f32p(d1), len(d2),
                          _lib.f32p(d2), w, ctypes.byref(h)))
    try:
        _check(L.ek_dyes_run(h, _lib.f32p(x), frames, _lib.f32p(Mt), int(chunk_frames)))
        if frames:
            _check(L.ek_dyes_counts(h, frames, _lib.i32p(kept), _lib.i32p(nbins)))
        counts = np.zeros(int(nbins.sum()), dtype=np.int64)
        _check(L.ek_dyes_fetch(h, _lib.i64p(counts)))
        timing = np.zeros(4)
        _check(L.ek_dyes_last_timing(h, _lib.f64p(timing)))
        _label_ms = timing
    finally:
        L.ek_dyes_close(h)
    empty = np.argwhere(kept == 0)
    if len(empty):
        raise exception.DataInvalid(
            "Frame %d: every point of placement %d (%s) touches the protein."
            % (empty[0][0], empty[0][1], _PLACEMENTS[empty[0][1]]))
    probs, edges, end = [], [], np.cumsum(nbins.reshape(-1))
    for f in range(frames):
        pe = [_edges_probs(counts[end[2 * f + o] - nbins[f, o]:end[2 * f + o]], w)
              for o in range(2)]
        p, e = _merge_histograms([pe[0][0], pe[1][0]], [pe[0][1], pe[1][1]],
                                 weights=[0.5, 0.5])
        probs.append(p)
        edges.append(e)
    return ra.RaggedArray(probs), ra.RaggedArray(edges)


def last_labelling_timing():
    """Milliseconds between device events of the last ``dye_distance_distribution``,
    summed over its chunks of frames: uploads, touch and compaction kernels, histogram
    kernels, download (ek_dyes_last_timing)."""
    return _label_ms.copy()
