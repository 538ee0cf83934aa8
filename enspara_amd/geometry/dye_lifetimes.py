"""Donor-excitation Monte Carlo on dye MSMs (the reference's
enspara/geometry/dye_lifetimes.py) on the device: csrc/ek_dye_pair.hip, DESIGN.md 4m.

Every dye is a small MSM of its own conformations; every pair of a donor and an
acceptor conformation has its own kappa squared, distance and Forster radius
(``geometry.explicit_r0_calc``).  An excitation is a Markov chain: while the donor is
excited it picks a decay channel from the pair's probabilities over one lag time
(radiative, non-radiative, energy transfer, still excited), then both dyes hop.  It
yields a lifetime (steps times the lag time) and a channel.

A *problem* is one protein centre with its two dye MSMs (``problem(...)``); a
``DyePair`` holds one or a list of them and runs all their excitations in one device
call per chunk.  Sample ``j`` of problem ``p`` is chain ``first_chain + p 2^32 + j``
of the seed; what a chain draws depends on ``(seed, chain, index)`` alone (Philox, as
in ``msm.synthetic_data``), so results do not depend on ``step_cap``, on how many
problems a handle holds, on the chunking or on how the samples are split across calls.
Per chain: the initial states are the inverse CDF of the equilibrium probabilities
with doubles 0 of its donor and acceptor streams; step ``t`` takes the channel with
double ``t`` of its decay stream and hops with doubles ``t + 1`` of the donor and
acceptor streams (the hops after the decisive draw are the reference's own
behaviour: a trajectory has ``steps + 1`` states).  The static treatment of chain
``c`` sees the initial states of the Monte Carlo of chain ``c`` and flips double 0 of
its coin stream; the isotropic one flips the same coin.

Host (numpy, the reference's expressions): ``FRET_rate``,
``calc_dye_radiative_rates``, ``calc_energy_transfer_prob``, ``calc_per_state_FE``.

There is no topology reader here: where the reference takes ``md.Trajectory``
centres and dye names, these functions take ``coords [n_states, 9]``
(``explicit_r0_calc.dye_r_mu``) and ``dye_params = (J, Qd, Td)``.

Where this differs from the reference, on purpose:

* ``random_state`` reproduces a run, and every excitation has its own chain (the
  reference reseeds every excitation of a ``calc_lifetimes`` call with the same
  ``rng_seed``, which repeats one excitation ``n_samples`` times);
* ``R0^6 = 0.02108^6 k2 Qd J / n^4`` is computed directly, without the sixth root and
  power of the reference; ``r^6 = (r^2)(r^2)(r^2)``: probabilities differ from the
  reference's by rounding (DESIGN.md 4m has the bound);
* the isotropic treatment flips its coins against ``avg_FE``, the weighted mean it
  computes; the reference's ``fully_averaged_explict_dyes`` compares with the ``FE`` of
  the last pair of its loop, which is a bug;
* outcomes are int8 codes (``OUTCOMES``, ``outcome_names``); only ``calc_lifetimes``
  returns the reference's strings;
* ``make_dye_msm`` sets the equilibrium probability of a removed state to exactly 0
  (nothing enters it; the eigensolver leaves rounding noise there);
* ``n_procs`` is accepted and ignored; invalid input raises ``DataInvalid`` before any
  device call; a dye that has to hop from a state whose row is empty, or an
  excitation still excited after ``max_steps`` steps, raises ``DataInvalid``.

Bursts (csrc/ek_dye_bursts.hip).  ``calc_lifetimes_many`` gives a table of
``(lifetimes, outcomes)`` per protein state; ``sample_lifetime_bursts`` resamples it on
the protein MSM's time scale: a burst is a chain of the protein MSM (burst ``b`` is
chain ``b`` of the seed, exactly the chain of
``dyes_from_expt_dist.sample_FRET_histograms`` and of
``explicit_r0_calc.simulate_burst_k2``), and photon ``k`` of it draws one of the photon
events of the state the chain is in, with double ``k`` of the chain's event stream:
entry ``min(m - 1, int(u m))`` of the ``m`` photon events (``event_table``).
``sample_lifetimes_guarenteed_photon`` is one such burst,
``_sample_lifetimes_guarenteed_photon`` the draw alone on a list of states,
``extract_fret_efficiency_lifetimes`` and ``remake_prot_MSM_from_lifetimes`` the
reference's host steps, ``run_mc`` their composition (the reference's ``remake_msms``
is its first step).  On purpose different from the reference here:

* *seeding and chains*: one seed reproduces a run and every burst has its own chain; the
  reference seeds only the initial state and lets ``synthetic_trajectory`` and the
  event draws use other generators;
* *the rejection loop becomes one draw*: drawing uniformly among all events and
  redrawing the non-radiative ones is the same distribution as one uniform draw among
  the photon events, so the loop is gone; a state without a photon event (dyeless, or
  with non-radiative events only) raises ``DataInvalid`` naming it, where the
  reference fails or spins forever;
* ``remake_prot_MSM_from_lifetimes`` and ``run_mc`` take arrays and return arrays:
  messages go to ``logging``, no file is read or written, and a removed state's
  equilibrium probability is exactly 0, as in ``make_dye_msm``.

Labelling: ``explicit_r0_calc.map_dye_on_protein`` places a dye library on
a residue of every centre and finds the conformations to keep; ``centres_from_maps`` turns
a donor's and an acceptor's map into the list ``calc_lifetimes_many`` takes, so that
labelling -> lifetimes -> bursts is three calls.

Not ported: ``load_dye``, ``load_library``, ``get_dye_overlap`` (files, yaml, pandas); the
``curve_fit`` helpers (scipy on the host); the ``save_*`` file outputs.
"""
import collections
import ctypes
import logging

import numpy as np

from .. import _lib, exception, ra
from ..msm import builders
from ..msm import synthetic_data as sd
from . import dyes_from_expt_dist as dyes
from . import explicit_r0_calc as r0c

__all__ = ["FRET_rate", "calc_dye_radiative_rates", "calc_energy_transfer_prob",
           "calc_per_state_FE", "make_dye_msm", "OUTCOMES", "outcome_names", "problem",
           "geometry_problem", "DyePair", "resolve_excitations", "explicit_static_dyes",
           "fully_averaged_explicit_dyes", "calc_lifetimes", "calc_lifetimes_many",
           "centres_from_maps",
           "last_seed", "last_timing", "CHUNK_BYTES", "MAX_STEPS", "EventTable", "event_table",
           "sample_lifetime_bursts", "sample_lifetimes_guarenteed_photon",
           "_sample_lifetimes_guarenteed_photon", "pick_events",
           "extract_fret_efficiency_lifetimes", "remake_prot_MSM_from_lifetimes", "run_mc",
           "last_burst_timing", "burst_timing"]

_log = logging.getLogger(__name__)

OUTCOMES = ("radiative", "non_radiative", "energy_transfer")
#: device bytes of one call's problems and samples, above which a list is cut
CHUNK_BYTES = 1 << 30
#: steps after which an excitation that is still excited raises (the library's default)
MAX_STEPS = 1 << 20
_SAMPLE_BYTES = 32          # device bytes of a sample in a resolve call

#: the seed of the last call that drew chains (an int; None before the first)
last_seed = None


# ---- host ----------------------------------------------------------------------------------
def FRET_rate(r, R0, Td):
    """Rate of energy transfer, 1/ns: ``(1 / Td) (R0 / r)^6``."""
    return (1 / Td) * ((R0 / r)**6)


def calc_dye_radiative_rates(Qd, Td):
    """``(krad, k_non_rad)`` in 1/ns from the quantum yield and the donor lifetime."""
    krad = Qd / Td
    k_non_rad = (1 / Td) - krad
    return krad, k_non_rad


def calc_energy_transfer_prob(krad, k_non_rad, kRET, dt):
    """Probabilities over ``dt`` of radiative decay, non-radiative decay, energy
    transfer and of staying excited; where the last would be negative (dyes very
    close) it is 0 and the others are renormalised."""
    p_rad = 1 - np.exp(-krad * dt)
    p_nonrad = 1 - np.exp(-k_non_rad * dt)
    p_RET = 1 - np.exp(-kRET * dt)
    p_remain_excited = 1 - p_rad - p_nonrad - p_RET
    all_probs = np.array([p_rad, p_nonrad, p_RET, p_remain_excited], dtype=np.float64)
    if p_remain_excited < 0:
        all_probs = np.array([p_rad, p_nonrad, p_RET, 0.0], dtype=np.float64)
        all_probs = all_probs / all_probs.sum()
    return all_probs.flatten()


def calc_per_state_FE(events):
    """``events [n_states, 2, ...]`` (lifetimes and outcome strings per protein state,
    from ``calc_lifetimes``) -> the FRET efficiency per state: acceptor photons over
    all photons, NaN for a state that could not be labelled."""
    per_state = []
    for event in events[:, 1]:
        if len(event) == 0:
            per_state.append(np.nan)
        else:
            event = np.asarray(event)
            acceptors = np.count_nonzero(event == "energy_transfer")
            donors = np.count_nonzero(event == "radiative")
            per_state.append(acceptors / (donors + acceptors))
    return np.array(per_state)


def outcome_names(codes):
    """int8 codes -> an object array of the reference's strings"""
    return np.array(OUTCOMES, dtype=object)[np.asarray(codes, dtype=np.int64)]


def make_dye_msm(t_counts, keep, device=0):
    """The dye MSM of the states ``keep`` (the conformations that do not clash with
    the protein): the counts of every other state zeroed, row-normalised, with its
    equilibrium probabilities.  -> ``(tprobs, eqs, keep)``; with no state kept
    ``([0], [0], [])`` as the reference."""
    t_counts = np.asarray(t_counts)
    keep = np.asarray(keep, dtype=np.int64).reshape(-1)
    if t_counts.ndim != 2 or t_counts.shape[0] != t_counts.shape[1]:
        raise exception.DataInvalid("t_counts is square, not %s" % (t_counts.shape,))
    if len(keep) and (keep.min() < 0 or keep.max() >= len(t_counts)):
        raise exception.DataInvalid("keep holds states of [0, %d)" % len(t_counts))
    if len(keep) == 0:
        return np.array([0]), np.array([0]), np.array([])
    all_indices = np.arange(len(t_counts))
    bad = all_indices[~np.isin(all_indices, keep)]
    new_tcounts = r0c.remove_bad_states(bad, t_counts)
    _, tprobs, eqs = builders.normalize(new_tcounts, calculate_eq_probs=True, device=device)
    eqs = np.array(eqs, dtype=np.float64)
    eqs[bad] = 0.0      # (nothing enters a removed state: exactly 0, not the solver's rounding)
    return tprobs, eqs, keep


# ---- problems ------------------------------------------------------------------------------
Problem = collections.namedtuple(
    "Problem", ["nd", "na", "d_rows", "a_rows", "d_init", "a_init", "d_xyz", "a_xyz", "consts",
                "d_eqs", "a_eqs", "bytes"])


def _coords(coords, what):
    c = np.ascontiguousarray(coords, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != 9 or c.shape[0] < 1:
        raise exception.DataInvalid("%s coordinates are [n_states, 9], got %s" % (what, c.shape))
    if not np.all(np.isfinite(c)):
        raise exception.DataInvalid("%s coordinates are not finite." % what)
    if np.any(np.all(c[:, 6:9] == 0, axis=1)):
        raise exception.DataInvalid("A %s state has a zero dipole vector." % what)
    return c


def _eqs(eqs, n, what):
    e = np.ascontiguousarray(eqs, dtype=np.float64)
    if e.shape != (n,):
        raise exception.DataInvalid(
            "%s eq probs of shape %s do not fit %d states." % (what, e.shape, n))
    sd._check_entries(e, "%s eq probs" % what)
    sd._check_sums(np.array([e.sum()]), "The %s eq probs" % what)
    cdf = np.cumsum(e)
    return e, cdf / cdf[-1]


def _rows(tprobs, n, what):
    indptr, cols, cdf = sd.compress_rows(tprobs)
    if len(indptr) - 1 != n:
        raise exception.DataInvalid(
            "%s tprobs of %d states do not fit %d coordinates." % (what, len(indptr) - 1, n))
    return indptr, cols, cdf


def problem(d_coords, d_tprobs, d_eqs, a_coords, a_tprobs, a_eqs, dye_params, dye_lagtime,
            n=1.333):
    """Validate and pack one labelled centre.

    d_coords, a_coords : ``[n_states, 9]`` (``explicit_r0_calc.dye_r_mu``);
    d_tprobs, a_tprobs : row-normalised transition probabilities, dense or scipy sparse
    (rows of clashing states may be empty); d_eqs, a_eqs : equilibrium probabilities;
    dye_params : ``(J, Qd, Td)``; dye_lagtime : ns; n : refractive index.
    """
    d_xyz, a_xyz = _coords(d_coords, "donor"), _coords(a_coords, "acceptor")
    if (d_xyz[:, None, 3:6] == a_xyz[None, :, 3:6]).all(axis=2).any():
        raise exception.DataInvalid("A donor and an acceptor state share their dipole origin.")
    try:
        J, Qd, Td = (float(v) for v in dye_params)
        dt, n = float(dye_lagtime), float(n)
    except (TypeError, ValueError):
        raise exception.DataInvalid("dye_params is (J, Qd, Td), dye_lagtime a number")
    if not (Td > 0 and np.isfinite(Td)):
        raise exception.DataInvalid("Td > 0, got %r" % Td)
    if not 0 < Qd <= 1:
        raise exception.DataInvalid("Qd in (0, 1], got %r" % Qd)
    if not (dt > 0 and np.isfinite(dt)):
        raise exception.DataInvalid("dye_lagtime > 0, got %r" % dt)
    if not (J >= 0 and np.isfinite(J) and n > 0 and np.isfinite(n)):
        raise exception.DataInvalid("J >= 0 and n > 0, got %r, %r" % (J, n))
    nd, na = len(d_xyz), len(a_xyz)
    d_rows, a_rows = _rows(d_tprobs, nd, "donor"), _rows(a_tprobs, na, "acceptor")
    d_e, d_init = _eqs(d_eqs, nd, "donor")
    a_e, a_init = _eqs(a_eqs, na, "acceptor")
    krad, k_non_rad = calc_dye_radiative_rates(Qd, Td)
    consts = np.array([1 - np.exp(-krad * dt), 1 - np.exp(-k_non_rad * dt), dt,
                       R0_6_constant(Qd, J, n), 1 / Td, 0.0])
    size = sum((len(r[0]) + 1) * 8 + len(r[1]) * 12 for r in (d_rows, a_rows)) + \
        (nd + na) * 80 + 64
    return Problem(nd, na, d_rows, a_rows, d_init, a_init, d_xyz, a_xyz, consts, d_e, a_e, size)


def R0_6_constant(Qd, J, n=1.333):
    """``c6`` with ``R0^6 = c6 k2``: ``0.02108^6 Qd J / n^4``"""
    return r0c.R0_CONSTANT**6 * Qd * J / n**4


def geometry_problem(d_coords, a_coords, dye_params, dye_lagtime, n=1.333):
    """A problem for the pair table alone: the dyes do not move"""
    nd, na = len(np.atleast_2d(d_coords)), len(np.atleast_2d(a_coords))
    return problem(d_coords, np.eye(nd), np.full(nd, 1.0 / nd), a_coords, np.eye(na),
                   np.full(na, 1.0 / na), dye_params, dye_lagtime, n=n)


def _n_samples(n_samples):
    if isinstance(n_samples, bool) or not isinstance(n_samples, (int, np.integer)) or \
            not 1 <= n_samples < 2 ** 32:
        raise exception.DataInvalid("n_samples is an integer in [1, 2^32), got %r" % (n_samples,))
    return int(n_samples)


def _positive(v, what):
    if v is None:
        return 0
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise exception.DataInvalid("%s is an integer >= 1, got %r" % (what, v))
    return int(v)


class DyePair(object):
    """One problem or a list of problems (``problem(...)``), run on the device
    (``ek_dye_pair`` of include/enspara_hip.h).  Usable as a context manager; ``close``
    frees the device memory.

    A call cuts the list into chunks of at most ``chunk_bytes`` device bytes (the
    problems' arrays plus 32 bytes a sample; ``CHUNK_BYTES`` = 1 GiB unless given) and
    fewer than 2^31 samples; a chunk is one device call.  A list that fits one chunk
    stays resident between calls; otherwise every chunk is uploaded for its call and
    released after it.  Results do not depend on the chunking.
    """

    def __init__(self, problems, device=0, chunk_bytes=None):
        if isinstance(problems, Problem):
            problems = [problems]
        problems = list(problems)
        if not problems or not all(isinstance(p, Problem) for p in problems):
            raise exception.DataInvalid("problems: one or a list of problem(...)")
        self.problems = problems
        self.device = int(device)
        self.chunk_bytes = int(CHUNK_BYTES if chunk_bytes is None else chunk_bytes)
        if self.chunk_bytes < 1:
            raise exception.DataInvalid("chunk_bytes >= 1")
        self.last_seed = None
        self._L = None
        self._resident = None       # ((lo, hi), handle)

    # -- chunks and handles
    def _chunks(self, n_samples):
        out, lo, size = [], 0, 0
        for i, p in enumerate(self.problems):
            b = p.bytes + _SAMPLE_BYTES * n_samples
            if i > lo and (size + b > self.chunk_bytes or (i - lo + 1) * n_samples >= 2 ** 31):
                out.append((lo, i))
                lo, size = i, 0
            size += b
        out.append((lo, len(self.problems)))
        return out

    def _create(self, lo, hi):
        ps = self.problems[lo:hi]
        self._L = _lib.load()
        packed = []
        for side in ("d", "a"):
            counts = np.array([getattr(p, "n" + side) for p in ps], dtype=np.int64)
            off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            rows = [getattr(p, side + "_rows") for p in ps]
            nnz = np.concatenate([[0], np.cumsum([len(r[1]) for r in rows])]).astype(np.int64)
            indptr = np.concatenate([r[0][:-1] + nnz[k] for k, r in enumerate(rows)] +
                                    [nnz[-1:]]).astype(np.int64)
            cols = np.concatenate([r[1] + off[k] for k, r in enumerate(rows)]).astype(np.int32)
            cdf = np.ascontiguousarray(np.concatenate([r[2] for r in rows]), dtype=np.float64)
            init = np.ascontiguousarray(
                np.concatenate([getattr(p, side + "_init") for p in ps]), dtype=np.float64)
            xyz = np.ascontiguousarray(
                np.concatenate([getattr(p, side + "_xyz") for p in ps]), dtype=np.float64)
            packed += [off, indptr, cols, cdf, init, xyz]
        consts = np.ascontiguousarray(np.stack([p.consts for p in ps]), dtype=np.float64)
        h = ctypes.c_void_p()
        args = []
        for k in (0, 6):
            args += [_lib.i64p(packed[k]), _lib.i64p(packed[k + 1]), _lib.i32p(packed[k + 2]),
                     _lib.f64p(packed[k + 3]), _lib.f64p(packed[k + 4]), _lib.f64p(packed[k + 5])]
        _lib.check(self._L.ek_dye_pair_create(self.device, len(ps), *args, _lib.f64p(consts),
                                              ctypes.byref(h)))
        return h

    def _each_chunk(self, n_samples, fn):
        """fn(handle, lo, hi) for every chunk, in order"""
        chunks = self._chunks(n_samples)
        for lo, hi in chunks:
            if self._resident is not None and self._resident[0] == (lo, hi):
                fn(self._resident[1], lo, hi)
                continue
            self.close()
            h = self._create(lo, hi)
            if len(chunks) == 1:
                self._resident = ((lo, hi), h)
                fn(h, lo, hi)
            else:
                try:
                    fn(h, lo, hi)
                finally:
                    self._L.ek_dye_pair_destroy(h)

    def close(self):
        if self._resident is not None:
            self._L.ek_dye_pair_destroy(self._resident[1])
            self._resident = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- calls
    def _begin(self, n_samples, random_state, first_chain):
        global last_seed
        n = _n_samples(n_samples)
        if isinstance(first_chain, bool) or not isinstance(first_chain, (int, np.integer)) or \
                not 0 <= first_chain or first_chain + (len(self.problems) << 32) > 2 ** 59:
            raise exception.DataInvalid(
                "first_chain >= 0 and first_chain + n_problems 2^32 <= 2^59, got %r"
                % (first_chain,))
        seed = sd._seed(random_state)
        self.last_seed = last_seed = seed
        return n, seed, int(first_chain)

    def _raise_bad(self, lo, hi, bad):
        for side, g in zip(("donor", "acceptor"), bad):
            if g >= 0:
                counts = [getattr(p, "n" + side[0]) for p in self.problems[lo:hi]]
                off = np.concatenate([[0], np.cumsum(counts)])
                p = int(np.searchsorted(off, g, side="right")) - 1
                raise exception.DataInvalid(
                    "The %s of problem %d stood on state %d, whose row of tprobs has no "
                    "nonzero entry, and had to hop." % (side, lo + p, g - off[p]))

    def resolve(self, n_samples, random_state=None, first_chain=0, return_trajectories=False,
                step_cap=None, max_steps=None):
        """``n_samples`` excitations of every problem.

        Returns ``steps`` int64 ``[P, n_samples]`` and ``outcomes`` int8 ``[P,
        n_samples]`` (indices into ``OUTCOMES``); with ``return_trajectories`` also two
        RaggedArrays of ``P * n_samples`` rows (sample after sample, problem after
        problem), the donor's and the acceptor's states, ``steps + 1`` each.

        step_cap : steps per kernel launch; after every launch the finished
            excitations leave the list.  The library's default (65536) is longer than
            any excitation measured, so that a call is one launch: a call lasts as
            long as its longest excitation and compacting did not pay.
        max_steps : an excitation still excited after so many steps raises
            ``DataInvalid`` (``MAX_STEPS`` = 2^20 if left out; below 2^24).
        Neither changes a result.
        """
        n, seed, first = self._begin(n_samples, random_state, first_chain)
        cap, most = _positive(step_cap, "step_cap"), _positive(max_steps, "max_steps")
        if most >= 2 ** 24:
            raise exception.DataInvalid("max_steps < 2^24, got %d" % most)
        P = len(self.problems)
        steps = np.zeros((P, n), dtype=np.int32)
        outcomes = np.zeros((P, n), dtype=np.int8)
        dparts, aparts = [], []
        null = ctypes.cast(None, ctypes.POINTER(ctypes.c_int32))

        def run(h, lo, hi):
            s = np.zeros((hi - lo) * n, dtype=np.int32)
            o = np.zeros((hi - lo) * n, dtype=np.int8)
            bad, over = (ctypes.c_int64 * 2)(-1, -1), ctypes.c_int64(-1)
            chain0 = first + (lo << 32)
            _lib.check(self._L.ek_dye_pair_resolve(h, seed, chain0, n, cap, most, _lib.i32p(s),
                                                   _lib.i8p(o), null, null, 0, bad,
                                                   ctypes.byref(over)))
            self._raise_bad(lo, hi, bad)
            if over.value >= 0:
                p, j = divmod(over.value, n)
                raise exception.DataInvalid(
                    "Sample %d of problem %d (chain %d) is still excited after %d steps."
                    % (j, lo + p, chain0 + (p << 32) + j, most or MAX_STEPS))
            steps[lo:hi] = s.reshape(hi - lo, n)
            outcomes[lo:hi] = o.reshape(hi - lo, n)
            if return_trajectories:
                cells = int(s.astype(np.int64).sum()) + len(s)
                dt, at = np.empty(cells, dtype=np.int32), np.empty(cells, dtype=np.int32)
                _lib.check(self._L.ek_dye_pair_resolve(h, seed, chain0, n, cap, most,
                                                       _lib.i32p(s), _lib.i8p(o), _lib.i32p(dt),
                                                       _lib.i32p(at), cells, bad,
                                                       ctypes.byref(over)))
                self._raise_bad(lo, hi, bad)
                dparts.append(dt)
                aparts.append(at)

        self._each_chunk(n, run)
        steps = steps.astype(np.int64)
        if not return_trajectories:
            return steps, outcomes
        lengths = (steps + 1).reshape(-1)
        return (steps, outcomes,
                ra.RaggedArray(np.concatenate(dparts), lengths=lengths, copy=False),
                ra.RaggedArray(np.concatenate(aparts), lengths=lengths, copy=False))

    def _static(self, n, seed, first, fe_fixed):
        P = len(self.problems)
        acc = np.zeros((P, n), dtype=np.int8)
        ds, as_ = np.zeros((P, n), dtype=np.int32), np.zeros((P, n), dtype=np.int32)

        def run(h, lo, hi):
            a = np.zeros((hi - lo) * n, dtype=np.int8)
            d, c = np.zeros(len(a), dtype=np.int32), np.zeros(len(a), dtype=np.int32)
            fe = ctypes.cast(None, ctypes.POINTER(ctypes.c_double))
            if fe_fixed is not None:
                keep = np.ascontiguousarray(fe_fixed[lo:hi], dtype=np.float64)
                fe = _lib.f64p(keep)
            _lib.check(self._L.ek_dye_pair_static(h, seed, first + (lo << 32), n, fe,
                                                  _lib.i8p(a), _lib.i32p(d), _lib.i32p(c)))
            acc[lo:hi], ds[lo:hi], as_[lo:hi] = (x.reshape(hi - lo, n) for x in (a, d, c))

        self._each_chunk(n, run)
        return acc, ds, as_

    def static(self, n_samples, random_state=None, first_chain=0, return_states=False):
        """The dyes do not move: every sample takes the initial states of its chain and
        is an acceptor photon iff its coin is ``<=`` the pair's FE.  -> ``outcomes``
        int8 ``[P, n_samples]`` (0 radiative, 2 energy transfer); with
        ``return_states`` also the donor and acceptor states."""
        n, seed, first = self._begin(n_samples, random_state, first_chain)
        acc, ds, as_ = self._static(n, seed, first, None)
        out = (acc * 2).astype(np.int8)
        return (out, ds, as_) if return_states else out

    def pair_table(self, problem=0):
        """``(k2, r, FE [nd, na], decay cdf [nd, na, 3])`` of one problem"""
        problem = int(problem)
        if not 0 <= problem < len(self.problems):
            raise exception.DataInvalid("no problem %d" % problem)
        p = self.problems[problem]
        k2, r, FE = (np.empty((p.nd, p.na)) for _ in range(3))
        cdf = np.empty((p.nd, p.na, 3))
        # (the resident chunk if it holds the problem, else the problem alone)
        if self._resident is not None and \
                self._resident[0][0] <= problem < self._resident[0][1]:
            h, own, lo = self._resident[1], False, self._resident[0][0]
        else:
            h, own, lo = self._create(problem, problem + 1), True, problem
        try:
            _lib.check(self._L.ek_dye_pair_table(h, problem - lo, _lib.f64p(k2), _lib.f64p(r),
                                                 _lib.f64p(FE), _lib.f64p(cdf)))
        finally:
            if own:
                self._L.ek_dye_pair_destroy(h)
        return k2, r, FE, cdf

    def isotropic(self, n_samples, random_state=None, first_chain=0):
        """The dyes are averaged out: per problem the FE of every pair of states with
        nonzero eq prob (donor-major, the reference's order), their weighted mean
        ``avg_FE``, and ``n_samples`` coins against it.  -> a list over the problems of
        ``(transfers int8 [n_samples] (0 radiative, 2 energy transfer), k2s, FEs, eqs,
        avg_FE)``."""
        n, seed, first = self._begin(n_samples, random_state, first_chain)
        per = []
        for k, p in enumerate(self.problems):
            k2, _, FE, _ = self.pair_table(k)
            ds, as_ = np.where(p.d_eqs != 0)[0], np.where(p.a_eqs != 0)[0]
            sel = np.ix_(ds, as_)
            eqs = (p.d_eqs[ds][:, None] * p.a_eqs[as_][None, :]).reshape(-1)
            FEs = FE[sel].reshape(-1)
            per.append((k2[sel].reshape(-1), FEs, eqs, float(np.average(FEs, weights=eqs))))
        acc, _, _ = self._static(n, seed, first, np.array([q[3] for q in per]))
        return [((acc[k] * 2).astype(np.int8),) + per[k] for k in range(len(per))]


# ---- the reference's functions -------------------------------------------------------------
def _pair(d_tprobs, a_tprobs, d_eqs, a_eqs, d_coords, a_coords, dye_params, dye_lagtime, device):
    return DyePair(problem(d_coords, d_tprobs, d_eqs, a_coords, a_tprobs, a_eqs, dye_params,
                           dye_lagtime), device=device)


def resolve_excitations(d_tprobs, a_tprobs, d_eqs, a_eqs, d_coords, a_coords, dye_params,
                        dye_lagtime, n_samples=1, random_state=None, first_chain=0,
                        return_trajectories=True, device=0):
    """The batch form of the reference's ``resolve_excitation``: ``n_samples``
    excitations of one labelled centre.  -> ``(steps int64 [n], outcomes int8 [n])`` and,
    with ``return_trajectories``, the donor's and the acceptor's states as
    RaggedArrays of ``n`` rows."""
    with _pair(d_tprobs, a_tprobs, d_eqs, a_eqs, d_coords, a_coords, dye_params, dye_lagtime,
               device) as pair:
        out = pair.resolve(n_samples, random_state=random_state, first_chain=first_chain,
                           return_trajectories=return_trajectories)
    return (out[0][0], out[1][0]) + tuple(out[2:])


def _identity(n):
    return np.eye(n)


def explicit_static_dyes(d_eqs, a_eqs, d_coords, a_coords, dye_params, n_samples=1000,
                         random_state=None, first_chain=0, device=0):
    """Static dyes drawn from their equilibrium probabilities -> ``outcomes`` int8
    ``[n_samples]`` (0 radiative, 2 energy transfer); the lifetimes are 0."""
    nd, na = len(np.atleast_1d(d_eqs)), len(np.atleast_1d(a_eqs))
    with _pair(_identity(nd), _identity(na), d_eqs, a_eqs, d_coords, a_coords, dye_params, 1.0,
               device) as pair:
        return pair.static(n_samples, random_state=random_state, first_chain=first_chain)[0]


def fully_averaged_explicit_dyes(d_eqs, a_eqs, d_coords, a_coords, dye_params, n_samples=1000,
                                 random_state=None, first_chain=0, device=0):
    """The reference's ``fully_averaged_explict_dyes`` -> ``[lifetimes (zeros),
    transfers int8, k2s, FEs, eqs]``, the coins flipped against the weighted mean of
    ``FEs`` (see the head of this module)."""
    nd, na = len(np.atleast_1d(d_eqs)), len(np.atleast_1d(a_eqs))
    with _pair(_identity(nd), _identity(na), d_eqs, a_eqs, d_coords, a_coords, dye_params, 1.0,
               device) as pair:
        transfers, k2s, FEs, eqs, _ = pair.isotropic(
            n_samples, random_state=random_state, first_chain=first_chain)[0]
    return [np.zeros(len(transfers), dtype=np.int64), transfers, k2s, FEs, eqs]


_TREATMENTS = ("Monte-carlo", "static", "isotropic")


def calc_lifetimes_many(centres, dye_params, dye_lagtime, n_samples=1000,
                        dye_treatment="Monte-carlo", random_state=None, n_procs=1, device=0,
                        chunk_bytes=None):
    """``calc_lifetimes`` over a list of protein centres, all in one ``DyePair``.

    centres : list of ``(d_coords, d_tcounts, d_keep, a_coords, a_tcounts, a_keep)``.
    -> a list of ``(lifetimes, outcomes)``, ``([], [])`` for a centre one of whose dyes
    keeps no state.  Centre ``i`` uses the chains ``i 2^32 + j`` whether or not other
    centres could be labelled.  ``n_procs`` is ignored.
    """
    if dye_treatment not in _TREATMENTS:
        raise exception.DataInvalid("dye_treatment is one of %s" % (_TREATMENTS,))
    n = _n_samples(n_samples)
    seed = sd._seed(random_state)
    results, problems, where = [([], [])] * len(centres), [], []
    for i, (d_coords, d_tcounts, d_keep, a_coords, a_tcounts, a_keep) in enumerate(centres):
        d_tprobs, d_eqs, _ = make_dye_msm(d_tcounts, d_keep, device=device)
        a_tprobs, a_eqs, _ = make_dye_msm(a_tcounts, a_keep, device=device)
        if np.sum(a_eqs) == 0 or np.sum(d_eqs) == 0:
            continue
        problems.append(problem(d_coords, d_tprobs, d_eqs, a_coords, a_tprobs, a_eqs, dye_params,
                                dye_lagtime))
        where.append(i)
    # runs of consecutive centres keep their chain numbers: first_chain = first centre 2^32
    k = 0
    while k < len(where):
        m = k
        while m + 1 < len(where) and where[m + 1] == where[m] + 1:
            m += 1
        with DyePair(problems[k:m + 1], device=device, chunk_bytes=chunk_bytes) as pair:
            first = where[k] << 32
            if dye_treatment == "Monte-carlo":
                steps, codes = pair.resolve(n, random_state=seed, first_chain=first)
            elif dye_treatment == "static":
                codes = pair.static(n, random_state=seed, first_chain=first)
                steps = np.zeros(codes.shape, dtype=np.int64)
            else:
                codes = np.stack([q[0] for q in pair.isotropic(n, random_state=seed,
                                                               first_chain=first)])
                steps = np.zeros(codes.shape, dtype=np.int64)
        for q in range(k, m + 1):
            results[where[q]] = (np.array(steps[q - k], dtype=float) * dye_lagtime,
                                 outcome_names(codes[q - k]))
        k = m + 1
    return results


def centres_from_maps(d_map, d_tcounts, a_map, a_tcounts):
    """The ``centres`` of ``calc_lifetimes_many`` from a donor's and an acceptor's
    ``explicit_r0_calc.DyeMap`` of the same protein centres and the transition counts of
    the two dye MSMs (one state per conformation of the dye library): per centre
    ``(d_coords_all, d_tcounts, d_kept, a_coords_all, a_tcounts, a_kept)``."""
    for m, what in ((d_map, "d_map"), (a_map, "a_map")):
        if not all(hasattr(m, f) for f in ("coords_all", "kept")):
            raise exception.DataInvalid("%s is what map_dye_on_protein returns." % what)
    if len(d_map.kept) != len(a_map.kept):
        raise exception.DataInvalid(
            "The donor's map has %d centres, the acceptor's %d."
            % (len(d_map.kept), len(a_map.kept)))
    for m, t, what in ((d_map, d_tcounts, "donor"), (a_map, a_tcounts, "acceptor")):
        shape = np.shape(t) if not hasattr(t, "shape") else t.shape
        n = m.coords_all.shape[1]
        if tuple(shape) != (n, n):
            raise exception.DataInvalid(
                "The %s's t_counts are %s; its library has %d conformations." % (what, shape, n))
    return [(d_map.coords_all[p], d_tcounts, d_map.kept[p],
             a_map.coords_all[p], a_tcounts, a_map.kept[p]) for p in range(len(d_map.kept))]


def calc_lifetimes(d_coords, d_tcounts, d_keep, a_coords, a_tcounts, a_keep, dye_params,
                   dye_lagtime, n_samples=1000, dye_treatment="Monte-carlo", random_state=None,
                   device=0):
    """Dye-emission events of one protein centre.

    d_coords, a_coords : ``[n_states, 9]`` of the dyes aligned to their residues;
    d_tcounts, a_tcounts : transition counts of the dye MSMs; d_keep, a_keep : the
    states that do not clash with the protein; dye_params : ``(J, Qd, Td)``;
    dye_treatment : 'Monte-carlo', 'static' or 'isotropic'.

    Returns ``(lifetimes = steps * dye_lagtime in ns, outcomes as the reference's
    strings)``, ``([], [])`` when either dye keeps no state.
    """
    return calc_lifetimes_many([(d_coords, d_tcounts, d_keep, a_coords, a_tcounts, a_keep)],
                               dye_params, dye_lagtime, n_samples=n_samples,
                               dye_treatment=dye_treatment, random_state=random_state,
                               device=device)[0]


def last_timing():
    """Milliseconds between device events of the last device call: upload, kernels,
    download."""
    ms = np.zeros(3)
    _lib.check(_lib.load().ek_dye_pair_last_timing(_lib.f64p(ms)))
    return ms


# ---- bursts on the protein MSM (csrc/ek_dye_bursts.hip) ------------------------
EventTable = collections.namedtuple("EventTable", ["off", "life", "flag", "counts", "n_events"])
_CODE_OF = {name: k for k, name in enumerate(OUTCOMES)}
_MAX_PICK = 2 ** 31 - 1       # entries of a state's list: pick(u, m) takes m < 2^31


def _outcome_codes(outcomes, state):
    o = np.asarray(outcomes)
    if o.ndim != 1:
        raise exception.DataInvalid("The outcomes of state %d are not a 1-D list." % state)
    if o.size == 0:
        return np.zeros(0, dtype=np.int8)
    if np.issubdtype(o.dtype, np.integer):
        codes = o
    else:
        try:
            codes = np.array([_CODE_OF[str(x)] for x in o], dtype=np.int8)
        except KeyError as e:
            raise exception.DataInvalid(
                "State %d has the outcome %s; outcomes are %s or their codes 0, 1, 2."
                % (state, e, ", ".join(OUTCOMES)))
    if codes.min() < 0 or codes.max() > 2:
        raise exception.DataInvalid(
            "State %d has an outcome code outside 0, 1, 2 (%s)." % (state, ", ".join(OUTCOMES)))
    return codes.astype(np.int8)


def event_table(events):
    """Compact the events of every protein state to its photon events.

    events : a list over protein states of ``(lifetimes, outcomes)`` as
        ``calc_lifetimes_many`` returns them (outcomes the reference's strings or int8
        codes; ``([], [])`` a dyeless state), or an ``[n_states, 2]`` object array.

    Returns ``EventTable(off int64 [n + 1], life float64, flag uint8, counts, n_events)``:
    state ``s`` owns ``off[s]:off[s + 1]``, its radiative (flag 0) and energy-transfer
    (flag 1) events in the list's own order, the non-radiative ones dropped;
    ``counts[s]`` of them out of ``n_events[s]`` events in all.
    """
    if isinstance(events, EventTable):
        return events
    try:
        rows = [tuple(ev) for ev in events]
    except TypeError:
        raise exception.DataInvalid("events is a list of (lifetimes, outcomes) per state.")
    if not rows or any(len(ev) != 2 for ev in rows):
        raise exception.DataInvalid("events is a non-empty list of (lifetimes, outcomes).")
    lifes, flags, counts, totals = [], [], [], []
    for s, (lifetimes, outcomes) in enumerate(rows):
        try:
            life = np.asarray(lifetimes, dtype=np.float64)
        except (TypeError, ValueError):
            raise exception.DataInvalid("The lifetimes of state %d are not numbers." % s)
        codes = _outcome_codes(outcomes, s)
        if life.ndim != 1 or len(life) != len(codes):
            raise exception.DataInvalid(
                "State %d has lifetimes of shape %s for %d outcomes."
                % (s, life.shape, len(codes)))
        if not np.all(np.isfinite(life)):
            raise exception.DataInvalid("The lifetimes of state %d are not finite." % s)
        photon = codes != 1
        if photon.sum() > _MAX_PICK:
            raise exception.DataInvalid("State %d has 2^31 photon events or more." % s)
        lifes.append(life[photon])
        flags.append((codes[photon] == 2).astype(np.uint8))
        counts.append(int(photon.sum()))
        totals.append(len(codes))
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return EventTable(off, np.ascontiguousarray(np.concatenate(lifes), dtype=np.float64),
                      np.ascontiguousarray(np.concatenate(flags), dtype=np.uint8),
                      np.asarray(counts, dtype=np.int64), np.asarray(totals, dtype=np.int64))


def _table_for(events, n_states):
    table = event_table(events)
    if len(table.counts) != n_states:
        raise exception.DataInvalid(
            "events of %d states do not fit %d protein states." % (len(table.counts), n_states))
    return table


def _raise_no_event(table, state):
    if state >= 0:
        raise exception.DataInvalid(
            "A photon was emitted in state %d, which has %s." % (
                state, "no event at all (a dyeless state)" if table.n_events[state] == 0
                else "only non-radiative events, so no photon event to draw"))


# Bounds on one device call's buffers, as in dyes_from_expt_dist (a call lasts as long as its
# longest burst, however few bursts it holds): 4 GiB of trajectories, 2^27 photons.
_TRAJ_CELLS = 1 << 30
_PHOTONS = 1 << 27
_burst_ms = np.zeros(3)


def _chain(chain, what="chain"):
    if isinstance(chain, bool) or not isinstance(chain, (int, np.integer)) or \
            not 0 <= chain < 2 ** 60:
        raise exception.DataInvalid("%s is an integer in [0, 2^60), got %r" % (what, chain))
    return int(chain)


def _null(t):
    return ctypes.cast(None, ctypes.POINTER(t))


def _run_bursts(sampler, populations, MSM_frames, random_state, return_trajectories, step_cap,
                outputs, call, first_burst=0):
    """The chunk loop of every explicit-dye burst sampler: cuts the bursts into device
    calls within ``_PHOTONS`` and ``_TRAJ_CELLS``.

    outputs : list of dtypes of the per-photon outputs after the flag byte
    call(L, h, seed, b0, nb, sub_off, sub_frames, pop, cap, [flags, *outs], traj) -> None
        one device call on bursts ``first_burst + b0 ..``; it raises what its rule flags

    -> (foff, [flags uint8, *outputs] flat, trajs or None)
    """
    n = sampler.n_states
    pop = dyes._pop_cdf(populations, n)
    foff, frames = dyes._frames(MSM_frames)
    cap = _positive(step_cap, "step_cap")
    first = _chain(first_burst, "first burst")
    n_bursts = len(foff) - 1
    if first + n_bursts > 2 ** 60:
        raise exception.DataInvalid("chains below 2^60")
    seed = sd._seed(random_state)
    sampler.last_seed = seed
    global last_seed
    last_seed = seed
    lasts = frames[foff[1:] - 1]
    flat = [np.empty(len(frames), dtype=np.uint8)] + \
        [np.empty(len(frames), dtype=t) for t in outputs]
    trajs = np.empty(n_bursts, dtype=object) if return_trajectories else None
    h = sampler._handle()
    L = sampler._L
    _burst_ms[:] = 0
    b0 = 0
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
        subs = [a[foff[b0]:foff[b1]] for a in flat]
        traj = np.empty(int(cells[b1 - b0 - 1]), dtype=np.int32) if return_trajectories else None
        call(L, h, seed, first + b0, b1 - b0, sub_off, sub_frames, pop, cap, subs,
             _lib.i32p(traj) if traj is not None else _null(ctypes.c_int32))
        _burst_ms[:] += last_burst_timing()
        if return_trajectories:
            ends = cells[:b1 - b0]
            for i in range(b1 - b0):
                trajs[b0 + i] = traj[ends[i] - lasts[b0 + i] - 1:ends[i]]
        b0 = b1
    return foff, flat, trajs


def _lifetime_call(table):
    def call(L, h, seed, b0, nb, sub_off, sub_frames, pop, cap, subs, traj):
        bad_row, bad_state = ctypes.c_int64(-1), ctypes.c_int64(-1)
        _lib.check(L.ek_dye_bursts_lifetimes(
            h, seed, b0, nb, _lib.i64p(sub_off), _lib.i64p(sub_frames), _lib.f64p(pop),
            _lib.i64p(table.off), _lib.f64p(table.life), _lib.u8p(table.flag), cap,
            _lib.u8p(subs[0]), _lib.f64p(subs[1]), _lib.i32p(subs[2]), traj,
            ctypes.byref(bad_row), ctypes.byref(bad_state)))
        sd._raise_bad_row(bad_row.value)
        _raise_no_event(table, bad_state.value)
    return call


def _ragged(flat, foff):
    return ra.RaggedArray(flat, lengths=np.diff(foff), copy=False)


def sample_lifetime_bursts(T, populations, events, MSM_frames, random_state=None,
                           return_trajectories=False, device=0, step_cap=None):
    """Bursts of photons with lifetimes: every burst runs a chain of the protein MSM and,
    at every frame of ``MSM_frames``, draws one of the photon events of the state the
    chain is in (the batch form of the reference's ``sample_lifetimes_guarenteed_photon``).

    T : array or scipy sparse matrix, or a ``synthetic_data.Sampler``
    populations : array, shape=(n_states,); every burst's chain starts from a draw of them
    events : what ``calc_lifetimes_many`` returns, or an ``event_table`` of it
    MSM_frames : list of lists, per burst the frames of its photons

    Returns ``(photons uint8, lifetimes float64, states int32)``, RaggedArrays of a row
    per burst (1: acceptor photon, 0: donor photon; the lifetime of the event drawn; the
    state the chain was in), and with ``return_trajectories`` the chains as an object
    array of int32 arrays.  Burst ``b`` is chain ``b`` of the seed: the chain of
    ``dyes_from_expt_dist.sample_FRET_histograms`` and of ``simulate_burst_k2``.
    """
    sampler, own = sd._sampler(T, device)
    try:
        table = _table_for(events, sampler.n_states)
        foff, flat, trajs = _run_bursts(
            sampler, populations, MSM_frames, random_state, return_trajectories, step_cap,
            [np.float64, np.int32], _lifetime_call(table))
    finally:
        if own:
            sampler.close()
    out = tuple(_ragged(a, foff) for a in flat)
    return out + (trajs,) if return_trajectories else out


def sample_lifetimes_guarenteed_photon(frames, t_probs, eqs, lifetimes, outcomes, rng_seed=None,
                                       chain=0, device=0):
    """One burst: ``(photons, lifetimes, trj[frames])`` for the frames of its photons
    (the reference's signature; ``lifetimes``, ``outcomes``: per protein state).  It is
    burst ``chain`` of ``sample_lifetime_bursts`` with the same seed."""
    sampler, own = sd._sampler(t_probs, device)
    try:
        table = _table_for(list(zip(lifetimes, outcomes)), sampler.n_states)
        _, flat, _ = _run_bursts(sampler, eqs, [frames], rng_seed, False, None,
                                 [np.float64, np.int32], _lifetime_call(table),
                                 first_burst=chain)
    finally:
        if own:
            sampler.close()
    return flat[0], flat[1], flat[2]


def _sample_lifetimes_guarenteed_photon(states, lifetimes, outcomes, rng_seed=None, chain=0,
                                        device=0):
    """A photon event for every entry of ``states`` -> ``(photons uint8, lifetimes)``.
    Entry *k* draws what photon *k* of burst ``chain`` draws."""
    table = event_table(list(zip(lifetimes, outcomes)))
    s = sd._states(states, len(table.counts), "states")
    chain = _chain(chain)
    global last_seed
    last_seed = seed = sd._seed(rng_seed)
    photons, life = np.empty(len(s), dtype=np.uint8), np.empty(len(s))
    bad = ctypes.c_int64(-1)
    _lib.check(_lib.load().ek_dye_photons_lifetimes(
        int(device), seed, chain, len(s), _lib.i32p(s), len(table.counts), _lib.i64p(table.off),
        _lib.f64p(table.life), _lib.u8p(table.flag), _lib.u8p(photons), _lib.f64p(life),
        ctypes.byref(bad)))
    _raise_no_event(table, bad.value)
    return photons, life


def pick_events(table, states, u, device=0):
    """The pick of the lifetime rule with the caller's own doubles ``u`` in [0, 1): for
    every entry the index ``min(m - 1, int(u m))`` among the ``m`` photon events of its
    state (``table``: an ``event_table`` or events).  -> int64 array."""
    table = event_table(table)
    shape = np.shape(states)
    s = sd._states(states, len(table.counts), "states")
    u = np.ascontiguousarray(np.asarray(u, dtype=np.float64).reshape(-1))
    if u.shape != s.shape:
        raise exception.DataInvalid("%d doubles for %d states" % (len(u), len(s)))
    if not np.all((u >= 0) & (u < 1)):
        raise exception.DataInvalid("u must lie in [0, 1).")
    out = np.empty(len(s), dtype=np.int64)
    bad = ctypes.c_int64(-1)
    _lib.check(_lib.load().ek_dye_pick_events(
        int(device), len(s), _lib.i32p(s), _lib.f64p(u), len(table.counts),
        _lib.i64p(table.off), _lib.i64p(out), ctypes.byref(bad)))
    _raise_no_event(table, bad.value)
    return out.reshape(shape)


def extract_fret_efficiency_lifetimes(lifetime_samples):
    """``(FEs, d_lifetimes, a_lifetimes)`` of bursts: per burst the share of acceptor
    photons and the lifetimes behind its donor and its acceptor photons (object arrays of
    a float array per burst).

    lifetime_samples : per burst ``(photons, lifetimes, ...)`` as repeated calls of
        ``sample_lifetimes_guarenteed_photon`` give them, or the tuple of RaggedArrays
        ``sample_lifetime_bursts`` returns.
    """
    if isinstance(lifetime_samples, tuple) and len(lifetime_samples) >= 2 and \
            all(isinstance(x, ra.RaggedArray) for x in lifetime_samples[:2]):
        bursts = list(zip(lifetime_samples[0], lifetime_samples[1]))
    else:
        try:
            bursts = [(b[0], b[1]) for b in lifetime_samples]
        except (TypeError, IndexError):
            raise exception.DataInvalid(
                "lifetime_samples is a list of (photons, lifetimes) per burst.")
    if not bursts:
        raise exception.DataInvalid("No bursts were given.")
    FEs = np.empty(len(bursts))
    d_lifetimes, a_lifetimes = (np.empty(len(bursts), dtype=object) for _ in range(2))
    for i, (photons, life) in enumerate(bursts):
        photons, life = np.asarray(photons), np.asarray(life, dtype=np.float64)
        if photons.ndim != 1 or photons.shape != life.shape or photons.size == 0:
            raise exception.DataInvalid(
                "Burst %d has photons of shape %s and lifetimes of shape %s."
                % (i, photons.shape, life.shape))
        FEs[i] = np.sum(photons) / len(photons)
        d_lifetimes[i] = life[np.where(photons == 0)[0]]
        a_lifetimes[i] = life[np.where(photons == 1)[0]]
    return FEs, d_lifetimes, a_lifetimes


def remake_prot_MSM_from_lifetimes(lifetimes, prot_tcounts, prot_eqs=None, device=0):
    """The protein MSM without the states that could not be labelled (those whose entry
    of ``lifetimes`` is empty): their rows and columns of the counts zeroed,
    row-normalised.  -> ``(new_tprobs, new_eqs)``; the equilibrium probability of a
    removed state is exactly 0, so no burst starts there.  Messages go to ``logging``;
    nothing is written."""
    prot_tcounts = np.asarray(prot_tcounts)
    if prot_tcounts.ndim != 2 or prot_tcounts.shape[0] != prot_tcounts.shape[1]:
        raise exception.DataInvalid("prot_tcounts is square, not %s" % (prot_tcounts.shape,))
    n = len(prot_tcounts)
    try:
        n_rows = len(lifetimes)
    except TypeError:
        raise exception.DataInvalid("lifetimes is a list of lifetimes per protein state.")
    if n_rows != n:
        raise exception.DataInvalid("lifetimes of %d states do not fit %d protein states."
                                    % (n_rows, n))
    if prot_eqs is not None:
        prot_eqs = np.asarray(prot_eqs, dtype=np.float64)
        if prot_eqs.shape != (n,):
            raise exception.DataInvalid(
                "prot_eqs of shape %s do not fit %d states." % (prot_eqs.shape, n))
    bad = np.asarray(r0c.find_dyeless_states(lifetimes), dtype=np.int64)
    if len(bad) == n:
        raise exception.DataInvalid("No protein state could be labelled.")
    _log.info("%d of %d protein states had steric clashes.", len(bad), n)
    if len(bad) / n > 0.2:
        _log.warning("Labeling lost %d%% of the MSM states.", round(100 * len(bad) / n))
    if prot_eqs is not None and len(bad):
        lost = float(np.sum(prot_eqs[bad]))
        _log.info("This was %.2f%% of the original equilibrium probability.", 100 * lost)
        if lost > 0.2:
            _log.warning("Lots of equilibrium probability lost.")
    trimmed = r0c.remove_bad_states(bad, prot_tcounts)
    _, new_tprobs, new_eqs = builders.normalize(trimmed, calculate_eq_probs=True, device=device)
    new_eqs = np.array(new_eqs, dtype=np.float64)
    new_eqs[bad] = 0.0      # (nothing enters a removed state: exactly 0, not the solver's rounding)
    return new_tprobs, new_eqs


def run_mc(events, prot_tcounts, MSM_frames, prot_eqs=None, random_state=None,
           return_trajectories=False, device=0, step_cap=None):
    """Remake the protein MSM without its dyeless states, sample a burst per entry of
    ``MSM_frames`` and extract -> ``(FEs, d_lifetimes, a_lifetimes, photons, states)``
    (with ``return_trajectories`` also the chains).  Nothing is written."""
    table = event_table(events)
    new_tprobs, new_eqs = remake_prot_MSM_from_lifetimes(
        [np.zeros(k) for k in table.n_events], prot_tcounts, prot_eqs=prot_eqs, device=device)
    out = sample_lifetime_bursts(new_tprobs, new_eqs, table, MSM_frames,
                                 random_state=random_state,
                                 return_trajectories=return_trajectories, device=device,
                                 step_cap=step_cap)
    FEs, d_lifetimes, a_lifetimes = extract_fret_efficiency_lifetimes(out[:3])
    return (FEs, d_lifetimes, a_lifetimes, out[0], out[2]) + tuple(out[3:])


def last_burst_timing():
    """Milliseconds between device events of the last device call of the burst samplers:
    upload, kernels, download (``burst_timing``: summed over a sampler's calls)."""
    ms = np.zeros(3)
    _lib.check(_lib.load().ek_dye_bursts_last_timing(_lib.f64p(ms)))
    return ms


def burst_timing():
    """``last_burst_timing`` summed over the device calls of the last burst sampler"""
    return _burst_ms.copy()
