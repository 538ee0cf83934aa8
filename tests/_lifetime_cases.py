"""The case table of tests/test_gpu_lifetime.py: one entry per public entry point, at
the smallest shape at which the call still takes every allocating branch (a chunk loop
runs twice, every optional output is asked for, sparse and dense forms are both called).
The shapes are those of each module's own smallest GPU test.

A case is either a one-shot function (``fn() -> result``) or a handle (``open() ->
context manager``, ``use(handle) -> result``).  ``bits(result)`` is what two clean calls
must agree on, byte for byte.  Nothing here decides what passes: the assertions are in
test_gpu_lifetime.py.

RAISES lists the device-side raise paths the suite already knows (the call, the
exception it must raise)."""
import contextlib
import functools
import os

import numpy as np
import scipy.sparse

import _numpy_cards as nc
import _numpy_entropy as ne
import _numpy_kmc as nk
import _numpy_mi as nm
import _numpy_pockets as npk
import _numpy_tpt as nt
from enspara_amd import _lib, info_theory, ra, synth, tpt
from enspara_amd.cards.disorder import CardsStates, disorder_interval
from enspara_amd.cluster import kmedoids
from enspara_amd.device import FrameStore
from enspara_amd.exception import DataInvalid, InsufficientResourceError
from enspara_amd.geometry import dyes_from_expt_dist as dyes
from enspara_amd.geometry import libdist, pockets, rotamer, sasa
from enspara_amd.info_theory import JointCounts, entropy
from enspara_amd.msm import bace as B
from enspara_amd.msm import builders
from enspara_amd.msm import synthetic_data as sd
from enspara_amd.msm.transition_matrices import (assigns_to_counts, eigenspectrum,
                                                 eq_probs)
from enspara_amd.tpt.core import _solve

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 0x5EED0123456789AB
R0 = 5.4


def _golden(name):
    return np.load(os.path.join(HERE, "golden", name))


def bits(r):
    """every byte of a result: arrays with dtype and shape, containers in order"""
    if r is None:
        return b"None"
    if isinstance(r, bytes):
        return r
    if scipy.sparse.issparse(r):
        c = scipy.sparse.csr_matrix(r)
        c.sort_indices()
        return b"csr" + bits((np.asarray(c.shape), c.indptr, c.indices, c.data))
    if isinstance(r, ra.RaggedArray):
        return b"ra" + bits([np.asarray(x) for x in r])
    if isinstance(r, np.ndarray):
        if r.dtype == object:
            return bits(list(r))
        return (str(r.dtype) + str(r.shape)).encode() + np.ascontiguousarray(r).tobytes()
    if isinstance(r, dict):
        return b"{" + b"|".join(bits(k) + b":" + bits(r[k]) for k in sorted(r)) + b"}"
    if isinstance(r, (list, tuple)):
        return b"[" + b"|".join(bits(x) for x in r) + b"]"
    if hasattr(r, "cells") and hasattr(r, "pocket_ids"):        # a frame of get_pockets
        return b"pk" + bits((np.asarray(r.shape), r.origin, r.cells, r.pocket_ids))
    if isinstance(r, (bool, int, float, str, np.generic)):
        return repr(r).encode()
    raise TypeError("bits() of %r" % type(r))


class Case:
    def __init__(self, name, fn=None, open=None, use=None, inject=True, recover=0):
        """recover: how many of the call's allocations the library is built to survive
        the failure of (the call returns, with the clean call's bytes); every other
        one must raise"""
        assert (fn is None) != (open is None)
        self.name, self.fn, self.open, self.use = name, fn, open, use
        self.inject, self.recover = inject, recover

    def run(self):
        """the whole lifetime, cleanly"""
        if self.open is None:
            return self.fn()
        with self.open() as h:
            return self.use(h)


CASES = []
RAISES = []


def case(name, **kw):
    def add(f):
        CASES.append(Case(name, fn=f, **kw))
        return f
    return add


def handle(name, open, **kw):
    def add(f):
        CASES.append(Case(name, open=open, use=f, **kw))
        return f
    return add


def raises(name, exc):
    def add(f):
        RAISES.append((name, f, exc))
        return f
    return add


# ---- FrameStore: 300 frames x 5 atoms ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _frames():
    x = synth.synth(300, 5, 8, seed=4)
    x.setflags(write=False)
    return x


def _open_frames():
    return FrameStore.from_array(_frames())


def _run(st, cands):
    st.set_option("candidates", cands)
    st.reset_state()
    idx, cd, fmax = st.kcenters_run(0, 8, 0.0)
    return idx, cd, fmax, st.download_state()


@case("FrameStore create + load + rmsd_to_frame")
def _():
    with FrameStore.from_array(_frames()) as st:
        return st.rmsd_to_frame(3)


@handle("FrameStore.kcenters_run, one candidate", _open_frames)
def _(st):
    return _run(st, 1)


# Two kinds of allocation the run is built to survive the failure of, and returns the
# clean run's bits after: the quad copy of the 16-candidate pass (ek_ensure_qtiles gives
# the upload's staging buffers back and asks again, else runs rounds of 8) and the ten
# buffers of the active view (ek_view_alloc: "the run is what it was without").  With the
# view switched off exactly one allocation may be survived, with it exactly eleven;
# every other one must raise.
def _run16_no_view(st):
    st.set_option("active_view", 0)
    return _run(st, 16)


handle("FrameStore.kcenters_run, 16 candidates, no active view", _open_frames,
       recover=1)(_run16_no_view)


@handle("FrameStore.kcenters_run, 16 candidates", _open_frames, recover=1 + 10)
def _(st):
    return _run(st, 16)


# (ek_last_run_form reads six numbers the run left in the context: no allocation, no
# launch -- rounds of 8 without a view, so that none of the run's own may be survived)
@handle("FrameStore.kcenters_run + last_run_form, 8 candidates, no active view", _open_frames)
def _(st):
    st.set_option("active_view", 0)
    return _run(st, 8), st.last_run_form()


@handle("FrameStore.assign_nearest", _open_frames)
def _(st):
    st.assign_nearest(_frames()[[0, 17, 99, 256, 299]])
    return st.download_state()


@handle("FrameStore PAM sweep", _open_frames)
def _(st):
    med = [0, 17, 99, 256, 299]
    st.assign_nearest(_frames()[med])
    st.set_option("state_exact", 1)
    med = kmedoids._pam_sweep_device(st, med, None, np.random.RandomState(0))
    return med, st.download_state()


@handle("FrameStore.load again + rmsd_to_frame", _open_frames)
def _(st):
    a = st.rmsd_to_frame(299)
    st.load(_frames())
    return a, st.rmsd_to_frame(0)


# (ek_pam_pairs_probe, the test entry of the window's distance kernels: one allocation
# per call, whatever the mode and the form)
def _pairs_inputs():
    from oracle import qcp
    c, G = qcp.center_and_trace(_frames()[:80])
    return (c[:66], G[:66]), (c[66:], G[66:])


@case("ek_pam_pairs_probe: tables, bounds and a list, both forms")
def _():
    import _pam_probe as pp
    (rc, rG), (cc, cG) = _pairs_inputs()
    dprop = np.linspace(0.0, 0.2, len(cc)).astype(np.float32)
    out = []
    for form in (1, 0):
        out += pp.tables(form, rc, rG, cc, cG, 7, 3, 9)
        out += pp.tables(form, rc, rG, cc, cG, 7, 3, len(cc), dprop)
        out.append(pp.listed(form, rc, rG, cc, cG, [65, 3, 40, 4], 70))
    return out


@contextlib.contextmanager
def _open_frame_shard():
    import torch
    ts = torch.cuda.Stream(device=0)
    x = _frames()
    with FrameStore(len(x), x.shape[1], device=0, stream=ts.cuda_stream) as st:
        st.load(x)
        yield st, ts


# (ek_local_candidate and ek_kcenters_step through DeviceShard; with the triangle
# inequality on, label 0 makes the table of accepted centers -- 256 entries --, the
# distance vector and the tile marks of the step)
@handle("FrameStore on a shard: kcenters_step with the triangle inequality",
        _open_frame_shard)
def _(h):
    import torch
    from enspara_amd import sharded
    st, ts = h
    st.reset_state()
    sh = sharded.DeviceShard(st)
    with torch.cuda.stream(ts):
        tri = sharded.kcenters_sharded(sh, 0, 6, 0.0, check_every=2,
                                       use_triangle_inequality=True)
    return tri, st.download_state()


# ---- feature store: 300 x 4 ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _samples():
    X = np.random.RandomState(3).randn(300, 4)
    X.setflags(write=False)
    return X


def _open_samples():
    return libdist.FeatureStore.from_array(_samples(), 0)


@case("FeatureStore create + load + distance")
def _():
    with _open_samples() as fs:
        out = np.zeros(300)
        fs.distance(0, _samples()[5], out)
        return out


@handle("feature k-centers", _open_samples)
def _(fs):
    d, a = np.full(300, np.inf), np.full(300, -1, dtype=np.int32)
    centers, fmax = fs.kcenters(0, 0, 8, 0.0, d, a)
    return centers, fmax, d, a


@handle("feature assign_nearest", _open_samples)
def _(fs):
    return fs.assign_nearest(1, _samples()[[0, 17, 99, 256, 299]])


@handle("feature PAM sweep", _open_samples)
def _(fs):
    med = np.array([0, 17, 99, 256, 299], dtype=np.int64)
    d, a = fs.assign_nearest(0, _samples()[med])
    accept = np.zeros(len(med), dtype=np.int32)
    raw = np.random.RandomState(0).randint(0, 2 ** 32, size=4096, dtype=np.uint32)
    out = fs.pam_sweep(0, med, None, raw, 0, d, a, accept, 0)
    return out, med, d, a, accept


@contextlib.contextmanager
def _open_shard():
    import torch
    ts = torch.cuda.Stream(device=0)
    with libdist.FeatureStore.from_array(_samples().astype(np.float32), 0, device=0,
                                         stream=ts.cuda_stream) as st:
        yield st, ts


# (the first step of a sharded run makes the shard's history: feat_shard_alloc)
@handle("feature k-centers on a shard (history growth)", _open_shard)
def _(h):
    import torch
    from enspara_amd import sharded
    st, ts = h
    sh = sharded.FeatureShard(st, 0)
    with torch.cuda.stream(ts):
        sh.reset_state()
        idx, cd = sharded.kcenters_sharded(sh, 0, 5, 0.0, check_every=4)
    return idx, cd, sh.state()


@case("libdist.euclidean / kcenters_resident / assign_nearest_resident")
def _():
    X = _samples()
    d0, a0 = np.full(300, np.inf), np.full(300, -1, dtype=np.int64)
    return (libdist.euclidean(X, X[7]),
            libdist.kcenters_resident(X, 1, 0, 4, 0.0, d0, a0),
            libdist.assign_nearest_resident(X, 0, X[[3, 200]]))


# ---- mutual information: (Fx, n_x, Fy, n_y) = (5, 3, 4, 4), 65 frames ------------------------
@functools.lru_cache(maxsize=None)
def _xy():
    rng = np.random.RandomState(16)
    X = nm.biased_codes(rng, 130, 5, 3)
    Y = nm.noisy_copy(rng, nm.biased_codes(rng, 130, 4, 4), X, 3, 2, 4)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@case("joint_counts + mutual_information + mi_matrix")
def _():
    X, Y = _xy()
    jc = info_theory.joint_counts(X[:65], Y[:65], 3, 4)
    return (jc, info_theory.joint_counts(X[:65], n_x=3), info_theory.mutual_information(jc),
            info_theory.mi_matrix([X[:65], X[65:]], [Y[:65], Y[65:]], 3, 4))


@handle("JointCounts.add + counts + mutual_information", lambda: JointCounts(5, 4, 3, 4))
def _(jc):
    X, Y = _xy()
    jc.add(X[:65], Y[:65])
    return jc.counts(), jc.mutual_information()


@case("JointCounts open")
def _():
    with JointCounts(5, 4, 3, 4) as jc:
        return jc.counts()


@case("weighted_mi + weighted_joint_probabilities")
def _():
    rng = np.random.RandomState(17)
    X = nm.biased_codes(rng, 65, 5, 3)
    w = rng.dirichlet(np.ones(65))
    return (info_theory.weighted_joint_probabilities(X, w, 3),
            info_theory.weighted_mi(X, w, n_feature_states=np.full(5, 3), normalize=False))


# ---- CARDS: 3 features, 65 frames, two trajectories ------------------------------------------
@functools.lru_cache(maxsize=None)
def _codes():
    rng = np.random.RandomState(18)
    return [nm.biased_codes(rng, 65, 3, 3, np.uint8) for _ in range(2)]


@handle("CardsStates.add + stats + disorder + matrices + counts", lambda: CardsStates(3, 3))
def _(d):
    for t in _codes():
        d.add(t)
    stats = d.stats()
    d.disorder(*disorder_interval(*d.mean_times()))
    codes = [d.disorder_codes(i) for i in range(2)]
    return stats, codes, d.matrices(), [d.counts(w) for w in range(4)]


@case("CardsStates open")
def _():
    with CardsStates(3, 3) as d:
        return d.stats()


# ---- rotamers: 3 dihedrals, 257 frames --------------------------------------------------------
BOUNDS = [nc.PHI, nc.PSI, nc.CHI]
SHIFTS = [0, 100, 0]


@functools.lru_cache(maxsize=None)
def _dihedrals():
    kind = np.arange(3) % 3
    xyz, quads, deg = nc.safe_trajectory(np.random.RandomState(57), 257, kind, BOUNDS, SHIFTS,
                                         15)
    return xyz, quads, kind


@case("dihedral_angles + rotamer_states + dihedral_rotamers")
def _():
    xyz, quads, kind = _dihedrals()
    ang = rotamer.dihedral_angles(xyz, quads)
    return (ang, rotamer.rotamer_states(ang, kind, BOUNDS, SHIFTS, 15),
            rotamer.dihedral_rotamers(xyz, quads, kind, BOUNDS, SHIFTS, 15,
                                      return_angles=True))


# ---- SASA: 65 atoms, 2 frames, 24 points ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _atoms():
    rng = np.random.RandomState(19)
    xyz = rng.uniform(0, 1.2, size=(2, 65, 3)).astype(np.float32)
    return xyz, rng.uniform(0.12, 0.2, size=65)


@case("shrake_rupley: groups, counts, chunk_frames=1")
def _():
    xyz, radii = _atoms()
    groups = [np.arange(0, 30), np.arange(30, 65)]
    return (sasa.shrake_rupley(xyz, radii, n_sphere_points=24, atom_groups=groups,
                               return_counts=True, chunk_frames=1),
            sasa.shrake_rupley(xyz, radii, n_sphere_points=24, chunk_frames=1))


# ---- pockets ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _peptide():
    E = _golden("exposons_golden.npz")
    return np.ascontiguousarray(E["bp_xyz"][:2]), npk.radii_of(E["bp_elements"])


@case("get_pockets: two frames, chunk_frames=1")
def _():
    xyz, radii = _peptide()
    return list(pockets.get_pockets(xyz, radii, 0.1, 0.07, 3, chunk_frames=1))


@case("determine_touches_protein + rank_cells + label_cells")
def _():
    xyz, radii = _peptide()
    rng = np.random.RandomState(20)
    T = rng.rand(6, 6, 6) < 0.5
    return (pockets.determine_touches_protein(xyz[0], radii, 0.1, 0.07),
            pockets.rank_cells(T), pockets.label_cells(rng.rand(6, 6, 6) < 0.5))


# ---- entropy: 3 x 9 ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows():
    rng = np.random.RandomState(21)
    return ne.random_rows(rng, 3, 9), ne.random_rows(rng, 3, 9)


@case("kl_divergence + js_divergence + shannon_entropy_rows")
def _():
    P, Q = _rows()
    return (entropy.kl_divergence(P, Q), entropy.js_divergence(P, Q),
            entropy.shannon_entropy_rows(P))


@case("relative_entropy_per_state(assignments=)")
def _():
    rng = np.random.RandomState(22)
    P = ne.random_rows(rng, 9, 9)
    A = rng.randint(0, 9, size=(2, 65))
    return entropy.relative_entropy_per_state(P, assignments=A)


@case("state_counts")
def _():
    return entropy.state_counts(_codes(), 3)


# ---- kinetic Monte Carlo ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chain_T():
    T = nk.random_T(np.random.RandomState(23), 70, 9)
    T.setflags(write=False)
    return T


@handle("Sampler.trajectories (both forms, step_cap=7) + next", lambda: sd.Sampler(_chain_T()))
def _(s):
    start = np.arange(65) % 70
    u = np.random.RandomState(24).rand(65)
    return ([s.trajectories(start, 17, random_state=SEED, form=f, step_cap=7)
             for f in ("lane", "wave")], s.next(start, u))


@case("Sampler open, dense and sparse")
def _():
    out = []
    for M in (_chain_T(), scipy.sparse.csr_matrix(_chain_T())):
        with sd.Sampler(M) as s:
            out.append(s.next([0, 1], [0.25, 0.75]))
    return out


@case("synthetic_ensemble: dense, sparse, observable")
def _():
    rng = np.random.RandomState(25)
    T = nk.random_T(rng, 65, 9)
    p0, obs = rng.dirichlet(np.ones(65)), rng.randn(65)
    return [sd.synthetic_ensemble(M, p0, 5, observable_per_state=o)
            for M in (T, scipy.sparse.csr_matrix(T)) for o in (None, obs)]


@functools.lru_cache(maxsize=None)
def _bursts():
    rng = np.random.RandomState(26)
    T = nk.random_T(rng, 6, 4)
    pops = rng.dirichlet(np.ones(6))
    dd = []
    for s, n_bins in enumerate([2, 1, 64, 65, 3, 2]):
        dd.append(np.stack([2.0 + 0.25 * np.arange(n_bins) + 0.1 * s,
                            rng.dirichlet(np.ones(n_bins))], axis=1))
    frames = [np.sort(rng.randint(0, [1, 17, 300][b % 3] + 1, size=[1, 2, 64, 65][b % 4]))
              for b in range(65)]
    return T, pops, ra.RaggedArray(dd), frames


@case("sample_FRET_histograms with and without trajectories + sample_FE_probs")
def _():
    T, pops, dd, frames = _bursts()
    out = [dyes.sample_FRET_histograms(T, pops, dd, frames, R0, n_photon_std=4,
                                       random_state=SEED, return_trajectories=keep)
           for keep in (True, False)]
    states = np.random.RandomState(27).randint(0, 6, size=65)
    return out, dyes.sample_FE_probs(dd, states, R0, random_state=SEED, chain=3)


# ---- transition path theory: the n17 golden chain ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _n17():
    G = _golden("tpt_golden.npz")
    C = G["C_n17"]
    return (nt.tprob_from_counts(C), nt.pops_from_counts(C), G["src_n17_qA"], G["snk_n17_qA"],
            G["snk_n17_t3"])


@case("committors")
def _():
    T, pops, src, snk, snk3 = _n17()
    return tpt.committors(T, src, snk)


@case("mfpts to sinks and all-to-all")
def _():
    T, pops, src, snk, snk3 = _n17()
    return tpt.mfpts(T, sinks=snk3), tpt.mfpts(T, populations=pops)


@case("reactive_fluxes + net_fluxes, dense and sparse")
def _():
    T, pops, src, snk, snk3 = _n17()
    return [f(M, src, snk, populations=pops) for f in (tpt.reactive_fluxes, tpt.net_fluxes)
            for M in (T, scipy.sparse.csr_matrix(T))]


@functools.lru_cache(maxsize=None)
def _system65():
    rng = np.random.RandomState(28)
    return rng.randn(65, 65) + 65 * np.eye(65), rng.randn(65, 3)


@case("_solve n = 65, nrhs = 3")
def _():
    return _solve(*_system65(), return_pivots=True)


# ---- MSM -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _assigns():
    A = np.random.RandomState(29).randint(0, 9, size=(3, 65))
    return A, assigns_to_counts(A, lag_time=1, max_n_states=9)


@case("assigns_to_counts: sliding window and not")
def _():
    A, _ = _assigns()
    return (assigns_to_counts(A, lag_time=1, max_n_states=9),
            assigns_to_counts(A, lag_time=2, sliding_window=False))


@case("builders.normalize, sparse and dense")
def _():
    C = _assigns()[1]
    return [builders.normalize(M, calculate_eq_probs=True) for M in (C, C.toarray())]


@case("builders.transpose, sparse and dense")
def _():
    C = _assigns()[1]
    return [builders.transpose(M, calculate_eq_probs=True) for M in (C, C.toarray())]


@case("builders.mle")
def _():
    return builders.mle(_assigns()[1].toarray() + 1.0)


@case("eq_probs + eigenspectrum, dense")
def _():
    T = _chain_T()
    return eq_probs(T), eigenspectrum(T, n_eigs=5)


@case("eigenspectrum, sparse")
def _():
    return eigenspectrum(scipy.sparse.csr_matrix(_chain_T()), n_eigs=3)


# ---- BACE -------------------------------------------------------------------------------------------
@case("bace on n24_p2")
def _():
    return B.bace(_golden("bace_golden.npz")["C_n24_p2"], 2, chunk_size=7)


@case("baysean_prune on n24_p2, dense and sparse")
def _():
    C = _golden("bace_golden.npz")["C_n24_p2"]
    return B.baysean_prune(C), B.baysean_prune(scipy.sparse.csr_matrix(C))


# ---- the raise paths the suite already knows -------------------------------------------------------
EMPTY_ROW = np.array([[0.5, 0.5, 0.0, 0.0], [0.0, 0.5, 0.5, 0.0], [0.0, 0.0, 0.0, 0.0],
                      [0.0, 0.0, 0.0, 1.0]])


@raises("k-MC empty row, lane form", DataInvalid)
def _():
    sd.synthetic_trajectories(EMPTY_ROW, [0, 0, 3], 200, random_state=SEED, form="lane")


@raises("k-MC empty row, wave form", DataInvalid)
def _():
    sd.synthetic_trajectories(EMPTY_ROW, [0, 0, 3], 200, random_state=SEED, form="wave")


@raises("k-MC empty row, sample_next", DataInvalid)
def _():
    sd.sample_next(EMPTY_ROW, [0, 2], [0.1, 0.1])


@raises("k-MC empty row, bursts", DataInvalid)
def _():
    T = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    dd = [np.array([[1.0, 0.5], [2.0, 0.5]])] * 3
    dyes.sample_FRET_histograms(T, [1.0, 0, 0], dd, [[0, 5]], R0, random_state=SEED)


@functools.lru_cache(maxsize=None)
def _closed_class():
    T = _n17()[0].copy()
    closed = [3, 4, 5]
    T[closed] = 0.0
    T[np.ix_(closed, closed)] = [[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]]
    return T


@raises("singular committor system", DataInvalid)
def _():
    tpt.committors(_closed_class(), 0, 16)


@raises("singular MFPT system", DataInvalid)
def _():
    tpt.mfpts(_closed_class(), sinks=[16])


@raises("singular system under net_fluxes", DataInvalid)
def _():
    tpt.net_fluxes(_closed_class(), 0, 16, populations=_n17()[1])


@raises("zero pivot in _solve", DataInvalid)
def _():
    n, k = 17, 9
    rng = np.random.RandomState(k)
    L = np.tril(rng.randint(-1, 2, size=(n, n)).astype(np.float64), -1) + np.eye(n)
    U = np.triu(rng.randint(-3, 4, size=(n, n)).astype(np.float64), 1)
    U += np.diag(4.0 * rng.choice([-1, 1], size=n))
    U[k, k] = 0.0
    _solve(L @ U, np.ones(n))


@raises("BACE on disconnected counts", DataInvalid)
def _():
    C = np.zeros((5, 5))
    C[:4, :4] = [[300, 40, 25, 12], [38, 280, 30, 9], [22, 35, 310, 14], [10, 8, 15, 90]]
    C[4, 4] = 500
    B.bace(C, 1)


@raises("negative entry under kl_divergence", DataInvalid)
def _():
    P, Q = _rows()
    P = P.copy()
    P[2, 8] = -0.25
    entropy.kl_divergence(P, Q)


@raises("negative entry under js_divergence", DataInvalid)
def _():
    P, Q = _rows()
    Q = Q.copy()
    Q[2, 8] = -0.25
    entropy.js_divergence(P, Q)


@raises("JointCounts.add with a wrong shape, handle open", DataInvalid)
def _():
    X, Y = _xy()
    with JointCounts(5, 4, 3, 4) as jc:
        jc.add(X[:65], Y[:65])
        jc.add(X[:65, :4], Y[:65])


@raises("joint_counts with a state out of range", DataInvalid)
def _():
    X, Y = _xy()
    info_theory.joint_counts(np.where(X == 2, 3, X), Y, 3, 4)


@raises("mi_matrix with trajectories of different widths", DataInvalid)
def _():
    X, Y = _xy()
    info_theory.mi_matrix([X[:65], X[65:, :4]], [Y[:65], Y[65:]], 3, 4)


@raises("CardsStates.add with a wrong shape, handle open", DataInvalid)
def _():
    with CardsStates(3, 3) as d:
        d.add(_codes()[0])
        d.add(_codes()[1][:, :2])


@raises("state_counts with a code that is no state", DataInvalid)
def _():
    entropy.state_counts(_codes(), 2)


@raises("ek_sasa_run with a null argument, handle open", _lib.HipError)
def _():
    import ctypes as C
    L = _lib.load()
    R = np.full(65, 0.3, dtype=np.float32)
    pts = np.ascontiguousarray(sasa.sphere_points(24), dtype=np.float32)
    h = C.c_void_p()
    _lib.check(L.ek_sasa_open(0, 65, _lib.f32p(R), len(pts), _lib.f32p(pts), 0, None, None,
                              C.byref(h)))
    try:
        _lib.check(L.ek_sasa_run(h, None, 2, 1, None, None, None))
    finally:
        L.ek_sasa_close(h)


@raises("ek_pam_pairs_probe with a list entry past the rows", _lib.HipError)
def _():
    import _pam_probe as pp
    (rc, rG), (cc, cG) = _pairs_inputs()
    pp.listed(1, rc, rG, cc, cG, [65, 66], 70)


@raises("ek_pam_pairs_probe with old columns past the table", _lib.HipError)
def _():
    import _pam_probe as pp
    (rc, rG), (cc, cG) = _pairs_inputs()
    pp.tables(0, rc, rG, cc, cG, 7, 60, 9)


@raises("JointCounts too large for the device", InsufficientResourceError)
def _():
    JointCounts(30000, 30000, 255, 255)


@raises("CardsStates too large for the device", InsufficientResourceError)
def _():
    CardsStates(30000, 255)
