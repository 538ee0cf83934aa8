"""The shipped RMSD kernels on the structure families of tests/_structure_cases.py:
collinear (exactly and nearly), planar, mirrored, noise-free copies, identical
frames, a cube, two atoms on a coarse grid, and scales on both sides of the
float32 certificate's range of q.  Every other GPU test draws from
enspara_amd.synth (generic chains at nanometre scale); the degenerate spectra of
tests/_qcp_cases.py reach ek_qcp_probe_kernel alone.  Here the frames go through
ek_step_kernel<FPL, .>, ek_pass2_kernel, ek_pass16_kernel (certificate, queue,
dense fallback), the three nearest-center kernels and the streaming form of a PAM
sweep.  (The ek_pam_pairs* kernels and the windows in one workgroup need 16384
frames and K well above 128: the families go through them in
tests/test_gpu_pam_pairs.py.)

Bars as everywhere: center indices and labels equal, distances equal as float32
bits to oracle.qcp / oracle.cluster.  No case is skipped: where the oracle raises
(a PAM draw from an empty cluster), the device path must raise too.

Shapes are the smallest that still reach each path: 1000 frames (four tiles of
256, the last one partly empty) for one-vs-all and the fits, 300 for assignment;
A in {2, 3, 4, 7, 33}: every remainder mod 4 (zero padding of the quad copy), 33
more than two groups of 16 atoms.
"""
import functools

import numpy as np
import pytest

from _structure_cases import FAMILIES, FIXED_ATOMS, family_cases, structure_family

pytestmark = pytest.mark.gpu

CASES = family_cases()
N_FIT, N_ASSIGN = 1000, 300
K_CENTERS, K_PAM = 40, 20
# one cut-off run per family
CUTOFF_CASES = [(f, FIXED_ATOMS.get(f, 7)) for f in FAMILIES]


def _store(x):
    from enspara_amd.device import FrameStore
    return FrameStore.from_array(x)


@functools.lru_cache(maxsize=None)
def _frames(family, A, n):
    """frames and their Prepared (shared, never written to)"""
    from oracle import qcp
    x = structure_family(family, n, A)
    return x, qcp.Prepared(x)


@functools.lru_cache(maxsize=None)
def _oracle_kcenters(family, A):
    from oracle import cluster as oc
    x, P = _frames(family, A, N_FIT)
    return oc.kcenters(P, n_clusters=K_CENTERS)


def _assert_fit(r, want):
    inds, a, d = want
    assert list(r.center_indices) == [int(i) for i in inds]
    np.testing.assert_array_equal(r.assignments, a)
    assert r.distances.dtype == np.float64
    np.testing.assert_array_equal(r.distances.astype(np.float32).view(np.uint32),
                                  d.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("family,A", CASES)
def test_one_vs_all(family, A):
    """ek_step_kernel at 1, 2 and 4 frames per lane, a frame of the store and
    foreign coordinates as the center"""
    from oracle import qcp
    x, P = _frames(family, A, N_FIT)
    other = structure_family(family, 1, A, seed=1)[0]
    want_other = qcp.rmsd(x, other)
    with _store(x) as st:
        for fpl in (1, 2, 4):
            st.set_frames_per_lane(fpl)
            for c in (0, N_FIT // 2, N_FIT - 1):
                got = st.rmsd_to_frame(c)
                want = P.rmsd_to_frame(c)
                assert got.dtype == np.float32
                np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
                assert got[c] <= 1e-3 * np.sqrt(2.0 * P.G[c] / A), (c, got[c])
            got = st.rmsd_to_xyz(other)
            np.testing.assert_array_equal(got.view(np.uint32),
                                          want_other.view(np.uint32))


@pytest.mark.parametrize("family,A", CASES)
def test_kcenters(family, A):
    """40 centers in rounds of 1, 8, 16 and 32 candidates, the cheap steps of a
    round of 16 chained and one by one (identical, rotated_copies: the oracle
    runs out of distinct frames and goes on with repeats)"""
    from enspara_amd.cluster import kcenters as kc
    x, P = _frames(family, A, N_FIT)
    want = _oracle_kcenters(family, A)
    with _store(x) as st:
        for cands, chained in ((1, 1), (8, 1), (16, 1), (32, 1), (16, 0)):
            st.set_option("candidates", cands)
            st.set_option("chained", chained)
            r = kc._kcenters_device(x, K_CENTERS, 0, None, 0, store=st)
            _assert_fit(r, want)


@pytest.mark.parametrize("family,A", CUTOFF_CASES)
def test_kcenters_cutoff(family, A):
    """the cut-off stop rule at the median of the distances 40 centers leave (at
    most one center per frame: a residual self-distance above the cut-off would
    otherwise never let the oracle stop)"""
    from enspara_amd.cluster import kcenters as kc
    from oracle import cluster as oc
    x, P = _frames(family, A, N_FIT)
    cut = float(np.median(_oracle_kcenters(family, A)[2]))
    want = oc.kcenters(P, n_clusters=N_FIT, dist_cutoff=cut)
    with _store(x) as st:
        r = kc._kcenters_device(x, N_FIT, cut, None, 0, store=st)
    _assert_fit(r, want)


@pytest.mark.parametrize("family,A", CASES)
def test_assign_nearest(family, A):
    """vector FMA, MFMA 32x32x2, MFMA 16x16x4 and the automatic choice against 8,
    24, 64 and 70 centers (both sides of the two dispatch boundaries), half of
    them frames of the store, half from the same family under another seed; with
    duplicated centers the lowest index wins"""
    from oracle import qcp
    x, P = _frames(family, A, N_ASSIGN)
    rng = np.random.RandomState(5)
    pool = np.concatenate([x[rng.randint(0, N_ASSIGN, size=35)],
                           structure_family(family, 35, A, seed=1)])
    pool = np.ascontiguousarray(pool[rng.permutation(len(pool))])
    with _store(x) as st:
        for K in (8, 24, 64, 70):
            ctrs = pool[:K]
            cc, Gc = qcp.center_and_trace(ctrs)
            wa, wd = qcp.assign_nearest(P.c, P.G, cc, Gc)
            for variant in (1, 2, 3, 0):
                st.set_option("assign_kernel", variant)
                st.assign_nearest(ctrs)
                d, a = st.download_state()
                np.testing.assert_array_equal(a, wa)
                np.testing.assert_array_equal(d.view(np.uint32), wd.view(np.uint32))
        dup = np.ascontiguousarray(np.concatenate([pool[:3], pool[:3], pool[3:24]]))
        cc, Gc = qcp.center_and_trace(dup)
        wa, wd = qcp.assign_nearest(P.c, P.G, cc, Gc)
        assert not np.isin(wa, [3, 4, 5]).any()
        for variant in (1, 2, 3):
            st.set_option("assign_kernel", variant)
            st.assign_nearest(dup)
            d, a = st.download_state()
            np.testing.assert_array_equal(a, wa)
            np.testing.assert_array_equal(d.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("family,A", CASES)
def test_one_pam_sweep(family, A):
    """hybrid(..., n_iters=1) at K = 20 -- its two steps on one store.  1000 frames
    reach the STREAMING form of the sweep only (a pass over all frames per group of
    proposals, three launches per proposal): ek_pam_prefetch_vectors takes the
    window's form -- ek_pam_pairs_kernel / ek_pam_pairs16_kernel, ek_pam_active_kernel,
    the window in one workgroup -- from 16384 frames on, so the two options set
    below (pam_pairs_mfma is process-wide: always said, and left at its default)
    select nothing here and the four runs are the same run.  The families go
    through those kernels in tests/test_gpu_pam_pairs.py::test_structure_families."""
    from enspara_amd.cluster import kcenters as kc
    from enspara_amd.cluster import kmedoids as km
    from oracle import cluster as oc
    x, P = _frames(family, A, N_FIT)
    inds, a, d = oc.kcenters(P, n_clusters=K_PAM)
    try:
        want = oc.pam_update(P, list(inds), a, d,
                             random_state=np.random.RandomState(3))
        want = (want[0], want[2], want[1])
    except ValueError:              # a draw from an empty cluster
        want = None

    def sweep(st):
        r = kc._kcenters_device(x, K_PAM, 0, None, 0, store=st)
        assert list(r.center_indices) == [int(i) for i in inds]
        return km._kmedoids_iterations_device(x, st, 1, r.center_indices, None,
                                              np.random.RandomState(3))

    with _store(x) as st:
        try:
            for mfma, one_wg in ((1, 1), (1, 0), (0, 1), (0, 0)):
                st.set_option("pam_pairs_mfma", mfma)
                st.set_option("pam_one_workgroup", one_wg)
                if want is None:
                    with pytest.raises(ValueError):
                        sweep(st)
                else:
                    _assert_fit(sweep(st), want)
        finally:
            st.set_option("pam_pairs_mfma", 1)
