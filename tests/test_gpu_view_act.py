"""The rounds under an active view read frame-major rows through the selection
(csrc/ek_common.h ``ek_round_row``): a view keeps no frame-major copy of its own, a
position of the view names a row of the shard's through ``v_act``.  A position that is
mapped twice, not at all, or taken for a shard row gives another frame's coordinates
to the pair distances, the candidate tile or a record -- and with them other centers.
Every fit here runs with the view's buffers filled with 0xFF bytes before every
rebuild (option value 3) and is compared with the CPU oracle bit for bit: centers,
labels, float32 distances.

Shapes: 700 and 1100 frames (three and five tiles of 256, the last one partial), 3, 5
and 8 atoms (rows of 16 and of 4 bytes, A % 4 != 0), clouds of 25 frames in random
frame order, so that frames that have settled lie before the far ones and the far
ones' positions in a view differ from their rows in the shard -- checked on the CPU,
with the oracle alone, before anything runs on the device."""
import numpy as np
import pytest

from enspara_amd import synth

pytestmark = pytest.mark.gpu

PER = 25                            # frames per cloud
SIGMA = 0.01                        # their noise per coordinate
SHAPES = [(700, 3), (700, 5), (700, 8), (1100, 3), (1100, 5), (1100, 8)]
FORMS = (16, 8, -1)                 # candidates pinned to 16, to 8, the ladder
RHO, REL, ABS = 0.75, 1e-3, 1e-3    # the view's margin (csrc/ek_run_policy.h)


@pytest.fixture(scope="module")
def ocl():
    from oracle import cluster
    return cluster


def _clouds(n, A, seed, twice=False):
    """n frames: clouds of PER noisy copies of a chain each, in random order; twice:
    every frame present two times"""
    rng = np.random.RandomState(seed)
    n_own = n // 2 if twice else n
    assert n_own % PER == 0
    tmpl = synth.templates(n_own // PER, A, seed + 100)
    x = np.concatenate([tmpl[t] + rng.normal(scale=SIGMA, size=(PER, A, 3))
                        for t in range(len(tmpl))]).astype(np.float32)
    if twice:
        x = np.concatenate([x, x])
    return np.ascontiguousarray(x[rng.permutation(len(x))])


def _replay(x, centers):
    """the maximum after every center, and whether -- before the last center -- a frame
    that has settled (distance <= theta of a view built then) lies before the next
    center: that center's position in the view is then not its row in the shard"""
    from oracle import qcp
    P = qcp.Prepared(x)
    dist = np.full(P.n, np.inf)
    maxima, shifted = [], False
    for k, c in enumerate(centers):
        cc, Gc = qcp.center_and_trace(P.xyz[int(c)])
        d = qcp.rmsd_centered(P.c, P.G, cc[0], Gc[0])
        dist = np.minimum(dist, d)
        m = float(dist.max())
        maxima.append(m)
        if k + 1 < len(centers):
            theta = (RHO * m - ABS) / (2.0 * (1.0 + REL))
            shifted = shifted or bool((dist[:int(np.argmax(dist))] <= theta).any())
    return maxima, shifted


_CASES = {}


def _case(ocl, n, A, k, twice=False):
    """data, the oracle's fit and its replay, computed once"""
    key = (n, A, k, twice)
    if key not in _CASES:
        x = _clouds(n, A, seed=7 * n + A, twice=twice)
        want = ocl.kcenters(x, n_clusters=k)
        _CASES[key] = (x, want, _replay(x, want[0]))
    return _CASES[key]


def _store(x):
    from enspara_amd.device import FrameStore
    return FrameStore.from_array(x)


def _fit(x, n_clusters, cutoff, cands, view):
    from enspara_amd.cluster import kcenters as kc
    with _store(x) as st:
        st.set_option("candidates", cands)
        st.set_option("active_view", view)
        r = kc._kcenters_device(x, n_clusters, cutoff, None, 0, store=st)
        return r, st.view_stats()


def _same(r, want):
    assert [int(i) for i in r.center_indices] == [int(i) for i in want[0]]
    np.testing.assert_array_equal(r.assignments, want[1])
    np.testing.assert_array_equal(r.distances, want[2].astype(np.float32))


@pytest.mark.parametrize("n,A", SHAPES)
def test_rows_through_the_selection(ocl, n, A):
    """fewer centers than clouds (24 of 28, 32 of 44): no maximum collapses, no guard
    ends a view, and the run ends under one"""
    k = 24 if n == 700 else 32
    x, want, (maxima, shifted) = _case(ocl, n, A, k)
    assert shifted, "no settled frame before a far one: the data tests nothing"
    for cands in FORMS:
        r, vs = _fit(x, k, 0.0, cands, 3)
        print(n, A, cands, vs)
        _same(r, want)
        assert vs["views"] >= 2 and vs["left_out"] > 0, (cands, vs)
    # option 24 = 0: the same arrays
    r, vs = _fit(x, k, 0.0, 16, 0)
    _same(r, want)
    assert vs["views"] == 0 and vs["left_out"] == 0, vs


@pytest.mark.parametrize("n,A", SHAPES)
def test_every_frame_twice(ocl, n, A):
    """equal maxima all along: the first of them by position is the center, and its twin
    -- another position, another row, the same coordinates -- must end at distance 0"""
    k = 24 if n == 700 else 32
    x, want, (maxima, shifted) = _case(ocl, n, A, k, twice=True)
    assert shifted
    for cands in FORMS:
        r, vs = _fit(x, k, 0.0, cands, 3)
        print(n, A, cands, vs)
        _same(r, want)
        assert vs["views"] >= 2 and vs["left_out"] > 0, (cands, vs)


@pytest.mark.parametrize("A", [3, 5, 8])
def test_cutoff_met_under_a_view(ocl, A):
    """a cut-off halfway down the largest relative drop of the maximum between the 12th
    center and two past the last cloud's: with 8 atoms that is where every cloud has
    its center and the maximum collapses (the view's guard ends it), with 3 -- chains of
    three atoms differ little -- an ordinary step; either way the forced view is on
    when the maximum meets the cut-off"""
    n, T = 700, 700 // PER
    x, _, (maxima, shifted) = _case(ocl, n, A, T + 2)
    assert shifted
    j = max(range(12, T + 2), key=lambda i: maxima[i - 1] / maxima[i])
    assert maxima[j - 1] > maxima[j]
    cutoff = 0.5 * (maxima[j - 1] + maxima[j])
    want = ocl.kcenters(x, dist_cutoff=cutoff)
    assert len(want[0]) == j + 1
    for cands in FORMS:
        r, vs = _fit(x, np.inf, cutoff, cands, 3)
        print(A, cands, j, vs)
        _same(r, want)
        assert vs["views"] >= 2 and vs["left_out"] > 0, (cands, vs)


@pytest.mark.parametrize("n,A", [(700, 5), (1100, 8)])
def test_pam_sweep_after_a_view(ocl, monkeypatch, n, A):
    """a run that ends under a view leaves the records for the next entry point: one PAM
    sweep on the same store must find shard rows in them"""
    from enspara_amd.cluster import hybrid as hy
    from enspara_amd.device import FrameStore
    k = 24 if n == 700 else 32
    x, _, (maxima, shifted) = _case(ocl, n, A, k)
    assert shifted
    wi, wa, wd = ocl.hybrid(x, n_clusters=k, n_iters=1,
                            random_state=np.random.RandomState(3))
    make = FrameStore.from_array.__func__
    stats = []

    def from_array(cls, X, *a, **kw):
        st = make(cls, X, *a, **kw)
        st.set_option("candidates", 16)
        st.set_option("active_view", 3)
        run = st.kcenters_run

        def kcenters_run(*ra, **rkw):
            out = run(*ra, **rkw)
            stats.append(st.view_stats())
            return out
        st.kcenters_run = kcenters_run
        return st
    monkeypatch.setattr(FrameStore, "from_array", classmethod(from_array))
    r = hy.hybrid(x, "rmsd", n_iters=1, n_clusters=k,
                  random_state=np.random.RandomState(3))
    monkeypatch.undo()
    print(n, A, stats)
    assert stats and stats[-1]["views"] >= 2 and stats[-1]["guard_exits"] == 0, stats
    assert [int(i) for i in r.center_indices] == [int(i) for i in wi]
    np.testing.assert_array_equal(r.assignments, wa)
    np.testing.assert_array_equal(r.distances, wd.astype(np.float32))
