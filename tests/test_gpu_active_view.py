"""The active view of k-centers rounds (option "active_view", csrc/ek_view.hip):
between two batches of rounds the frames no coming center can change are left
out of the store the rounds stream.  It is exact, so every run here is compared
with the CPU oracle bit for bit -- centers, labels, float32 distances -- with the
option off (0), by the policy (1) and forced (2: rebuilt every other round)."""
import numpy as np
import pytest

from enspara_amd import synth

pytestmark = pytest.mark.gpu

FORMS = (16, 8, 1, -1)      # option key 4: pinned rounds of 16 / 8, one center, adaptive


@pytest.fixture(scope="module")
def ocl():
    from oracle import cluster
    return cluster


def _store(x):
    from enspara_amd.device import FrameStore
    return FrameStore.from_array(x)


def _clouds(n_templates, per, A, seed, shuffle=True, sigma=0.05):
    """`per` noisy copies of each of `n_templates` chains, in random order"""
    rng = np.random.RandomState(seed)
    tmpl = synth.templates(n_templates, A, seed + 100)
    x = np.concatenate([tmpl[t] + rng.normal(scale=sigma, size=(per, A, 3))
                        for t in range(n_templates)]).astype(np.float32)
    if shuffle:
        x = x[rng.permutation(len(x))]
    return np.ascontiguousarray(x)


def _fit(x, n_clusters, cutoff, cands, view, tri=False):
    from enspara_amd.cluster import kcenters as kc
    with _store(x) as st:
        st.set_option("candidates", cands)
        st.set_option("active_view", view)
        assert st.get_option("active_view") == view
        r = kc._kcenters_device(x, n_clusters, cutoff, None, 0, store=st,
                                use_triangle_inequality=tri)
        return r, st.view_stats()


def _same(r, want):
    assert list(r.center_indices) == [int(i) for i in want[0]]
    np.testing.assert_array_equal(r.assignments, want[1])
    np.testing.assert_array_equal(r.distances, want[2])


@pytest.mark.parametrize("A", [20, 21, 22, 23])
def test_templates_shuffled(ocl, A):
    """40 clouds of 61 frames (2440: no multiple of 64 or 256), 60 centers: the
    maximum collapses once every cloud has a center -- inside a view, whose guard
    ends it -- and the run goes on at small distances.  And a cut-off that stops
    the run inside a view."""
    x = _clouds(40, 61, A, seed=A)
    for n_clusters, cutoff in ((60, 0.0), (np.inf, 0.17)):
        want = ocl.kcenters(x, n_clusters=None if np.isinf(n_clusters) else n_clusters,
                            dist_cutoff=cutoff or None)
        for cands in FORMS:
            for view in (0, 1, 2):
                r, vs = _fit(x, n_clusters, cutoff, cands, view)
                _same(r, want)
                if view == 0:
                    assert vs["views"] == 0 and vs["left_out"] == 0, vs
                if view == 2 and cands == 1:
                    # (key 4 pinned to 1 runs no rounds: the plain one-center loop,
                    # which has no view -- the one-center steps of the adaptive run
                    # are the ones that see one)
                    assert vs["views"] == 0, vs
                elif view == 2:
                    assert vs["views"] > 0 and vs["left_out"] > 0, (cands, vs)
                    # (a pinned round that accepts the last cloud's center walks on
                    # to the collapsed maximum in the same launch: its guard ends the
                    # view.  One-center steps of the adaptive run meet the collapse
                    # inside a batch or at its end, where the next view is simply
                    # built lower: no exit to count there)
                    if cutoff == 0.0 and cands in (16, 8):
                        assert vs["guard_exits"] >= 1, (cands, vs)


@pytest.mark.parametrize("cands", [16, -1])
def test_continuous_data(ocl, cands):
    """one time-ordered walk: no gap in the distances, frames on both sides of
    every theta -- the empirical check of the margin"""
    x = synth.walk(4000, 20, 3)
    want = ocl.kcenters(x, n_clusters=64)
    r, vs = _fit(x, 64, 0.0, cands, 2)
    _same(r, want)
    assert vs["views"] > 0, vs


def test_ties(ocl):
    """every frame twice, at shuffled positions: equal maxima all along, and the
    first of them by position must be the center (the view keeps the order)"""
    rng = np.random.RandomState(5)
    x = _clouds(12, 25, 20, seed=31)
    x = np.concatenate([x, x])
    x = np.ascontiguousarray(x[rng.permutation(len(x))])
    want = ocl.kcenters(x, n_clusters=40)
    for cands in FORMS:
        r, vs = _fit(x, 40, 0.0, cands, 2)
        _same(r, want)
        assert vs["views"] > 0 or cands == 1, vs


def test_view_smaller_than_a_tile_and_a_wave(ocl):
    """three clouds and five outliers: after three centers the view holds the
    outliers alone"""
    x = _clouds(3, 300, 20, seed=41, shuffle=False)
    out = _clouds(5, 1, 20, seed=77, shuffle=False)
    x = np.concatenate([x, out])
    x = np.ascontiguousarray(x[np.random.RandomState(6).permutation(len(x))])
    want = ocl.kcenters(x, n_clusters=12)
    for cands in FORMS:
        r, vs = _fit(x, 12, 0.0, cands, 2)
        _same(r, want)
        assert vs["views"] > 0 or cands == 1, vs


def test_continuation_and_neighbours(ocl, monkeypatch):
    from enspara_amd.cluster import KHybrid
    from enspara_amd.device import FrameStore
    x = _clouds(40, 61, 20, seed=20)
    want = ocl.kcenters(x, n_clusters=30)
    states = {}
    for view in (0, 2):
        with _store(x) as st:
            st.set_option("active_view", view)
            st.reset_state()
            i1, d1, _ = st.kcenters_run(0, 17, 0.0)
            s1 = st.download_state()
            i2, d2, m2 = st.kcenters_run(17, 13, 0.0)
            s2 = st.download_state()
        assert [int(i) for i in i1] + [int(i) for i in i2] == [int(i) for i in want[0]]
        np.testing.assert_array_equal(s2[1], want[1])
        np.testing.assert_array_equal(s2[0], want[2].astype(np.float32))
        states[view] = (s1, s2, np.concatenate([d1, d2]), m2)
    for a, b in zip(states[0][:2], states[2][:2]):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(states[0][2], states[2][2])
    assert states[0][3] == states[2][3]

    # k-hybrid: the fit inside KHybrid with the option 0 and 2
    make = FrameStore.from_array.__func__
    fits = {}
    for view in (0, 2):
        def from_array(cls, X, *a, _view=view, **kw):
            st = make(cls, X, *a, **kw)
            st.set_option("active_view", _view)
            return st
        monkeypatch.setattr(FrameStore, "from_array", classmethod(from_array))
        fits[view] = KHybrid("rmsd", n_clusters=30, kmedoids_updates=2,
                             random_state=0).fit(x)
    monkeypatch.undo()
    assert list(fits[0].center_indices_) == list(fits[2].center_indices_)
    np.testing.assert_array_equal(fits[0].labels_, fits[2].labels_)
    np.testing.assert_array_equal(fits[0].distances_, fits[2].distances_)


def test_no_view_where_none_belongs(ocl):
    # iid coordinates: every frame about as far from every other; nothing settles
    rng = np.random.RandomState(11)
    x = rng.normal(size=(3000, 12, 3)).astype(np.float32)
    want = ocl.kcenters(x, n_clusters=48)
    r, vs = _fit(x, 48, 0.0, -1, 1)
    _same(r, want)
    assert vs["views"] == 0, vs
    # two atoms: RMSD over rotations of a pair is no use as a metric here
    x2 = _clouds(10, 50, 2, seed=2)
    r, vs = _fit(x2, 20, 0.0, -1, 2)
    _same(r, ocl.kcenters(x2, n_clusters=20))
    assert vs["views"] == 0, vs
    # the triangle option on: its kernels read the history as positions
    x3 = _clouds(40, 61, 20, seed=20)
    want3 = ocl.kcenters(x3, n_clusters=30)
    r, vs = _fit(x3, 30, 0.0, 16, 2, tri=True)
    _same(r, want3)
    assert vs["views"] == 0, vs
    # an uploaded state: the distances are the caller's numbers
    with _store(x3) as st:
        st.set_option("active_view", 2)
        st.reset_state()
        i1, _, _ = st.kcenters_run(0, 10, 0.0)
        d, a = st.download_state()
        st.upload_state(d, a)
        i2, _, _ = st.kcenters_run(10, 20, 0.0)
        vs = st.view_stats()
        d, a = st.download_state()
    assert [int(i) for i in i1] + [int(i) for i in i2] == [int(i) for i in want3[0]]
    np.testing.assert_array_equal(a, want3[1])
    np.testing.assert_array_equal(d, want3[2].astype(np.float32))
    assert vs["views"] == 0, vs
