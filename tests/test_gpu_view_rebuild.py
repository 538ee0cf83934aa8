"""A rebuild of the active view (csrc/ek_view.hip): the gather writes the view's quad
copy itself, its frame-minor tiles are made on demand, the policy's look rides on
the batch, and the policy's two numbers are options.  Layouts are compared on the
device word for word with the earlier path (``ek_view_layout_check``); fits run
with the view's buffers filled with 0xFF bytes before every rebuild (option value
3) and are compared with the CPU oracle bit for bit."""
import numpy as np
import pytest

from enspara_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ocl():
    from oracle import cluster
    return cluster


def _store(x):
    from enspara_amd.device import FrameStore
    return FrameStore.from_array(x)


def _clouds(n_templates, per, A, seed, sigma=0.05):
    """`per` noisy copies of each of `n_templates` chains, in random order"""
    rng = np.random.RandomState(seed)
    tmpl = synth.templates(n_templates, A, seed + 100)
    x = np.concatenate([tmpl[t] + rng.normal(scale=sigma, size=(per, A, 3))
                        for t in range(n_templates)]).astype(np.float32)
    return np.ascontiguousarray(x[rng.permutation(len(x))])


_WANT = {}


def _oracle(ocl, A, n_clusters=60, cutoff=None):
    """the clouds of `A` atoms and the oracle's fit of them, computed once"""
    key = (A, n_clusters, cutoff)
    if key not in _WANT:
        x = _clouds(40, 61, A, seed=A)
        _WANT[key] = (x, ocl.kcenters(x, n_clusters=n_clusters, dist_cutoff=cutoff))
    return _WANT[key]


def _same(idx, labels, dist, want):
    assert [int(i) for i in idx] == [int(i) for i in want[0]]
    np.testing.assert_array_equal(labels, want[1])
    np.testing.assert_array_equal(dist, want[2].astype(np.float32))


def _fit(x, n_clusters, cutoff, cands, view, rho=None, ratio=None):
    from enspara_amd.cluster import kcenters as kc
    with _store(x) as st:
        st.set_option("candidates", cands)
        st.set_option("active_view", view)
        if rho is not None:
            st.set_option("view_rho", rho)
            st.set_option("view_ratio", ratio)
        r = kc._kcenters_device(x, n_clusters, cutoff, None, 0, store=st)
        return r, st.view_stats()


N_V = (1, 255, 256, 257, 513)


@pytest.mark.parametrize("cands", [16, 8])
@pytest.mark.parametrize("A", [3, 4, 5, 15, 16, 17, 33, 63, 64, 65, 68])
def test_layout(A, cands):
    """every A mod 4 (16-byte and 4-byte rows), both sides of 16 atoms and of the
    staging chunk of 64, with either kind of row; views inside one wave and either
    side of one and of two tiles.  A store that only ever ran rounds of 8 has no quad
    copy: its rebuild writes the frame-minor tiles directly (the second form of the
    kernel)."""
    x = _clouds(40, 61, A, seed=A)
    with _store(x) as st:
        st.set_option("candidates", cands)
        st.set_option("active_view", 0)
        st.reset_state()
        st.kcenters_run(0, 10, 0.0)
        d, a = st.download_state()
        top = np.sort(d)[::-1]
        for n_v in N_V:
            theta = float(top[n_v])
            assert np.count_nonzero(d > np.float32(theta)) == n_v, "a tie at the cut"
            got = st.view_layout_check(theta)
            print(A, cands, n_v, got)
            assert got == (n_v, 0, 0, 0)
        d2, a2 = st.download_state()
    np.testing.assert_array_equal(d, d2)
    np.testing.assert_array_equal(a, a2)


@pytest.mark.parametrize("A", [3, 5, 17, 20])
def test_fits_with_poisoned_views(ocl, A):
    """rebuilt every other round into buffers of 0xFF bytes: a padding slot or an atom
    past the last that a rebuild leaves unwritten is a NaN in the matrix loop"""
    for n_clusters, cutoff in ((60, None), (None, 0.17)):
        x, want = _oracle(ocl, A, n_clusters, cutoff)
        for cands in (16, 8, -1):
            r, vs = _fit(x, n_clusters or np.inf, cutoff or 0.0, cands, 3)
            _same(r.center_indices, r.assignments, r.distances, want)
            if cands in (16, 8):
                assert vs["views"] > 0 and vs["left_out"] > 0, (cands, vs)


def test_tiles_on_demand(ocl):
    """rounds of 16 leave a view without frame-minor tiles; the rounds of 8 and the
    adaptive run that follow on the same store read them"""
    x, want = _oracle(ocl, 20)
    idx = []
    with _store(x) as st:
        st.set_option("active_view", 3)
        st.reset_state()
        for first, cands in ((0, 16), (20, 8), (40, -1)):
            st.set_option("candidates", cands)
            i, _, _ = st.kcenters_run(first, 20, 0.0)
            idx += [int(v) for v in i]
            assert st.view_stats()["views"] > 0 or cands == -1
        d, a = st.download_state()
    _same(idx, a, d, want)


def test_the_look(ocl):
    # iid coordinates: nothing settles, every look finds as much and the looks pause
    rng = np.random.RandomState(11)
    x = rng.normal(size=(3000, 12, 3)).astype(np.float32)
    want = ocl.kcenters(x, n_clusters=48)
    r, vs = _fit(x, 48, 0.0, -1, 1)
    _same(r.center_indices, r.assignments, r.distances, want)
    assert vs["views"] == 0, vs
    # the clouds: the policy is free to build none at this size
    x, want = _oracle(ocl, 20)
    r, vs = _fit(x, 60, 0.0, -1, 1)
    _same(r.center_indices, r.assignments, r.distances, want)
    assert vs["views"] >= 0, vs


def test_option_keys(ocl):
    from enspara_amd._lib import HipError
    x, want = _oracle(ocl, 20)
    with _store(x) as st:
        assert st.get_option("view_rho") == 750 and st.get_option("view_ratio") == 800
        for key in ("view_rho", "view_ratio"):
            for v in (500, 625, 950):
                st.set_option(key, v)
                assert st.get_option(key) == v
            for v in (499, 951, 0, -1, 1000):
                with pytest.raises(HipError):
                    st.set_option(key, v)
                assert st.get_option(key) == 950
        st.set_option("active_view", 3)
        assert st.get_option("active_view") == 3
        with pytest.raises(HipError):
            st.set_option("active_view", 4)
    for rho in (500, 950):
        for ratio in (700, 900):
            for cands in (16, -1):
                r, vs = _fit(x, 60, 0.0, cands, 1, rho, ratio)
                _same(r.center_indices, r.assignments, r.distances, want)
