"""Dye labelling on the device (csrc/ek_dyes.hip) against the numpy model
(tests/_numpy_dyes.py) and the reference's recorded outputs (tests/golden/dyes_golden.npz):
exact equality throughout -- kept points, bin counts, and the float64 probabilities made
from them by the same numpy expressions.

Shapes: one lane per point in workgroups of 256 (points 1, 63, 65, 257, 1025), atoms
staged 1024 at a time (1, 63, 64, 65, 300, and 1100 for a second batch); pairs in
workgroups of 256 points of the larger cloud, chunks of 2048 points above 5e7 pairs."""
import contextlib
import gc
import os

import numpy as np
import pytest

import _numpy_dyes as nd
from _lifetime_cases import bits
from enspara_amd import _lib
from enspara_amd.exception import DataInvalid, InsufficientResourceError
from enspara_amd.geometry import dyes_from_expt_dist as dyes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FAILED = (_lib.HipError, InsufficientResourceError)


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "dyes_golden.npz"))


# ---- touches -------------------------------------------------------------------------------
@pytest.mark.parametrize("atoms", [1, 63, 64, 65, 300, 1100])
@pytest.mark.parametrize("points", [1, 63, 65, 257, 1025])
def test_touches_against_the_model(atoms, points):
    rng = np.random.RandomState(1000 * atoms + points)
    side = max(0.5, (atoms / 40.0) ** (1 / 3.))        # about 40 atoms per nm^3
    xyz = (rng.rand(atoms, 3) * side).astype(np.float32)
    radii = 0.12 + 0.08 * rng.rand(atoms)
    coords = nd.ball(rng, points, 0.5 * side + 0.4, centre=(side / 2,) * 3)
    mask = nd.keep_mask(coords, xyz, radii + 0.17)
    got = dyes.remove_touches_protein(coords, xyz, radii)
    assert got.dtype == np.float32 and np.array_equal(got, coords[mask])
    if points >= 257:
        assert 0 < mask.sum() < points


def test_touch_exactly_at_the_cutoff():
    xyz = np.zeros((1, 3), dtype=np.float32)
    at = np.float32(0.375)
    out = np.nextafter(at, np.float32(1))
    coords = np.array([[at, 0, 0], [out, 0, 0], [0, -at, 0], [0, -out, 0], [0, 0, at],
                       [0, 0, out], [1, 1, 1], [0, 0, 0]], dtype=np.float32)
    got = dyes.remove_touches_protein(coords, xyz, np.array([0.25]), probe_radius=0.125)
    assert np.array_equal(got, coords[[1, 3, 5, 6]])
    # a cutoff that is no float32 and whose square is inexact
    cutoff = 0.2 + 0.17
    assert np.array_equal(
        dyes.remove_touches_protein(coords, xyz, np.array([0.2])),
        coords[nd.keep_mask(coords, xyz, np.array([cutoff]))])


def test_touches_all_none_and_order():
    rng = np.random.RandomState(5)
    xyz = (rng.rand(50, 3) * 0.5).astype(np.float32)
    radii = np.full(50, 0.17)
    inside = nd.ball(rng, 300, 0.1, centre=(0.25, 0.25, 0.25))
    got = dyes.remove_touches_protein(inside, xyz, radii)
    assert got.shape == (0, 3) and got.dtype == np.float32
    outside = nd.ball(rng, 300, 0.5, centre=(5.0, 5.0, 5.0))
    assert np.array_equal(dyes.remove_touches_protein(outside, xyz, radii), outside)
    # kept and removed points interleaved, several workgroups: the order stays
    mixed = np.empty((600, 3), dtype=np.float32)
    mixed[0::2], mixed[1::2] = outside, inside
    assert np.array_equal(dyes.remove_touches_protein(mixed, xyz, radii), outside)


def test_touches_goldens(G):
    kept = dyes.remove_touches_protein(G["rt_coords"], G["pep_xyz"], G["pep_radii"],
                                       probe_radius=float(G["rt_probe"]))
    assert np.array_equal(kept, G["rt_coords"][G["rt_kept"]])
    # above the reference's own chunking threshold: 170 000 points
    big = nd.touch_cloud(int(G["rtc_seed"]), int(G["rtc_n"]), float(G["rtc_radius"]),
                         G["pep_xyz"][150])
    kept = dyes.remove_touches_protein(big, G["pep_xyz"], G["pep_radii"])
    # (the golden holds the reference's count and index sum, not its 120 000 indices: the
    # model is held to those, the device to the model)
    mask = nd.keep_mask(big, G["pep_xyz"], G["pep_radii"] + 0.17)
    assert mask.sum() == int(G["rtc_count"])
    assert int(np.flatnonzero(mask).sum()) == int(G["rtc_index_sum"])
    assert np.array_equal(kept, big[mask])


# ---- pair histograms -------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 257]


@pytest.mark.parametrize("n1", SIZES)
@pytest.mark.parametrize("n2", SIZES)
def test_pair_histogram_against_the_model(n1, n2):
    rng = np.random.RandomState(100 * n1 + n2)
    a, b = nd.ball(rng, n1, 1.3), nd.ball(rng, n2, 0.9, centre=(1.5, -0.7, 0.4))
    probs, edges = dyes.pairwise_distance_distribution(a, b, bin_width=0.1)
    m_probs, m_edges = nd.pair_distribution(a, b, 0.1)
    assert np.array_equal(edges, m_edges) and np.array_equal(probs, m_probs)


def test_pair_histogram_distances_on_the_edges():
    w = 0.125
    a = np.zeros((21, 3), dtype=np.float32)
    b = np.zeros((300, 3), dtype=np.float32)
    a[:, 0] = np.arange(21) * w
    b[:, 0] = (np.arange(300) % 31) * w + 3.0
    b[:, 1] = 0.0
    probs, edges = dyes.pairwise_distance_distribution(a, b, bin_width=w)
    m_probs, m_edges = nd.pair_distribution(a, b, w)
    assert np.array_equal(edges, m_edges) and np.array_equal(probs, m_probs)
    # every distance is an edge: it counts in the bin that starts there
    d = nd.distances(a, b).reshape(-1)
    assert np.all(d == np.round(d / w) * w)
    want = np.bincount(np.round(d / w).astype(int), minlength=len(probs))
    assert np.array_equal(probs, dyes.int_norm_hist(edges, want))
    # the same distances off the axes (3-4-5 triangles) and a width that is no power of two
    a2 = np.array([[0, 0, 0], [0.3, 0.4, 0]], dtype=np.float32)
    b2 = np.array([[0.3, 0.4, 0], [0.6, 0.8, 0], [0, 0, 1.2], [0.5, 0, 0]], dtype=np.float32)
    for width in (0.1, 0.05, 0.25):
        probs, edges = dyes.pairwise_distance_distribution(a2, b2, bin_width=width)
        m_probs, m_edges = nd.pair_distribution(a2, b2, width)
        assert np.array_equal(edges, m_edges) and np.array_equal(probs, m_probs)


def test_pair_histogram_of_coincident_points():
    a = np.full((70, 3), 1.25, dtype=np.float32)
    probs, edges = dyes.pairwise_distance_distribution(a, a[:5], bin_width=0.1)
    assert np.array_equal(edges, np.linspace(0, 0.2, 3))
    assert np.array_equal(probs, dyes.int_norm_hist(edges, np.array([350, 0])))


def test_pair_histogram_unchunked_golden(G):
    probs, edges = dyes.pairwise_distance_distribution(G["pd_a"], G["pd_b"],
                                                       bin_width=float(G["pd_width"]))
    assert np.array_equal(probs, G["pd_probs"]) and np.array_equal(edges, G["pd_edges"])


def test_pair_histogram_chunked_golden(G):
    a, b = nd.chunk_clouds(int(G["pc_seed"]), int(G["pc_n1"]), int(G["pc_n2"]))
    probs, edges = dyes.pairwise_distance_distribution(a, b, bin_width=float(G["pc_width"]))
    assert np.array_equal(edges, G["pc_edges"]) and np.array_equal(probs, G["pc_probs"])
    # the other way round the same chunks are cut: the larger cloud's
    probs, edges = dyes.pairwise_distance_distribution(b, a, bin_width=float(G["pc_width"]))
    assert np.array_equal(edges, G["pc_edges"]) and np.array_equal(probs, G["pc_probs"])


@pytest.mark.parametrize("n1,n2", [(4097, 12300), (7072, 7072)])
def test_pair_histogram_chunked_against_the_model(n1, n2):
    assert n1 * n2 > nd.ONE_CHUNK_PAIRS
    a, b = nd.chunk_clouds(n1 + n2, n1, n2)
    counts, per_chunk = nd.pair_counts(a, b, 0.1)
    assert len(set(per_chunk)) == 2 and per_chunk[-1] == max(per_chunk) > per_chunk[0]
    probs, edges = dyes.pairwise_distance_distribution(a, b, bin_width=0.1)
    m_edges = np.linspace(0, len(counts) * 0.1, len(counts) + 1)
    assert np.array_equal(edges, m_edges)
    assert np.array_equal(probs, nd.int_norm_hist(m_edges, counts))


# ---- the trajectory call ---------------------------------------------------------------------
def _trajectory(G, frames):
    rng = np.random.RandomState(31)
    xyz = np.stack([G["pep_xyz"]] * frames)
    xyz[1:] += (0.02 * rng.randn(frames - 1, xyz.shape[1], 3)).astype(np.float32)
    bbs = np.array([dyes.backbone_indices(G["pep_names"], G["pep_seqs"], int(r))
                    for r in G["e2e_res"]])
    return xyz, bbs


@pytest.mark.parametrize("frames", [1, 3, 5])
def test_trajectory_against_model_and_golden(G, frames):
    xyz, bbs = _trajectory(G, frames)
    probs, edges = dyes.dye_distance_distribution(
        xyz, G["pep_radii"], G["e2e_dye1"], G["e2e_dye2"], bbs, chunk_frames=2)
    assert len(probs) == len(edges) == frames
    assert np.array_equal(probs[0], G["e2e_probs"]) and np.array_equal(edges[0], G["e2e_edges"])
    for f in range(frames):
        m_probs, m_edges, _, _ = nd.frame_distribution(
            xyz[f], G["pep_radii"] + 0.2, G["e2e_dye1"], G["e2e_dye2"], bbs, 0.1)
        assert np.array_equal(probs[f], m_probs), f
        assert np.array_equal(edges[f], m_edges), f
    ms = dyes.last_labelling_timing()
    assert ms.shape == (4,) and np.all(ms > 0)
    # the same whatever the chunks of frames
    again, _ = dyes.dye_distance_distribution(
        xyz, G["pep_radii"], G["e2e_dye1"], G["e2e_dye2"], bbs)
    assert bits(again) == bits(probs)


def test_trajectory_is_the_stages_frame_by_frame(G):
    xyz, bbs = _trajectory(G, 3)
    radii, d1, d2 = G["pep_radii"], G["e2e_dye1"], G["e2e_dye2"]
    probs, edges = dyes.dye_distance_distribution(xyz, radii, d1, d2, bbs, chunk_frames=2)
    for f in range(3):
        kept = [dyes.remove_touches_protein(dyes.align_dye_to_res(xyz[f], d, bb), xyz[f],
                                            radii, probe_radius=0.2)
                for d in (d1, d2) for bb in bbs]
        if f == 0:
            for p in range(4):
                assert len(kept[p]) == len(G["e2e_kept%d" % p])
        p1, e1 = dyes.pairwise_distance_distribution(kept[0], kept[3])
        p2, e2 = dyes.pairwise_distance_distribution(kept[1], kept[2])
        p, e = dyes._merge_histograms([p1, p2], [e1, e2], weights=[0.5, 0.5])
        assert np.array_equal(probs[f], p) and np.array_equal(edges[f], e)


def _buried(G):
    """three frames; in frame 1 an atom far along the chain sits in the middle of a small
    cloud on the first residue, and nothing of placement 0 is left"""
    xyz, bbs = _trajectory(G, 3)
    rng = np.random.RandomState(8)
    small = nd.ball(rng, 70, 0.05, centre=(0, 0, 1.0))
    M, t = dyes.determine_rot_mat(xyz[1], bbs[0])
    xyz[1, -1] = nd.align(np.array([[0, 0, 1.0]], dtype=np.float32), M, t)[0]
    return xyz, bbs, small


def test_empty_placement_names_the_frame(G):
    xyz, bbs, small = _buried(G)
    cutoff = G["pep_radii"] + 0.2
    for f in range(3):
        M, t = nd.rot_mat(xyz[f], bbs[0])
        kept = nd.keep_mask(nd.align(small, M, t), xyz[f], cutoff).sum()
        assert (kept == 0) == (f == 1), (f, kept)
    with pytest.raises(DataInvalid, match=r"Frame 1: every point of placement 0 \(dye1 on "
                                         r"residue 0\)"):
        dyes.dye_distance_distribution(xyz, G["pep_radii"], small, G["e2e_dye2"], bbs,
                                       chunk_frames=2)


def test_output_feeds_the_burst_simulation(G):
    xyz, bbs = _trajectory(G, 3)
    probs, edges = dyes.dye_distance_distribution(
        xyz, G["pep_radii"], G["e2e_dye1"], G["e2e_dye2"], bbs)
    dist = dyes.make_distribution(probs, edges)
    T = np.array([[0.8, 0.1, 0.1], [0.2, 0.7, 0.1], [0.3, 0.3, 0.4]])
    pops = np.array([0.5, 0.3, 0.2])
    bursts = [[0, 3, 3, 9, 20], [1, 2, 40], [5]]
    FEs, trajs = dyes.sample_FRET_histograms(T, pops, dist, bursts, R0=5.4, random_state=3)
    assert FEs.shape == (3, 2) and np.all((FEs[:, 0] >= 0) & (FEs[:, 0] <= 1))
    assert [len(t) for t in trajs] == [21, 41, 6]
    again, _ = dyes.sample_FRET_histograms(T, pops, dist, bursts, R0=5.4, random_state=3)
    assert np.array_equal(again[:, 0], FEs[:, 0])


# ---- what a call leaves behind (the three properties of tests/test_gpu_lifetime.py) ----------
def _live():
    return tuple(_lib.live_resources())[:6]


def _baseline():
    gc.collect()
    return _live()


def _calls(G):
    xyz, bbs = _trajectory(G, 3)
    a, b = nd.ball(np.random.RandomState(2), 300, 1.0), nd.ball(np.random.RandomState(3), 65, 1.0)
    return {
        "remove_touches_protein": lambda: dyes.remove_touches_protein(
            G["rt_coords"], G["pep_xyz"], G["pep_radii"]),
        "pairwise_distance_distribution": lambda: dyes.pairwise_distance_distribution(a, b),
        "dye_distance_distribution": lambda: dyes.dye_distance_distribution(
            xyz, G["pep_radii"], G["e2e_dye1"], G["e2e_dye2"], bbs, chunk_frames=2),
    }


ENTRY_POINTS = ["remove_touches_protein", "pairwise_distance_distribution",
                "dye_distance_distribution"]


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_balance(G, name):
    call = _calls(G)[name]
    first = bits(call())                            # warm-up
    before = _baseline()
    for _ in range(3):
        assert bits(call()) == first
    assert _live() == before


def test_raise_path_balance(G):
    xyz, bbs, small = _buried(G)

    def call():
        dyes.dye_distance_distribution(xyz, G["pep_radii"], small, G["e2e_dye2"], bbs,
                                       chunk_frames=2)
    with pytest.raises(DataInvalid):                # warm-up
        call()
    before = _baseline()
    for _ in range(3):
        with pytest.raises(DataInvalid):
            call()
    assert _live() == before


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_injected_allocation_failure(G, name):
    call = _calls(G)[name]
    want = bits(call())                             # warm-up, and the bytes to return
    base = _baseline()
    t0 = _lib.live_resources().dev_allocs_total
    assert bits(call()) == want
    n_allocs = _lib.live_resources().dev_allocs_total - t0
    assert _live() == base
    print("%s: %d device allocations" % (name, n_allocs))
    assert 0 < n_allocs <= 40
    for k in range(n_allocs):
        assert _lib.fail_alloc_at(k) == -1
        with contextlib.ExitStack() as stack:
            stack.callback(_lib.fail_alloc_at, -1)
            with pytest.raises(FAILED):
                call()
            pending = _lib.fail_alloc_at(-1)
        assert pending == -1, "allocation %d: the arm is still set" % k
        assert _live() == base, "allocation %d" % k
        assert bits(call()) == want, "the clean call after allocation %d" % k
