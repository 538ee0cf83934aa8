"""geometry.pockets on the device: the touch, line-extent, rank, labelling and compaction
kernels of csrc/ek_pockets.hip.

No expected value comes from a device call: everything is compared, with array_equal,
with the numpy restatement tests/_numpy_pockets.py, which tests/test_pockets_host.py holds
to what the reference's own functions gave (tests/golden/pockets_golden.npz).  Every test
asserts, on the restatement's values, the condition that makes it a check."""
import functools
import os

import numpy as np
import pytest

import _numpy_pockets as npk
from enspara_amd.geometry import pockets

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "pockets_golden.npz"))
E = np.load(os.path.join(HERE, "golden", "exposons_golden.npz"))
BP_XYZ = np.ascontiguousarray(E["bp_xyz"][:6])
BP_RADII = npk.radii_of(E["bp_elements"])
FIXTURES = {"shell%d" % k: (G["shell%d_xyz" % k], npk.radii_of(G["shell%d_elements" % k]))
            for k in range(3)}
for _f in range(6):
    FIXTURES["bp%d" % _f] = (BP_XYZ[_f], BP_RADII)


@functools.lru_cache(maxsize=None)
def stages(name, spacing, probe):
    """origin, dims, touches, ranks of a named frame by the restatement, computed once"""
    xyz, radii = FIXTURES[name]
    origin, dims = npk.grid_of(xyz, spacing)
    T = npk.touches(xyz, probe + radii, spacing, origin, dims)
    T.setflags(write=False)
    R = npk.ranks(T)
    R.setflags(write=False)
    return origin, dims, T, R


@functools.lru_cache(maxsize=None)
def expected(name, spacing, probe, min_rank, min_cluster_size=0):
    origin, dims, T, R = stages(name, spacing, probe)
    out = dict(origin=origin, dims=dims, touches=T, ranks=R)
    out.update(npk.pockets_of_ranks(R, min_rank, min_cluster_size))
    return out


def check_frame(got, want, spacing):
    assert got.shape == tuple(int(d) for d in want["dims"])
    assert got.origin.dtype == np.float32 and np.array_equal(got.origin, want["origin"])
    assert got.cells.dtype == np.float64 and got.cells.shape == (len(want["cells"]), 3)
    assert np.array_equal(got.cells,
                          npk.coordinates(want["cells"], want["origin"], want["dims"], spacing))
    assert np.array_equal(got.pocket_ids, want["ids"])


def check_against_restatement(xyz, radii, spacing, probe, min_rank, min_cluster_size=0, **kw):
    """get_pockets of frames that have no name"""
    got = pockets.get_pockets(xyz, radii, spacing, probe, min_rank, min_cluster_size, **kw)
    want = [npk.frame_pockets(x, radii, spacing, probe, min_rank, min_cluster_size) for x in xyz]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        check_frame(g, w, spacing)
    return got, want


# ---- the beta-peptide frames: one call, frames of different grids, chunks ----------------
@pytest.mark.parametrize("chunk_frames", [1, 2, 5, None])
def test_beta_peptide_frames_in_one_call(chunk_frames):
    for spacing, probe, min_rank in [(0.1, 0.07, 3), (0.1, 0.14, 5), (0.07, 0.14, 3)]:
        want = [expected("bp%d" % f, spacing, probe, min_rank) for f in range(6)]
        assert len(set(tuple(w["dims"]) for w in want)) > 1
        assert sum(len(w["cells"]) > 0 for w in want) >= 5
        if min_rank == 3:
            for w in want:
                sizes = np.bincount(w["ids"])
                assert len(sizes) >= 2 and sizes[0] > sizes[-1]
        got = pockets.get_pockets(BP_XYZ, BP_RADII, spacing, probe, min_rank,
                                  chunk_frames=chunk_frames)
        assert len(got) == 6
        for g, w in zip(got, want):
            check_frame(g, w, spacing)
        vol = pockets.pocket_volumes(got, spacing)
        for v, w in zip(vol, want):
            assert np.array_equal(v, np.bincount(w["ids"]) * spacing ** 3 if len(w["ids"])
                                  else np.zeros(0))
    t = pockets.last_timing()
    assert t.shape == (4,) and np.all(t >= 0) and t[1:].sum() > 0


def test_defaults_are_the_references():
    got = pockets.get_pockets(BP_XYZ, BP_RADII)
    for f, g in enumerate(got):
        check_frame(g, expected("bp%d" % f, 0.1, 0.14, 5), 0.1)
    want = expected("bp5", 0.1, 0.07, 3)
    assert len(want["flat"]) > 0
    cells = pockets.get_pocket_cells(BP_XYZ[5], BP_RADII)
    assert np.array_equal(cells, npk.coordinates(want["flat"], want["origin"], want["dims"], 0.1))


# ---- the shells: every rank, every threshold --------------------------------------------
@pytest.mark.parametrize("name", ["shell0", "shell1", "shell2"])
@pytest.mark.parametrize("probe", [0.14, 0.07])
def test_shells(name, probe):
    xyz, radii = FIXTURES[name]
    origin, dims, T, R = stages(name, 0.1, probe)
    case = "%s_%s" % (name, "a" if probe == 0.14 else "b")
    assert np.array_equal(R, G[case + "_ranks"])        # the reference's own
    if probe == 0.07:
        assert set(np.unique(R)) == set(range(8))
    assert np.array_equal(pockets.determine_touches_protein(xyz, radii, 0.1, probe), T)
    assert np.array_equal(pockets.rank_cells(T), R)
    for min_rank in range(1, 9):
        largest = int(np.bincount(expected(name, 0.1, probe, min_rank)["ids"]).max(initial=0))
        assert (largest > 0) == (min_rank < 8)
        for mcs in (0, 1, largest):
            want = expected(name, 0.1, probe, min_rank, mcs)
            got = pockets.get_pockets(xyz[None], radii, 0.1, probe, min_rank, mcs)
            check_frame(got[0], want, 0.1)
            if mcs == largest:
                assert len(got[0].cells) == 0
    assert len(expected(name, 0.1, probe, 5)["cells"]) >= 18


def test_shifted_by_100_nm():
    """far from the origin float32 coordinates are coarse (2^-17 nm); the cells' float64
    coordinates must still decide every cell as the restatement does"""
    xyz, radii = FIXTURES["shell0"]
    far = (xyz + np.float32(100.0))[None]
    got, want = check_against_restatement(far, radii, 0.1, 0.07, 3)
    assert len(want[0]["cells"]) > 100 and want[0]["origin"].min() > 99
    assert np.array_equal(pockets.determine_touches_protein(far[0], radii, 0.1, 0.07),
                          want[0]["touches"])


# ---- where the kernels change form -------------------------------------------------------
def _round_shell(atoms, seed):
    rng = np.random.RandomState(seed)
    v = rng.normal(size=(atoms, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    xyz = (v * rng.uniform(0.3, 0.4, size=(atoms, 1))).astype(np.float32)
    return xyz, npk.radii_of(rng.choice(["H", "C", "N", "O"], size=atoms))


def test_a_fine_grid():
    """every axis and the diagonals longer than 64 cells, more than 65 536 cells in the
    frame, not a multiple of 256"""
    xyz, radii = _round_shell(40, 5)
    spacing = 0.009
    got, want = check_against_restatement(xyz[None], radii, spacing, 0.07, 5)
    dims = want[0]["dims"]
    assert dims.min() > 64 and dims.prod() > 65536 and dims.prod() % 256 != 0
    assert set(np.unique(want[0]["ranks"])) == set(range(8))
    sizes = np.bincount(want[0]["ids"])
    assert len(sizes) >= 2 and sizes[0] > 1000 and sizes[0] > sizes[-1]
    assert np.array_equal(pockets.rank_cells(want[0]["touches"]), want[0]["ranks"])
    assert np.array_equal(pockets.determine_touches_protein(xyz, radii, spacing, 0.07),
                          want[0]["touches"])


@pytest.mark.parametrize("atoms", [1, 2, 63, 64, 65])
def test_numbers_of_atoms(atoms):
    xyz, radii = BP_XYZ[:3, :atoms], BP_RADII[:atoms]
    got, want = check_against_restatement(xyz, radii, 0.1, 0.07, 1)
    if atoms == 1:
        assert all(g.shape == (0, 0, 0) and len(g.cells) == 0 for g in got)
        assert pockets.determine_touches_protein(xyz[0], radii, 0.1, 0.07).shape == (0, 0, 0)
        return
    for x, w in zip(xyz, want):
        assert w["dims"].min() >= 1 and w["touches"].any()
        assert np.array_equal(pockets.determine_touches_protein(x, radii, 0.1, 0.07),
                              w["touches"])
    if atoms >= 63:
        assert all(len(w["cells"]) > 0 for w in want)


def test_degenerate_frames():
    """collinear or coplanar along an axis: n == 0 there, no cells, no pockets -- also among
    ordinary frames of the same call; an axis of one cell is computed as any other"""
    xyz = np.repeat(BP_XYZ[:1], 5, axis=0).copy()
    xyz[1, :, 2] = 0.25                     # coplanar: nz == 0
    xyz[2, :, 1:] = 1.5                     # collinear along x: ny == nz == 0
    xyz[3, :, 2] = 0.25                     # one cell along z
    xyz[3, ::2, 2] += np.float32(0.04)
    xyz[4] = BP_XYZ[1]
    for chunk in (None, 1, 2):
        got, want = check_against_restatement(xyz, BP_RADII, 0.1, 0.07, 1, chunk_frames=chunk)
    assert got[1].shape[2] == 0 and got[1].shape[0] > 0 and len(got[1].cells) == 0
    assert got[2].shape[1:] == (0, 0) and len(got[2].cells) == 0
    assert got[3].shape[2] == 1 and want[3]["ranks"].max() >= 1 and len(got[3].cells) > 0
    assert len(got[0].cells) > 0 and len(got[4].cells) > 0
    assert np.array_equal(pockets.rank_cells(want[3]["touches"]), want[3]["ranks"])


# ---- the rank kernels alone ----------------------------------------------------------------
def test_rank_cells_two_plates():
    T = np.zeros((6, 8, 8), dtype=bool)
    T[1], T[4] = True, True
    want = npk.ranks(T)
    # between the plates: the x scan and every diagonal that meets both plates
    assert want[2, 4, 3] == 5 and want.max() == 5 and want[0].max() == 0 and want[5].max() == 0
    assert len(np.unique(want)) >= 4
    assert np.array_equal(pockets.rank_cells(T), want)
    for axes in [(1, 0, 2), (2, 1, 0), (1, 2, 0)]:
        assert np.array_equal(pockets.rank_cells(T.transpose(axes)),
                              npk.ranks(T.transpose(axes)))


def test_rank_cells_one_touching_cell_per_line():
    """one touching cell on a line surrounds nothing"""
    T = np.zeros((6, 6, 6), dtype=bool)
    T[2, 3, 4] = True
    assert npk.ranks(T).max() == 0
    assert np.array_equal(pockets.rank_cells(T), np.zeros(T.shape, dtype=np.uint8))
    T[4, 1, 0] = True       # shares no line with the first
    assert npk.ranks(T).max() == 0
    assert np.array_equal(pockets.rank_cells(T), np.zeros(T.shape, dtype=np.uint8))
    assert pockets.rank_cells(np.ones((5, 4, 3), dtype=bool)).max() == 0
    assert pockets.rank_cells(np.zeros((5, 4, 3), dtype=bool)).max() == 0


@pytest.mark.parametrize("ends, cell", [
    (((0, 0, 1), (2, 2, 3)), (1, 1, 2)),        # (1, 1, 1)
    (((3, 0, 1), (1, 2, 3)), (2, 1, 2)),        # (-1, 1, 1)
    (((3, 3, 1), (1, 1, 3)), (2, 2, 2)),        # (-1, -1, 1)
    (((0, 3, 1), (2, 1, 3)), (1, 2, 2)),        # (1, -1, 1)
])
def test_rank_cells_edge_line_quirk(ends, cell):
    T = np.zeros((4, 4, 5), dtype=bool)
    T[ends[0]] = T[ends[1]] = True
    assert npk.ranks(T, quirk=False)[cell] == 1 and npk.ranks(T).max() == 0
    assert np.array_equal(pockets.rank_cells(T), npk.ranks(T))
    # one cell further from the edge the line is scanned
    T = np.zeros((4, 4, 5), dtype=bool)
    step = np.sign(np.subtract(ends[1], ends[0]))
    a, b = np.array(ends[0]), np.array(ends[1])
    a[2] -= 1
    b[2] -= 1                                   # the line from z = 0
    T[tuple(a)] = T[tuple(b)] = True
    want = npk.ranks(T)
    assert want[tuple(a + step)] == 1 and want.sum() == 1
    assert np.array_equal(pockets.rank_cells(T), want)


@pytest.mark.parametrize("shape", [(70, 3, 5), (3, 70, 4), (4, 5, 70), (66, 67, 68), (1, 1, 40),
                                   (1, 9, 9), (17, 1, 33)])
def test_rank_cells_random(shape):
    rng = np.random.RandomState(sum(shape))
    T = rng.rand(*shape) < 0.15
    want = npk.ranks(T)
    assert want.max() >= (7 if min(shape) > 60 else 1)
    if min(shape) > 60:
        assert not np.array_equal(want, npk.ranks(T, quirk=False))
    assert np.array_equal(pockets.rank_cells(T), want)


# ---- the labelling kernels alone --------------------------------------------------------------
def _serpentine(nx, ny, nz):
    """one chain through the grid: full rows y = 0, 2, .. joined at alternating ends, in the
    layers z = 0, 2, .. joined at alternating corners"""
    m = np.zeros((nx, ny, nz), dtype=bool)
    for z in range(0, nz, 2):
        m[:, 0:ny:2, z] = True
        for k, y in enumerate(range(1, ny, 2)):
            m[-1 if k % 2 == 0 else 0, y, z] = True
    for k, z in enumerate(range(1, nz, 2)):
        m[0, -1 if k % 2 == 0 else 0, z] = True
    return m


def _combs(nx, ny, nz):
    m = np.zeros((nx, ny, nz), dtype=bool)
    m[:, 0, :] = True
    m[0::4, 0:ny - 2, :] = True         # teeth up
    m[:, ny - 1, :] = True
    m[2::4, 2:ny, :] = True             # teeth down
    return m


def test_label_cells_crafted():
    x, y, z = np.ogrid[:9, :8, :7]
    masks = {
        "serpentine": (_serpentine(21, 21, 5), 1),
        "checkerboard": ((x + y + z) % 2 == 0, 1),
        "corners": ((x == y) & (y == z), 7),
        "full": (np.ones((9, 8, 7), dtype=bool), 1),
        "empty": (np.zeros((9, 8, 7), dtype=bool), 0),
        "combs": (_combs(23, 12, 2), 2),
        "one cell": (np.ones((1, 1, 1), dtype=bool), 1),
    }
    for name, (m, parts) in masks.items():
        want = npk.labels(m)
        assert len(np.unique(want[m])) == parts, name
        got = pockets.label_cells(m)
        assert got.dtype == np.int32 and got.shape == m.shape
        assert np.array_equal(got, want), name
    # the chain is a chain: far longer than it is wide
    assert _serpentine(21, 21, 5).sum() > 700


@pytest.mark.parametrize("shape, density", [((40, 41, 42), 0.1), ((40, 41, 42), 0.2),
                                            ((300, 5, 3), 0.35), ((2, 2, 1000), 0.5)])
def test_label_cells_random(shape, density):
    m = np.random.RandomState(shape[0]).rand(*shape) < density
    want = npk.labels(m)
    sizes = np.bincount(want[m])
    assert (sizes > 0).sum() > 5 and sizes.max() > 20
    assert np.array_equal(pockets.label_cells(m), want)


def test_the_same_call_twice_gives_the_same_bytes():
    """the merges of the labelling happen in whatever order the hardware takes them"""
    xyz, radii = FIXTURES["shell1"]
    a = pockets.get_pockets(xyz[None], radii, 0.1, 0.07, 2)
    b = pockets.get_pockets(xyz[None], radii, 0.1, 0.07, 2)
    assert len(a[0].cells) > 500 and a[0].pocket_ids.max() >= 1
    assert a[0].cells.tobytes() == b[0].cells.tobytes()
    assert a[0].pocket_ids.tobytes() == b[0].pocket_ids.tobytes()
    check_frame(a[0], expected("shell1", 0.1, 0.07, 2), 0.1)
    m = np.random.RandomState(9).rand(50, 50, 50) < 0.18
    assert pockets.label_cells(m).tobytes() == pockets.label_cells(m).tobytes()
