"""geometry.sasa.shrake_rupley on the device (csrc/ek_sasa.hip).

No expected value comes from a device call.  Counts are array_equal to the brute-force
numpy restatement (tests/_numpy_sasa.py: all j != i, no culling), areas and group sums
bit-equal to it -- the arithmetic is a contract.  The beta-peptide frames'
counts were recorded from the same restatement (tests/golden/make_exposons_golden.py;
tests/test_exposons_host.py repeats two of them).

Data: uniform random blobs at protein density (170 atoms in a 1.3 nm cube), radii of
H / C / N / O, a different blob per frame; at probe 0.14 and 96 points about a third of
the atoms are buried and the rest keep up to half of their points, so both branches of
the point loop are at work.  Atom counts sit either side of a wave and of a 256-lane
workgroup.  Point counts: 1, 24, 96, 100 and 960 on 170 atoms (fewer points than lanes, and
3.75 a lane), and on 65 atoms 255, 256 and 257 -- either side of one point per lane -- and
MAX_POINTS - 1 and MAX_POINTS, where a lane's sixteenth point takes the last bit of its
mask; one point more is refused.  2047, 2048 and 2049 atoms sit either side of one batch of
the neighbour scan (exactly full; a second batch of one atom), 2100 take two batches."""
import functools
import os

import numpy as np
import pytest

import _limit_cases as lc
import _numpy_sasa as ns
from enspara_amd.exception import DataInvalid
from enspara_amd.geometry import sasa

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "exposons_golden.npz"))
SC_IDS = [G["bp_sc_atoms"][a:b] for a, b in zip(G["bp_sc_offsets"][:-1],
                                                G["bp_sc_offsets"][1:])]


@functools.lru_cache(maxsize=None)
def _blob(frames, atoms, seed=0):
    xyz, radii = ns.blob(np.random.RandomState(1000 * seed + 7 * atoms + frames), frames, atoms)
    xyz.setflags(write=False)
    radii.setflags(write=False)
    return xyz, radii


@functools.lru_cache(maxsize=None)
def _expected(frames, atoms, probe, n, seed=0):
    xyz, radii = _blob(frames, atoms, seed)
    c = ns.counts(xyz, radii, probe, n)
    c.setflags(write=False)
    return c


def _check(xyz, radii, probe, n, want_counts, groups=None, **kw):
    area, counts = sasa.shrake_rupley(xyz, radii, probe_radius=probe, n_sphere_points=n,
                                      return_counts=True, **kw)
    assert counts.dtype == np.int32 and area.dtype == np.float32
    assert np.array_equal(counts, want_counts)
    want_area = ns.areas(want_counts, radii, probe, n)
    assert np.array_equal(area, want_area)
    if groups is not None:
        sums = sasa.shrake_rupley(xyz, radii, probe_radius=probe, n_sphere_points=n,
                                  atom_groups=groups, **kw)
        assert sums.dtype == np.float32
        assert np.array_equal(sums, ns.group_sums(want_area, groups))
    return counts


@pytest.mark.parametrize("atoms", [1, 2, 63, 64, 65, 170, 257])
def test_atom_counts(atoms):
    xyz, radii = _blob(2, atoms)
    c = _check(xyz, radii, 0.14, 96, _expected(2, atoms, 0.14, 96))
    if atoms == 1:
        assert np.all(c == 96)
    if atoms == 170:
        buried = (c == 0).mean()
        print("170 atoms: counts %d .. %d of 96, %.0f%% buried" % (c.min(), c.max(),
                                                                    100 * buried))
        assert 0.1 < buried < 0.7 and c.max() > 20


LANES = lc.define("ek_sasa.hip", "SASA_WG")
SCAN = lc.define("ek_sasa.hip", "SASA_SCAN")


@pytest.mark.parametrize("n", [1, 24, 96, 100, 960, LANES - 1, LANES, LANES + 1,
                               sasa.MAX_POINTS - 1, sasa.MAX_POINTS])
def test_sphere_point_counts(n):
    atoms = 170 if n in (1, 24, 96, 100, 960) else 65
    xyz, radii = _blob(1, atoms)
    c = _check(xyz, radii, 0.14, n, _expected(1, atoms, 0.14, n))
    if atoms == 65:
        # buried atoms and atoms that keep over a quarter of their points: both branches
        assert c.min() == 0 and c.max() > n // 4
    if n == sasa.MAX_POINTS:
        assert n == 16 * LANES == lc.define("ek_sasa.hip", "SASA_MAX_POINTS")


def test_one_sphere_point_too_many_is_refused():
    xyz, radii = _blob(1, 65)
    with pytest.raises(DataInvalid):
        sasa.shrake_rupley(xyz, radii, n_sphere_points=sasa.MAX_POINTS + 1)


@pytest.mark.parametrize("frames", [1, 3, 17])
def test_frames(frames):
    xyz, radii = _blob(frames, 170)
    _check(xyz, radii, 0.14, 96, _expected(frames, 170, 0.14, 96))


@pytest.mark.parametrize("chunk", [1, 5, 8, 16, 17])
def test_host_chunks(chunk):
    """17 frames in uploads of `chunk`: 17, 4, 3, 2 and 1 launches, the last ragged"""
    xyz, radii = _blob(17, 170)
    groups = [np.arange(0, 170, 3), np.array([5])]
    _check(xyz, radii, 0.14, 96, _expected(17, 170, 0.14, 96), groups=groups,
           chunk_frames=chunk)


def test_two_batches_of_the_neighbour_scan():
    xyz, radii = _blob(1, 2100)
    c = _check(xyz, radii, 0.14, 24, _expected(1, 2100, 0.14, 24))
    assert c.min() == 0 and c.max() > 0


@pytest.mark.parametrize("atoms", [SCAN - 1, SCAN, SCAN + 1])
def test_atoms_around_one_batch_of_the_neighbour_scan(atoms):
    """SCAN atoms fill the batch exactly; with SCAN + 1 the second batch holds one atom"""
    xyz, radii = _blob(1, atoms)
    want = _expected(1, atoms, 0.14, 8)
    if atoms == SCAN + 1:
        # the lone atom of the second batch is blocked by atoms of the first, and blocks some
        assert want[0, SCAN] < 8
        alone = ns.counts(xyz[:, :SCAN], radii[:SCAN], 0.14, 8)
        assert not np.array_equal(alone, want[:, :SCAN])
    c = _check(xyz, radii, 0.14, 8, want)
    assert c.min() == 0 and c.max() > 0


def test_probe_028():
    xyz, radii = _blob(2, 170)
    _check(xyz, radii, 0.28, 96, _expected(2, 170, 0.28, 96))


def test_duplicated_atom():
    """r_ij = 0 with equal radii: a point of one lies on the other's sphere up to the
    rounding of p, so which points are blocked is decided in the last bit; with a smaller
    twin inside, the smaller is buried whole"""
    xyz, radii = _blob(1, 65)
    xyz, radii = xyz.copy(), radii.copy()
    xyz[0, 64] = xyz[0, 10]
    radii[64] = radii[10]
    want = ns.counts(xyz, radii, 0.14, 96)
    _check(xyz, radii, 0.14, 96, want)
    lone = np.zeros((1, 2, 3), dtype=np.float32)
    c = _check(lone, np.array([0.17, 0.12], np.float32), 0.14, 96,
               ns.counts(lone, [0.17, 0.12], 0.14, 96))
    assert c[0, 0] == 96 and c[0, 1] == 0


def test_atoms_exactly_touching():
    """|x_i - x_j| = R_i + R_j in float32: inside the culling margin, and the restatement
    decides every point"""
    R = np.float32(0.17) + np.float32(0.14)
    xyz = np.zeros((3, 2, 3), dtype=np.float32)
    xyz[0, 1, 0] = R + R
    xyz[1, 1, 1] = R + R
    xyz[2, 1, 2] = np.nextafter(R + R, np.float32(0))
    radii = np.array([0.17, 0.17], np.float32)
    for n in (96, 960):
        _check(xyz, radii, 0.14, n, ns.counts(xyz, radii, 0.14, n))


def test_atom_without_a_neighbour():
    xyz, radii = _blob(1, 64)
    xyz = xyz.copy()
    xyz[0, 63] = [9.0, -7.0, 30.0]
    want = ns.counts(xyz, radii, 0.14, 100)
    c = _check(xyz, radii, 0.14, 100, want)
    assert c[0, 63] == 100


@pytest.mark.parametrize("shift", [40.0, -126.0])
def test_translated_blob(shift):
    """coordinates of 40 nm and near the limit of 128 nm: p rounds to 2^-18 and 2^-17 nm
    there, which the culling margin has to cover"""
    xyz, radii = _blob(1, 170)
    xyz = (xyz + np.float32(shift)).astype(np.float32)
    assert np.abs(xyz).max() <= sasa.MAX_COORD
    want = ns.counts(xyz, radii, 0.14, 96)
    c = _check(xyz, radii, 0.14, 96, want)
    assert (c == 0).any() and (c > 0).any()


def test_groups():
    xyz, radii = _blob(3, 170)
    rng = np.random.RandomState(5)
    groups = [np.array([169]), rng.permutation(170)[:7], np.arange(8), np.arange(9)[::-1],
              rng.permutation(170)[:33], np.array([4, 4, 4, 2]), np.arange(170)]
    _check(xyz, radii, 0.14, 96, _expected(3, 170, 0.14, 96), groups=groups)


def test_beta_peptide():
    """the reference's fixture at the exposons' settings: 960 points, probe 0.28 nm,
    sidechain groups"""
    xyz = G["bp_xyz"]
    radii = sasa.radii_from_elements(G["bp_elements"])
    want = G["bp_counts"].astype(np.int32)
    c = _check(xyz, radii, 0.28, 960, want, groups=SC_IDS)
    assert c.max() > 300 and (c == 0).any()
