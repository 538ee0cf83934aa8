"""enspara_amd.geometry.rotamer on the device (csrc/ek_rotamer.hip): buffered rotamer
states from angles, dihedral angles from coordinates, and both in one pass.

No expected value comes from a device call.  States are array_equal to the numpy
restatement (tests/_numpy_cards.py: the state machine walked frame by frame) and to the
reference's `_rotamers` outputs in tests/golden/cards_golden.npz.  Frames as in
tests/test_gpu_cards.py (cards.SCAN_CHUNK is a multiple of the state scan's own chunk,
rotamer.SCAN_CHUNK, so its neighbours are chunk boundaries here too) and around one chunk;
dihedrals 1, 3, 64, 65, 300: one lane, fewer than a wave, a wave and one more, more than
a workgroup.  Column j is of kind j % 3 (phi, psi shifted by 100, chi), so the kinds are
mixed within every call; every fifth column draws its angles from the values that sit
exactly on a gate or boundary, the others walk at steps of 5, 25 or 90 degrees.

Dihedral angles are held to a float64 numpy evaluation of the same formula, within four
times the largest error of a *float32 numpy* evaluation on the same inputs (the device's
atan2f need not be correctly rounded).  Measured on the MI355X: the float32 numpy error is
2.98e-5 degrees on these inputs and the device's largest error 2.98e-5, 0.25 of the allowance.
From coordinates to states, the generator keeps every angle 0.01 degrees (over 300 times
the float32 error) from every gate, boundary and the 359.5 clip, so the states equal the
restatement's on the float64 angles with no case left out."""
import functools
import os

import numpy as np
import pytest

import _numpy_cards as nc
from enspara_amd import cards
from enspara_amd.geometry import rotamer

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                         "cards_golden.npz"))
CH = cards.SCAN_CHUNK
RC = rotamer.SCAN_CHUNK
FRAMES = [1, 2, 63, 64, 65, RC - 1, RC, RC + 1, CH - 1, CH, CH + 1, 2 * CH + 1, 3 * CH + 5]
DIHEDRALS = [1, 3, 64, 65, 300]
WIDTHS = (0, 15, 15.5, 60)
BOUNDS = [nc.PHI, nc.PSI, nc.CHI]
SHIFTS = [0, 100, 0]


@functools.lru_cache(maxsize=None)
def _angles():
    """float32 [3 CH + 5, 300] and the kinds of the columns"""
    rng = np.random.RandomState(51)
    T, n = FRAMES[-1], DIHEDRALS[-1]
    kind = np.arange(n) % 3
    A = np.zeros((T, n), dtype=np.float32)
    for j in range(n):
        if j % 5 == 4:      # on the gates (for psi: the raw angles whose shifted values are)
            v = np.array(nc.ON_GATES)[rng.randint(0, len(nc.ON_GATES), T)]
            A[:, j] = np.mod(v + SHIFTS[kind[j]], 360)
        else:
            step = (5.0, 25.0, 90.0)[j % 4 % 3]
            A[:, j] = np.mod(np.cumsum(rng.normal(0, step, T)) + rng.uniform(0, 360), 360)
    A[A >= 360] = 0
    assert A.min() >= 0 and A.max() < 360
    # no shifted angle rounds to 360 (the documented difference from the reference)
    assert all(nc.shifted(A[:, j], SHIFTS[kind[j]]).max() < 360 for j in range(n))
    A.setflags(write=False)
    return A, kind


@functools.lru_cache(maxsize=None)
def _want(width, frames):
    A, kind = _angles()
    S = nc.rotamer_states(A[:frames], kind, BOUNDS, SHIFTS, width)
    S.setflags(write=False)
    return S


# ---- states from angles ----------------------------------------------------------------------
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("n", DIHEDRALS)
def test_states_equal_the_restatement(n, frames):
    A, kind = _angles()
    got = rotamer.rotamer_states(A[:frames, :n], kind[:n], BOUNDS, SHIFTS, 15)
    assert got.dtype == np.uint8 and got.shape == (frames, n)
    # (the machine is causal and the columns are independent: a prefix of the full answer)
    assert np.array_equal(got, _want(15, FRAMES[-1])[:frames, :n])


@pytest.mark.parametrize("width", [0, 15.5, 60])
def test_other_buffer_widths(width):
    A, kind = _angles()
    got = rotamer.rotamer_states(A[:CH + 65], kind, BOUNDS, SHIFTS, width)
    want = _want(width, CH + 65)
    assert np.array_equal(got, want)
    assert len(np.unique(want[:, 2])) == 3 and len(np.unique(want[:, 0])) == 2


def test_chunk_lengths():
    assert RC == 256 and CH % RC == 0


def test_states_against_the_reference():
    for key, res in (("rot_angles", "rot_states"), ("rot_gates", "rot_gate_states")):
        A = G[key]
        for w, width in enumerate(WIDTHS):
            # all three kinds in one call
            got = rotamer.rotamer_states(A, [0, 1, 2], BOUNDS, SHIFTS, width)
            assert np.array_equal(got.T, G[res][:, w]), (key, width)
            # one kind a call, through the reference's signature
            for k in range(3):
                one = rotamer.rotamers(A[:, k], BOUNDS[k], width, shift=SHIFTS[k])
                assert one.dtype == np.int16 and one.shape == (len(A),)
                assert np.array_equal(one, G[res][k, w]), (key, width, k)
    two_d = rotamer._rotamers(G["rot_angles"][:, [0, 0]], nc.PHI)
    assert two_d.shape == (1500, 2) and np.array_equal(two_d[:, 1], G["rot_states"][0, 1])
    assert rotamer.rotamers(np.zeros(0, dtype=np.float32), nc.PHI).shape == (0,)


def test_more_basins_and_a_shifted_angle_of_360():
    rng = np.random.RandomState(52)
    hb8 = [0, 45, 90, 135, 180, 225, 270, 315, 360]
    A = rng.uniform(0, 360, (CH + 3, 5)).astype(np.float32)
    A[A >= 360] = 0
    got = rotamer.rotamer_states(A, [0, 1, 0, 1, 0], [hb8, [0, 10, 360]], [0, 0], 4)
    assert np.array_equal(got, nc.rotamer_states(A, [0, 1, 0, 1, 0], [hb8, [0, 10, 360]],
                                                 [0, 0], 4))
    assert got[:, 0].max() == 7
    # 99.999996 - 100 + 360 rounds to 360.0 in float32: the last basin, on frame 0 and later
    a = np.array([np.nextafter(np.float32(100), np.float32(0)), 250, 99.999996, 300],
                 dtype=np.float32)
    assert list(nc.shifted(a, 100)) == [360, 150, 360, 200]
    got = rotamer.rotamers(a, nc.CHI, 15, shift=100)
    assert list(got) == [2, 1, 2, 1]
    assert np.array_equal(got, nc.rotamer_states(a[:, None], [0], [nc.CHI], [100], 15)[:, 0])


# ---- dihedral angles ---------------------------------------------------------------------------
def test_dihedral_angles_within_four_float32_errors():
    """Largest device error / allowance, measured on the MI355X: 0.25 (the float32 numpy
    error on these inputs: 2.98e-5 degrees, the device's the same)."""
    rng = np.random.RandomState(53)
    target = rng.uniform(0.5, 359.0, (70, 333))
    quads = np.arange(4 * 333).reshape(333, 4)
    xyz = nc.place_dihedrals(rng, target.ravel()).reshape(70, 4 * 333, 3)
    # the same atoms in another order: the indices are read, not assumed
    perm = rng.permutation(4 * 333)
    xyz, quads = xyz[:, perm], np.argsort(perm)[quads]
    want = nc.dihedral_deg(xyz, quads)
    assert np.abs(want - target).max() < 1e-2 and want.min() > 0.4 and want.max() < 359.1
    allow = 4 * np.abs(nc.dihedral_deg(xyz, quads, np.float32).astype(np.float64) - want).max()
    got = rotamer.dihedral_angles(xyz, quads)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want).max()
    print("float32 numpy error %.3g degrees, allowance %.3g, device error %.3g = %.2f of it"
          % (allow / 4, allow, err, err / allow))
    assert 1e-5 < allow < 4e-4
    assert err <= allow


def test_angle_transforms():
    # flat dihedrals: 180 stays, -0 and tiny negative angles wrap and clip to 359.5
    xyz = np.zeros((3, 4, 3), dtype=np.float32)
    xyz[:, 0] = (0, 1, 0)
    xyz[:, 2] = (1, 0, 0)
    xyz[0, 3] = (1, -1, 0)                  # trans: 180
    xyz[1, 3] = (1, 1, -1e-4)               # just below 0: 360 - 0.0057 -> 359.5
    xyz[2, 3] = (1, 0, 1)                   # 90
    got = rotamer.dihedral_angles(xyz, [[0, 1, 2, 3]])[:, 0]
    want = nc.dihedral_deg(xyz, [[0, 1, 2, 3]])[:, 0]
    assert got[1] == np.float32(359.5) and want[1] == 359.5
    assert np.abs(got - want).max() < 1e-4 and abs(want[0] - 180) < 1e-9


# ---- coordinates to states -----------------------------------------------------------------------
@pytest.mark.parametrize("frames,n", [(1, 1), (65, 3), (CH + 1, 64), (2 * CH + 1, 65),
                                      (64, 300)])
def test_states_from_coordinates(frames, n):
    rng = np.random.RandomState(54 + n)
    kind = np.arange(n) % 3
    xyz, quads, deg = nc.safe_trajectory(rng, frames, kind, BOUNDS, SHIFTS, 15)
    want = nc.rotamer_states(deg, kind, BOUNDS, SHIFTS, 15)       # on the float64 angles
    fused, ang = rotamer.dihedral_rotamers(xyz, quads, kind, BOUNDS, SHIFTS, 15,
                                           return_angles=True)
    assert np.array_equal(fused, want)
    # the two-step path: the same angles, the same states, bit for bit
    angles = rotamer.dihedral_angles(xyz, quads)
    assert np.array_equal(ang, angles)
    assert np.abs(angles.astype(np.float64) - deg).max() < 2e-4
    assert np.array_equal(rotamer.rotamer_states(angles, kind, BOUNDS, SHIFTS, 15), fused)
    assert np.array_equal(rotamer.dihedral_rotamers(xyz, quads, kind, BOUNDS, SHIFTS, 15),
                          fused)


def test_phi_psi_chi_and_all_rotamers():
    rng = np.random.RandomState(60)
    kind = np.array([0, 0, 1, 1, 1, 2, 2])
    xyz, quads, deg = nc.safe_trajectory(rng, 500, kind, BOUNDS, SHIFTS, 10)
    want = nc.rotamer_states(deg, kind, BOUNDS, SHIFTS, 10)
    d = {"phi": quads[:2], "psi": quads[2:5], "chi": quads[5:]}
    states, inds, n_states = rotamer.all_rotamers(xyz, d, buffer_width=10)
    assert states.dtype == np.int16 and np.array_equal(states, want)
    assert np.array_equal(inds, quads) and list(n_states) == [2, 2, 2, 2, 2, 3, 3]
    for f, sl in ((rotamer.phi_rotamers, slice(0, 2)), (rotamer.psi_rotamers, slice(2, 5)),
                  (rotamer.chi_rotamers, slice(5, 7))):
        s, q, n = f(xyz, quads[sl], buffer_width=10)
        assert np.array_equal(s, want[:, sl]) and np.array_equal(q, quads[sl])
        assert np.array_equal(n, n_states[sl]) and n.dtype == np.int16
    only_chi = rotamer.all_rotamers(xyz, {"chi": quads[5:]}, buffer_width=10)
    assert np.array_equal(only_chi[0], want[:, 5:])
