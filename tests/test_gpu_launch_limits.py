"""The device paths an input enters only when it outgrows one launch: a capped grid.y and
the stride over it, a second batch of launches with a chunk offset, a chunk that starts to
grow, a second chunk of the host loop.  Each is run once, at the smallest input that
reaches it, every size computed from the kernel file's own constants (tests/
_limit_cases.py).

    rotamer.dihedral_angles        grid.y = min(frames, RT_MAX_GRID_Y), t += gridDim.y
    rotamer.rotamer_states,        map and emit kernels in batches of RT_MAX_GRID_Y chunks,
      dihedral_rotamers              the later batches with chunk0 > 0
    entropy.state_counts           grid.y = min(chunks, ENT_SC_MAX_GRID_Y), ch += gridDim.y
    weighted_joint_probabilities,  past WMI_CHUNK * WMI_MAX_CHUNKS frames the chunk grows
      weighted_mi
    sasa.shrake_rupley             the chunk clamped to SASA_MAX_FRAMES, a second launch
    pockets.get_pockets            the chunk builder stops at POCK_MAX_FRAMES, a second chunk

No expected value comes from a device call: the references are the numpy restatements the
modules' own tests use (tests/_numpy_cards.py, _numpy_wmi.py, _numpy_sasa.py,
_numpy_pockets.py, np.bincount).  Every comparison is array_equal except the three whose
bounds the project already derives: dihedral angles within four float32-numpy errors
(tests/test_gpu_rotamer.py), weighted sums and informations within _numpy_wmi.p_bound and
mi_bound; those tests print the ratio they see.  Each test asserts, on the reference's
values, the condition that makes it a check: that the frames behind the limit differ from
the frames a wrong offset or a dropped trip would read instead."""
import functools

import numpy as np
import pytest

import _limit_cases as lc
import _numpy_cards as nc
import _numpy_pockets as npk
import _numpy_sasa as ns
import _numpy_wmi as nw
from enspara_amd import info_theory
from enspara_amd.exception import DataInvalid
from enspara_amd.geometry import pockets, rotamer, sasa
from enspara_amd.info_theory import entropy, mutual_info
from test_gpu_pockets import _round_shell, check_frame
from test_gpu_sasa import _check as check_sasa

pytestmark = pytest.mark.gpu

RT_G = lc.define("ek_rotamer.hip", "RT_MAX_GRID_Y")
ROT_CHUNK = lc.define("ek_rotamer.hip", "ROT_CHUNK")
SC_CHUNK = lc.define("ek_entropy.hip", "ENT_SC_CHUNK")
SC_Y = lc.define("ek_entropy.hip", "ENT_SC_MAX_GRID_Y")
SC_REG = lc.define("ek_entropy.hip", "ENT_SC_REG")
WMI_C = lc.define("ek_wmi.hip", "WMI_CHUNK")
WMI_M = lc.define("ek_wmi.hip", "WMI_MAX_CHUNKS")
SASA_F = lc.define("ek_sasa.hip", "SASA_MAX_FRAMES")
POCK_F = lc.define("ek_pockets.hip", "POCK_MAX_FRAMES")


# ---- rotamer: dihedral angles past grid.y ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dihedral_case():
    """2 G + 1 frames of 3 dihedrals on 12 atoms in permuted order, every target drawn on
    its own -> (xyz, quads, float64 angles, the float32-numpy error)"""
    rng = np.random.RandomState(81)
    T = 2 * RT_G + 1
    target = rng.uniform(0.5, 359.0, (T, 3))
    quads = np.arange(12).reshape(3, 4)
    xyz = nc.place_dihedrals(rng, target.ravel()).reshape(T, 12, 3)
    perm = rng.permutation(12)
    xyz, quads = np.ascontiguousarray(xyz[:, perm]), np.argsort(perm)[quads]
    want = nc.dihedral_deg(xyz, quads)
    assert np.abs(want - target).max() < 1e-2 and want.min() > 0.4 and want.max() < 359.1
    err32 = np.abs(nc.dihedral_deg(xyz, quads, np.float32).astype(np.float64) - want)
    for a in (xyz, want, err32):
        a.setflags(write=False)
    return xyz, quads, want, err32


@pytest.mark.parametrize("frames", [RT_G, RT_G + 1, 2 * RT_G + 1])
def test_dihedral_angles_past_the_grid_cap(frames):
    """G frames fill grid.y, G + 1 send workgroup y = 0 on a second trip, 2 G + 1 on a
    third.  Measured on the MI355X: the float32 numpy error on these inputs is 3.05e-5
    degrees (3.14e-5 at 2 G + 1 frames), the device's largest error 3.05e-5, 0.25 (0.24) of
    the allowance."""
    xyz, quads, want, err32 = _dihedral_case()
    xyz, want = xyz[:frames], want[:frames]
    allow = 4 * err32[:frames].max()
    assert 1e-5 < allow < 4e-4
    # a frame is no repeat of the frame G before it: some dihedral of the two differs by more
    # than two allowances, so frame t - G written in place of frame t is out of the allowance
    if frames > RT_G:
        assert np.all(np.abs(want[RT_G:] - want[:frames - RT_G]).max(axis=1) > 2 * allow)
    got = rotamer.dihedral_angles(xyz, quads)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want).max()
    print("%d frames: float32 numpy error %.3g degrees, allowance %.3g, device error %.3g = "
          "%.2f of it" % (frames, allow / 4, allow, err, err / allow))
    assert err <= allow


# ---- rotamer: states of more than G chunks ------------------------------------------------------
P = 1000                                    # frames of the block that is tiled
ROT_FRAMES = (RT_G + 1) * ROT_CHUNK + 1     # G + 2 chunks: a second batch of 2, the last of 1 frame


def _check_tiling(want, block, kind):
    """the conditions that make a tiled block a check of the second batch"""
    assert (ROT_FRAMES + ROT_CHUNK - 1) // ROT_CHUNK == RT_G + 2
    # chunks G apart hold different frames of the block, and no chunk starts where one of
    # the block's copies does, except chunk 0
    assert (RT_G * ROT_CHUNK) % P != 0 and P % ROT_CHUNK != 0
    tail = want[RT_G * ROT_CHUNK:]
    assert len(tail) == ROT_CHUNK + 1
    assert all(len(np.unique(tail[:, j])) >= 2 for j in range(want.shape[1]))
    # (so the tail is not what the chunks G earlier -- chunks 0 and 1 -- hold)
    assert not np.array_equal(tail, want[:ROT_CHUNK + 1])
    # the one frame of the last chunk shows the state that chunk starts in -- what the carry
    # makes of chunk G's map, a map of the second batch: in some column its angle moves the
    # machine out of no basin, and the state it keeps is not 0
    last = block[(ROT_FRAMES - 1) % P]
    assert any(lc.keeps_every_start(last[j], kind[j], lc.BOUNDS, lc.SHIFTS, 15) and
               want[-1, j] == want[-2, j] != 0 for j in range(len(kind)))


def test_rotamer_states_past_the_grid_cap():
    """about 135 MB of angles on the host: 2 columns, psi walking at 25 degrees and chi at
    90 (a walk at 5 degrees crosses no gate in the 257 frames of the second batch)"""
    block, kind = lc.angle_block(98, P, 3)
    block, kind = block[:, 1:], kind[1:]
    assert list(kind) == [1, 2]
    want = lc.periodic_states(block, kind, lc.BOUNDS, lc.SHIFTS, 15, ROT_FRAMES)
    _check_tiling(want, block, kind)
    got = rotamer.rotamer_states(lc.tiled(block, ROT_FRAMES), kind, lc.BOUNDS, lc.SHIFTS, 15)
    assert got.dtype == np.uint8 and got.shape == (ROT_FRAMES, 2)
    assert np.array_equal(got, want)


def test_dihedral_rotamers_past_the_grid_cap():
    """the same through the fused entry (the kernels' XYZ = true instantiation), 2 columns:
    nc.safe_trajectory makes a block of 1000 frames in milliseconds, whose coordinates are
    tiled as the angles are above (1.6 GB of coordinates on the host)"""
    rng = np.random.RandomState(84)
    kind = np.array([0, 1])
    xyz, quads, deg = nc.safe_trajectory(rng, P, kind, lc.BOUNDS, lc.SHIFTS, 15)
    want = lc.periodic_states(deg, kind, lc.BOUNDS, lc.SHIFTS, 15, ROT_FRAMES)
    _check_tiling(want, deg, kind)
    got = rotamer.dihedral_rotamers(lc.tiled(xyz, ROT_FRAMES), quads, kind, lc.BOUNDS,
                                    lc.SHIFTS, 15)
    assert got.dtype == np.uint8 and got.shape == (ROT_FRAMES, 2)
    assert np.array_equal(got, want)


# ---- entropy: state counts past grid.y ----------------------------------------------------------
SC_FRAMES = (SC_Y + 1) * SC_CHUNK + 5       # Y + 2 chunks: y = 0 a second trip, y = 1 a ragged one


@functools.lru_cache(maxsize=2)
def _sc_codes(n):
    """uint8 [SC_FRAMES, 2] (about 67 MB): states 0 .. n - 2 up to frame Y * ENT_SC_CHUNK,
    all n states from there on; the 5 frames of the ragged chunk are in state n - 1"""
    rng = np.random.RandomState(84 + n)
    X = rng.randint(0, n - 1, size=(SC_FRAMES, 2), dtype=np.uint8)
    second = SC_Y * SC_CHUNK
    X[second:] = rng.randint(0, n, size=(SC_FRAMES - second, 2), dtype=np.uint8)
    X[-5:] = n - 1
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("n", [SC_REG - 1, SC_REG + 1])
def test_state_counts_past_the_grid_cap(n):
    """3 states: the register kernel; 5: the LDS kernel"""
    X = _sc_codes(n)
    second = SC_Y * SC_CHUNK
    assert (SC_FRAMES + SC_CHUNK - 1) // SC_CHUNK == SC_Y + 2
    want = np.stack([np.bincount(X[:, j], minlength=n) for j in range(2)]).astype(np.uint64)
    # the highest state occurs on the second trips only, and there in the whole chunk as well
    # as in the ragged one: without them its count is 0, or 5, and no count is the same
    head = np.stack([np.bincount(X[:second, j], minlength=n) for j in range(2)])
    assert np.all(head[:, n - 1] == 0) and np.all(want[:, n - 1] > 5)
    assert np.all(want != head.astype(np.uint64))
    got = entropy.state_counts(X, n)
    assert got.shape == (2, n) and got.dtype == np.int64 and got.min() >= 0
    assert np.array_equal(got.astype(np.uint64), want)
    # the same frames as two trajectories, split at an odd frame inside the second trip
    cut = second + SC_CHUNK // 2 + 1
    assert cut % 2 == 1 and second < cut < SC_FRAMES - 5
    got = entropy.state_counts([X[:cut], X[cut:]], n)
    assert np.array_equal(got.astype(np.uint64), want)


# ---- weighted MI: chunks that have grown ----------------------------------------------------------
WMI_FULL = WMI_C * WMI_M                    # the last frame count with chunks of WMI_CHUNK
WMI_GROWN = WMI_C + WMI_C // 2              # a grown chunk; below 64 WMI_MAX_CHUNKS, see below
WMI_FRAMES = [
    WMI_FULL,                               # WMI_MAX_CHUNKS chunks of WMI_CHUNK
    WMI_FULL + 1,                           # the chunk grows by 64, fewer chunks, a short last
    WMI_M * (WMI_C + 64) + 197,             # two steps of 64; frames no multiple of 64
    (WMI_M - 1) * WMI_GROWN + 65,           # WMI_MAX_CHUNKS chunks of WMI_GROWN, a short last
]
WMI_SHAPES = [(5, 3), (1, 2)]


def test_weighted_mi_frame_counts_lie_in_their_regimes():
    assert lc.wmi_chunk(WMI_FRAMES[0]) == (WMI_C, WMI_M, WMI_C)
    for T in WMI_FRAMES[1:3]:
        chunk, chunks, last = lc.wmi_chunk(T)
        assert chunk > WMI_C and chunks < WMI_M and last < chunk
    assert lc.wmi_chunk(WMI_FRAMES[1])[0] != lc.wmi_chunk(WMI_FRAMES[2])[0]
    assert WMI_FRAMES[2] % 64 != 0
    chunk, chunks, last = lc.wmi_chunk(WMI_FRAMES[3])
    assert chunk == WMI_GROWN and chunks == WMI_M and last < chunk
    # dyadic weights below 2^10 * 2^-20: every partial sum is below 2^33 * 2^-20, exact
    assert max(WMI_FRAMES) * 2 ** 10 < 2 ** 33


@functools.lru_cache(maxsize=None)
def _wmi_data(F, S):
    """codes, dyadic weights, general weights of max(WMI_FRAMES) frames; tests take prefixes"""
    T = max(WMI_FRAMES)
    rng = np.random.RandomState(8500 + 100 * F + S)
    X = nw.codes(rng, T, F, S)
    dy = rng.randint(1, 1024, size=T) * 2.0 ** -20
    ge = rng.rand(T) * np.exp(3 * rng.randn(T))
    ge[rng.rand(T) < 0.05] = 0.0
    ge[0] = 0.7
    for a in (X, dy, ge):
        a.setflags(write=False)
    return X, dy, ge


@pytest.mark.parametrize("T", WMI_FRAMES)
@pytest.mark.parametrize("F,S", WMI_SHAPES)
def test_grown_chunks_sum_dyadic_weights_exactly(F, S, T):
    X, w, _ = _wmi_data(F, S)
    X, w = X[:T], w[:T]
    want = nw.joint_probabilities(X, w, S)
    # the frames of the last chunk change the expected sums: they hold weight of their own
    chunk, chunks, _ = lc.wmi_chunk(T)
    t0 = (chunks - 1) * chunk
    assert 0 < t0 < T
    last = nw.joint_probabilities(X[t0:], w[t0:], S)
    assert last[0, 0].sum() == w[t0:].sum() > 0
    P = info_theory.weighted_joint_probabilities(X, w, S)
    assert P.dtype == np.float64 and P.shape == (F, F, S, S)
    assert np.array_equal(P, want)


@pytest.mark.parametrize("T", WMI_FRAMES)
@pytest.mark.parametrize("F,S", WMI_SHAPES)
def test_grown_chunks_general_weights_within_the_bounds(F, S, T):
    """Largest error / bound measured on the MI355X over the eight cases: 7.1e-5 for P
    (5 x 3 at WMI_CHUNK * WMI_MAX_CHUNKS + 1 frames), 1.5e-5 for the information."""
    X, _, w = _wmi_data(F, S)
    X, w = X[:T], nw.normalise(w[:T])
    want = nw.joint_probabilities(X, w, S)
    P = info_theory.weighted_joint_probabilities(X, w, S)
    err, bound = np.abs(P - want), nw.p_bound(T, want)
    ratio_p = (err[bound > 0] / bound[bound > 0]).max()
    mi_want, L, A = nw.mutual_information(want)
    mi = mutual_info._weighted_run(X, w, S, False, True, 0)[1]
    mb = nw.mi_bound(T, S, L, A)
    ratio_mi = (np.abs(mi - mi_want) / mb).max()
    print("F %d S %d T %d: P error / bound %.3g, MI error / bound %.3g"
          % (F, S, T, ratio_p, ratio_mi))
    assert np.all(err <= bound)
    assert np.all(P[want == 0] == 0)
    assert np.all(np.abs(mi - mi_want) <= mb)
    pub = info_theory.weighted_mi(X, w, n_feature_states=np.full(F, S), normalize=False)
    assert np.all(np.abs(pub - np.clip(mi_want, 0, np.inf)) <= mb)


# ---- SASA: more frames than one launch ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sasa_case():
    """SASA_MAX_FRAMES + 1 frames of 3 atoms in a 0.45 nm cube, a different blob per frame"""
    xyz, radii = ns.blob(np.random.RandomState(86), SASA_F + 1, 3, side=0.45)
    c = ns.counts(xyz, radii, 0.14, 8)
    for a in (xyz, radii, c):
        a.setflags(write=False)
    return xyz, radii, c


@pytest.mark.parametrize("chunk", [None, SASA_F])
def test_sasa_more_frames_than_one_launch(chunk):
    """the second launch holds one frame, at the offset SASA_MAX_FRAMES of the host arrays"""
    xyz, radii, want = _sasa_case()
    assert set(np.unique(want)) == set(range(9))
    # the frame of the second launch is not frame 0 over again, nor left at zero
    assert not np.array_equal(want[SASA_F], want[0]) and want[SASA_F].max() > 0
    check_sasa(xyz, radii, 0.14, 8, want, groups=[[2, 0], [1]], chunk_frames=chunk)


def test_sasa_chunk_frames_beyond_one_launch_are_refused():
    xyz, radii, _ = _sasa_case()
    with pytest.raises(DataInvalid):
        sasa.shrake_rupley(xyz[:2], radii, n_sphere_points=8, chunk_frames=SASA_F + 1)


# ---- pockets: more frames than one chunk ----------------------------------------------------------
POCK_ARGS = (0.1, 0.07, 3)                  # spacing, probe, min_rank
POCK_SEEDS = (1, 2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def _pocket_case():
    """5 round shells of 14 atoms (a few hundred cells each) and their pockets by the
    restatement; the radii are the first shell's"""
    shells = [_round_shell(14, seed) for seed in POCK_SEEDS]
    radii = shells[0][1]
    five = np.stack([s[0] for s in shells])
    want = [npk.frame_pockets(x, radii, *POCK_ARGS) for x in five]
    return five, radii, want


@pytest.mark.parametrize("chunk", [None, POCK_F])
def test_pockets_more_frames_than_one_chunk(chunk):
    """POCK_MAX_FRAMES + 1 frames: the second chunk holds one frame, whose cells and lines
    start at offset 0 again"""
    five, radii, want = _pocket_case()
    frames = POCK_F + 1
    assert POCK_F % 5 != 0
    assert len(set(tuple(w["dims"]) for w in want)) >= 2
    assert all(100 < int(np.prod(w["dims"])) < 1000 for w in want)
    assert sum(len(w["cells"]) > 0 for w in want) >= 4
    assert len(want[POCK_F % 5]["cells"]) > 0       # the frame of the second chunk
    got = pockets.get_pockets(lc.tiled(five, frames), radii, *POCK_ARGS, chunk_frames=chunk)
    assert len(got) == frames
    for f, g in enumerate(got):
        check_frame(g, want[f % 5], POCK_ARGS[0])
    ends = list(range(10)) + list(range(frames - 10, frames))
    vol = pockets.pocket_volumes([got[f] for f in ends], POCK_ARGS[0])
    for f, v in zip(ends, vol):
        ids = want[f % 5]["ids"]
        assert np.array_equal(v, np.bincount(ids) * POCK_ARGS[0] ** 3 if len(ids)
                              else np.zeros(0))
