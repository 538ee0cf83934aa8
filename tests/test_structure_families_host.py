"""The structure families of tests/_structure_cases.py on the CPU.

1. The oracle (oracle/qcp_oracle.c) against a float64 Kabsch superposition:
   |d^2 - msd| <= TOL (Gx + Gy) / A for every frame against the centers
   {0, n // 2, n - 1}, n = 300, and a frame's distance to itself at most
   1e-3 sqrt((Gx + Gy) / A).  Worst |d^2 - msd| A / (Gx + Gy) per family, over
   its atom counts (2, 3, 4, 7, 33; cube 8, two_atom_quantised 2), measured with
   the step rule of DESIGN.md section 2 item 4 in place:

       generic            1.9e-6      cube                1.1e-7
       collinear_exact    4.4e-5      two_atom_quantised  2.9e-7
       collinear_rotated  1.1e-5      scale_tiny          3.3e-7
       near_collinear     1.1e-6      scale_small         4.7e-7
       planar             9.0e-7      scale_large         9.8e-6
       mirror             2.2e-6      scale_huge          1.4e-6
       rotated_copies     1.8e-6      far_offset          2.1e-5
       identical          1.6e-15

   (Every family's worst is at A = 2 -- the float32 roundings of S and of the
   traces against a two-atom extent -- except collinear_exact, A = 7, below;
   from A = 3 on all others stay under 2.6e-7 but collinear_rotated, 1.1e-5.)
   Before the step rule collinear_exact and two_atom_quantised stood at 2.0: a
   frame's distance to itself came out as twice its extent.

   TOL is 1e-4, the cap, not four times the worst figure (1.75e-4), and the
   reason is a finding of its own.  Two DIFFERENT frames on the same axis give
   an exactly rank-one S whose quartic is (l^2 - s1^2)^2 again, approached from
   (Gx + Gy) / 2 > s1: the iterates halve their distance to the double root for
   ~28 steps and then wander in rounding noise at 1e-8 s1; a noise step can
   throw the iterate anywhere, and one that lands INSIDE [sqrt(q / 3),
   (Gx + Gy) / 2] is taken like any other.  4.4e-5 is such a jump on the
   fiftieth and last step (frame 49 against frame 0, A = 7: the root left at
   0.382585 for 0.382622).  The step rule cannot see it, and a rule that could
   (refusing every rising step) would change results the old iteration left
   inside the interval, which this contract change does not do.  The bound is
   kept where a wider one would hide a regression everywhere else.

2. The device header enspara_amd/csrc/ek_qcp.h, compiled with g++ as
   tests/test_qcp_host.py does, on the S, Gx, Gy of the same pairs:
   ek_rmsd_from_S gives the oracle's bits; ek_rmsd_from_S_below those bits or
   +inf, +inf only where the oracle's distance is >= cur; ek_far_certified_f32
   never says "far" of a pair whose oracle distance is < cur.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import qcp
from _structure_cases import SCALES, family_cases, kabsch_msd, structure_family
from test_qcp_host import host      # noqa: F401  (the g++ build of ek_qcp.h)

N = 300
CENTERS = (0, N // 2, N - 1)
TOL = 1e-4
CASES = family_cases()


@functools.lru_cache(maxsize=None)
def _case(family, A):
    """-> frames, Prepared, and per center the oracle's distances (never written
    to afterwards)"""
    x = structure_family(family, N, A)
    assert x.dtype == np.float32 and x.shape == (N, A, 3) and np.isfinite(x).all()
    P = qcp.Prepared(x)
    return x, P, {c: P.rmsd_to_frame(c) for c in CENTERS}


@pytest.mark.parametrize("family,A", CASES)
def test_oracle_against_float64_kabsch(family, A):
    x, P, dist = _case(family, A)
    worst = 0.0
    for c in CENTERS:
        d = dist[c].astype(np.float64)
        msd, scale = kabsch_msd(x, x[c])
        assert np.all(scale > 0)
        ratio = np.abs(d * d - msd) / scale
        worst = max(worst, float(ratio.max()))
        print("%s A=%d center %d: worst |d^2 - msd| A / (Gx + Gy) = %.3g (frame %d), "
              "self-distance %.3g sqrt((Gx + Gy) / A)"
              % (family, A, c, ratio.max(), ratio.argmax(), d[c] / np.sqrt(scale[c])))
        assert np.all(ratio <= TOL), (c, int(ratio.argmax()), float(ratio.max()))
        assert d[c] <= 1e-3 * np.sqrt(scale[c]), (c, d[c], scale[c])


@pytest.mark.parametrize("family,A", CASES)
def test_every_frame_is_at_distance_zero_of_itself(family, A):
    """all N frames, not only the three centers (S and the traces of a frame with
    itself through the same oracle calls the one-vs-all pass makes)"""
    x, P, _ = _case(family, A)
    bad = []
    for i in range(N):
        S = qcp.S_matrices(P.c[i:i + 1], P.c[i])[0]
        d = np.sqrt(qcp.msd_from_S(S, P.G[i], P.G[i], A))
        if not d <= 1e-3 * np.sqrt(2.0 * P.G[i] / A):
            bad.append((i, d))
    assert not bad, (len(bad), bad[:5])


def _pairs(family, A):
    """S [3 N, 9], Gx, Gy [3 N], oracle distances [3 N] of every frame against
    the three centers"""
    x, P, dist = _case(family, A)
    S = np.concatenate([qcp.S_matrices(P.c, P.c[c]) for c in CENTERS])
    Gx = np.ascontiguousarray(np.tile(P.G, len(CENTERS)))
    Gy = np.ascontiguousarray(np.repeat(P.G[list(CENTERS)], N))
    want = np.concatenate([dist[c] for c in CENTERS])
    return np.ascontiguousarray(S), Gx, Gy, want


@pytest.mark.parametrize("family,A", CASES)
def test_host_compiled_header_against_the_oracle(host, family, A):   # noqa: F811
    S, Gx, Gy, want = _pairs(family, A)
    m = len(want)
    Gsum = np.ascontiguousarray(Gx + Gy)
    for factor in (0.2, 0.7, 0.999, 1.0, 1.001, 1.5, np.inf):
        with np.errstate(invalid="ignore"):      # 0 * inf: a NaN bound, never stops
            cur = (want * np.float32(factor)).astype(np.float32)
        full = np.empty(m, dtype=np.float32)
        below = np.empty(m, dtype=np.float32)
        host.h_batch(S.ctypes.data_as(C.c_void_p), Gx.ctypes.data_as(C.c_void_p),
                     Gy.ctypes.data_as(C.c_void_p), A,
                     cur.ctypes.data_as(C.c_void_p), C.c_int64(m),
                     full.ctypes.data_as(C.c_void_p),
                     below.ctypes.data_as(C.c_void_p))
        np.testing.assert_array_equal(full.view(np.uint32), want.view(np.uint32))
        gave_up = np.isinf(below) & ~np.isinf(want)
        np.testing.assert_array_equal(below[~gave_up].view(np.uint32),
                                      want[~gave_up].view(np.uint32))
        with np.errstate(invalid="ignore"):
            assert np.all(want[gave_up] >= cur[gave_up])     # never a winner
        if not np.isfinite(factor):
            assert not gave_up.any()
            continue
        cert = np.empty(m, dtype=np.uint8)
        host.h_cert(S.ctypes.data_as(C.c_void_p), Gsum.ctypes.data_as(C.c_void_p), A,
                    cur.ctypes.data_as(C.c_void_p), C.c_int64(m),
                    cert.ctypes.data_as(C.c_void_p))
        far = (cert & 1).astype(bool)
        assert not np.any(want[far] < cur[far])
        if family in SCALES:
            assert not far.any()        # q outside [1e-12, 1e12]: nothing certified
