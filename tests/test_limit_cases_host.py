"""tests/_limit_cases.py on the host: the sizes tests/test_gpu_launch_limits.py computes
from the kernels' constants rest on these.

* The constants the Python modules mirror equal the `#define`s of the sources.
* `periodic_states` -- the expected rotamer states of 16.7 million frames, made from three
  periods -- equals the restatement walked frame by frame.
* `wmi_chunk` restates `wmi_chunk` of csrc/ek_wmi.hip: at WMI_CHUNK * WMI_MAX_CHUNKS frames
  the chunk is still WMI_CHUNK, one frame more and it has grown."""
import numpy as np
import pytest

import _limit_cases as lc
import _numpy_cards as nc
from enspara_amd import info_theory
from enspara_amd.geometry import pockets, rotamer, sasa


def test_python_mirrors_equal_the_source():
    assert sasa.MAX_CHUNK_FRAMES == lc.define("ek_sasa.hip", "SASA_MAX_FRAMES")
    assert sasa.MAX_POINTS == lc.define("ek_sasa.hip", "SASA_MAX_POINTS")
    assert pockets.MAX_CHUNK_FRAMES == lc.define("ek_pockets.hip", "POCK_MAX_FRAMES")
    assert rotamer.SCAN_CHUNK == lc.define("ek_rotamer.hip", "ROT_CHUNK")
    assert info_theory.WMI_CHUNK == lc.define("ek_wmi.hip", "WMI_CHUNK")
    assert info_theory.MI_CHUNK == lc.define("ek_mi_launch.h", "MI_CHUNK")


def test_define_reads_whole_names_only():
    # SASA_MAX_FRAMES is no prefix match of another name, and a name that is not there fails
    assert lc.define("ek_entropy.hip", "ENT_SC_CHUNK") % 64 == 0
    with pytest.raises(AssertionError, match="no integer #define"):
        lc.define("ek_entropy.hip", "ENT_SC")


def test_tiled():
    assert lc.tiled([1, 2, 3], 7).tolist() == [1, 2, 3, 1, 2, 3, 1]
    assert lc.tiled([1, 2, 3], 2).tolist() == [1, 2]
    assert lc.tiled([1, 2, 3], 3).tolist() == [1, 2, 3]
    two_d = lc.tiled(np.arange(6).reshape(3, 2), 4)
    assert two_d.shape == (4, 2) and two_d[3].tolist() == [0, 1]


def test_periodic_states_equal_the_walk():
    """5 columns: phi, psi, chi walking at 5, 25 and 90 degrees, a phi at 5, a psi on the
    gates; 5 periods and a ragged tail"""
    p = 1000
    A, kind = lc.angle_block(71, p, 5)
    assert set(kind) == {0, 1, 2}
    frames = 5 * p + 137
    for width in (15, 0):
        want = nc.rotamer_states(lc.tiled(A, frames), kind, lc.BOUNDS, lc.SHIFTS, width)
        got = lc.periodic_states(A, kind, lc.BOUNDS, lc.SHIFTS, width, frames)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        # every column moves, so the periods are no constant
        assert all(len(np.unique(want[p:, j])) >= 2 for j in range(5))
        # a prefix shorter than a period
        assert np.array_equal(lc.periodic_states(A, kind, lc.BOUNDS, lc.SHIFTS, width, 300),
                              want[:300])


def test_wmi_chunk_where_the_chunk_starts_to_grow():
    C, M = lc.define("ek_wmi.hip", "WMI_CHUNK"), lc.define("ek_wmi.hip", "WMI_MAX_CHUNKS")
    assert lc.wmi_chunk(1) == (C, 1, 64)
    assert lc.wmi_chunk(2 * C + 7) == (C, 3, 64)
    assert lc.wmi_chunk(C * M) == (C, M, C)
    chunk, chunks, last = lc.wmi_chunk(C * M + 1)
    assert chunk > C and chunk % 64 == 0 and chunks < M and 0 < last < chunk
    if (C, M) == (2048, 64):
        assert (chunk, chunks, last) == (2112, 63, 192)
