"""Sizes and expected values for the tests that push an input past one launch
(tests/test_gpu_launch_limits.py, tests/test_limit_cases_host.py).  Host only: nothing
here imports device code.

Every size of those tests is computed from an integer `#define` of the kernel file it
belongs to, read by `define`, so the tests follow the constants when they change."""
import os
import re

import numpy as np

import _numpy_cards as nc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "enspara_amd", "csrc")


def define(file, name):
    """the integer `#define name` of csrc/<file>"""
    text = open(os.path.join(CSRC, file)).read()
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % re.escape(name), text, re.MULTILINE)
    assert m, "%s has no integer #define %s" % (file, name)
    return int(m.group(1))


def tiled(seq, n):
    """the first n items of the cyclic repetition of seq (along its first axis)"""
    seq = np.asarray(seq)
    reps = -(-n // len(seq))
    return np.tile(seq, (reps,) + (1,) * (seq.ndim - 1))[:n]


BOUNDS = [nc.PHI, nc.PSI, nc.CHI]
SHIFTS = [0, 100, 0]


def angle_block(seed, p, n):
    """float32 [p, n] angles and the kinds of the columns, drawn as tests/test_gpu_rotamer.py
    draws them: column j of kind j % 3, every fifth column on the gates, the others random
    walks at steps of 5, 25 or 90 degrees"""
    rng = np.random.RandomState(seed)
    kind = np.arange(n) % 3
    A = np.zeros((p, n), dtype=np.float32)
    for j in range(n):
        if j % 5 == 4:
            v = np.array(nc.ON_GATES)[rng.randint(0, len(nc.ON_GATES), p)]
            A[:, j] = np.mod(v + SHIFTS[kind[j]], 360)
        else:
            step = (5.0, 25.0, 90.0)[j % 4 % 3]
            A[:, j] = np.mod(np.cumsum(rng.normal(0, step, p)) + rng.uniform(0, 360), 360)
    A[A >= 360] = 0
    assert A.min() >= 0 and A.max() < 360
    assert all(nc.shifted(A[:, j], SHIFTS[kind[j]]).max() < 360 for j in range(n))
    return A, kind


def periodic_states(block, kind, boundaries, shifts, width, frames):
    """The rotamer states of `block` ([p, n] angles) repeated to `frames` frames, without
    walking them: the state of a frame depends on the state before it and the frame's angle
    alone, so once a period starts in the states the period before it started in, it
    repeats.  The restatement walks three periods; period 2 must equal period 3 (the
    caller's angles have to make it so: random walks that visit every basin do).
    -> uint8 [frames, n]: period 1, then period 2 again and again."""
    block = np.asarray(block)
    p = len(block)
    S = nc.rotamer_states(np.concatenate([block] * 3), kind, boundaries, shifts, width)
    assert np.array_equal(S[p:2 * p], S[2 * p:]), "the states do not repeat from period 2 on"
    if frames <= p:
        return S[:frames].copy()
    return np.concatenate([S[:p], tiled(S[p:2 * p], frames - p)])


def keeps_every_start(angle, k, boundaries, shifts, width):
    """Whether a frame with this angle, in a column of kind k, leaves the machine in the
    basin it was in whichever basin that is (the angle lies within the gates of all of
    them): the state of such a frame is the state its chunk started in, if it is the
    chunk's first."""
    hb = np.asarray(boundaries[k], dtype=np.float64)
    for b in range(len(hb) - 1):
        a0 = np.mod(0.5 * (hb[b] + hb[b + 1]) + shifts[k], 360)     # a frame 0 in basin b
        two = np.array([[a0], [angle]], dtype=np.asarray(angle).dtype)
        s = nc.rotamer_states(two, [k], boundaries, shifts, width)
        assert s[0, 0] == b
        if s[1, 0] != b:
            return False
    return True


def wmi_chunk(frames):
    """(chunk, chunks, frames of the last chunk) as ek_wmi.hip cuts `frames` frames: a
    chunk is WMI_CHUNK frames, or what makes WMI_MAX_CHUNKS chunks, in whole steps of 64;
    the chunks cover the frames padded to 64 (ek_mi_tpad), and so does the last count."""
    least, most = define("ek_wmi.hip", "WMI_CHUNK"), define("ek_wmi.hip", "WMI_MAX_CHUNKS")
    chunk = max(least, _up(_up(frames, most), 64) * 64)
    tpad = _up(frames, 64) * 64
    chunks = _up(tpad, chunk)
    return chunk, chunks, tpad - (chunks - 1) * chunk


def _up(a, b):
    return (a + b - 1) // b
