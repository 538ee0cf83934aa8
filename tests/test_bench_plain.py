"""bench.py's plain run and --full (bench.parse), and the threaded frame
generator of its setup (bench.make_shard) -- no GPU."""
import argparse
import importlib.util
import os

import numpy as np
import pytest

from enspara_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_turns_the_other_legs_off():
    a = _bench().parse([])
    assert not a.full
    assert a.pam_sweeps == 0 and a.no_msm and a.no_cpu_baseline
    # the off switches the project's scripts pass stay accepted
    a = _bench().parse(["--pam-sweeps", "0", "--no-msm", "--no-cpu-baseline"])
    assert a.pam_sweeps == 0 and a.no_msm and a.no_cpu_baseline


def test_full_keeps_the_legs_and_their_defaults():
    a = _bench().parse(["--full"])
    assert a.full
    assert a.pam_sweeps is None          # 1 on one GPU, 0 on several, decided later
    assert not a.no_msm and not a.no_cpu_baseline
    assert a.cpu_seconds == 15.0 and a.pam_runs == 2 and a.msm_frames == 10_000_000
    a = _bench().parse(["--full", "--cpu-seconds", "0", "--pam-sweeps", "2",
                        "--pam-runs", "3", "--msm-frames", "1000"])
    assert (a.cpu_seconds, a.pam_sweeps, a.pam_runs, a.msm_frames) == (0.0, 2, 3, 1000)


@pytest.mark.parametrize("argv", [["--cpu-seconds", "0"], ["--pam-sweeps", "1"],
                                  ["--pam-runs", "2"], ["--msm-frames", "100"]])
def test_full_only_options_are_refused_without_full(argv, capsys):
    with pytest.raises(SystemExit) as e:
        _bench().parse(argv)
    assert e.value.code == 2
    assert "only with --full" in capsys.readouterr().err


def _args(frames):
    return argparse.Namespace(templates=16, atoms=4, seed=3, frames=frames)


@pytest.mark.parametrize("threads", [1, 3, 8])
def test_make_shard_threads_give_the_same_frames(threads):
    """Any number of threads, any block: the frames of the sequential stream."""
    b = _bench()
    n = 3 * synth.CHUNK + 1234
    whole = synth.synth(n, 4, 16, seed=3)
    got = b.make_shard(_args(n), 0, n, n, threads)
    assert got.dtype == np.float32 and np.array_equal(got, whole)
    # blocks that start and end inside chunks (strong scaling's cuts)
    for lo, cnt in ((0, 1), (5, synth.CHUNK), (synth.CHUNK - 7, 2 * synth.CHUNK + 9),
                    (n - 100, 100)):
        np.testing.assert_array_equal(b.make_shard(_args(n), lo, cnt, n, threads),
                                      whole[lo:lo + cnt])
