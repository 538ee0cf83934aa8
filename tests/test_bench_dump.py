"""bench.py --dump-outputs (bench.dump_outputs): the files, their dtypes and
the fixed sample of frames above DUMP_MAX_FRAMES, with a stand-in for the
device store -- no GPU."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Store:
    """what dump_outputs asks of a FrameStore"""

    def __init__(self, d, a):
        self.d, self.a = d, a

    def download_state(self):
        return self.d.copy(), self.a.copy()


def _state(n):
    rs = np.random.RandomState(3)
    return rs.rand(n).astype(np.float32), rs.randint(0, 7, size=n).astype(np.int32)


def test_dump_outputs_whole_state(tmp_path):
    b = _bench()
    n = 1000
    d, a = _state(n)
    idx = np.array([3, 500, 9], dtype=np.int64)
    cd = np.array([np.inf, 2.5, 1.25], dtype=np.float32)
    b.dump_outputs(str(tmp_path), _Store(d, a), idx, cd, 0, n, n, False, 0)
    assert sorted(os.listdir(tmp_path)) == ["center_distances.npy", "center_indices.npy",
                                            "distances.npy", "labels.npy"]
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert got["center_indices"].dtype == np.float64
    assert got["labels"].dtype == np.float64
    assert got["distances"].dtype == np.float32
    assert got["center_distances"].dtype == np.float32
    np.testing.assert_array_equal(got["center_indices"], idx)
    # (the first center's +inf, which no fit computes, is not an output)
    np.testing.assert_array_equal(got["center_distances"], cd[1:])
    for key, arr in got.items():
        assert np.all(np.isfinite(arr)), key
    np.testing.assert_array_equal(got["labels"], a)
    np.testing.assert_array_equal(got["distances"], d)


def test_dump_outputs_sample_is_fixed(tmp_path):
    b = _bench()
    b.DUMP_MAX_FRAMES = 100
    n = 1000
    d, a = _state(n)
    idx = np.array([0, 1], dtype=np.int64)
    cd = np.array([np.inf, 1.0], dtype=np.float32)
    runs = []
    for k in range(2):
        out = os.path.join(str(tmp_path), str(k))
        os.makedirs(out)
        b.dump_outputs(out, _Store(d, a), idx, cd, 0, n, n, False, 0)
        runs.append({f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)})
    fi = runs[0]["frame_index"]
    assert fi.dtype == np.float64 and len(fi) == 100
    assert np.all(np.diff(fi) > 0) and fi[0] >= 0 and fi[-1] < n
    rows = fi.astype(np.int64)
    np.testing.assert_array_equal(runs[0]["labels"], a[rows])
    np.testing.assert_array_equal(runs[0]["distances"], d[rows])
    for key in runs[0]:
        assert np.all(np.isfinite(runs[0][key])), key
        np.testing.assert_array_equal(runs[0][key], runs[1][key])


def test_dump_outputs_rank_block_of_the_sample(tmp_path):
    """a rank that holds frames [lo, lo + n_local) of n_total keeps the sampled
    frames of its own block, in frame order"""
    b = _bench()
    b.DUMP_MAX_FRAMES = 100
    n_total, lo, n_local = 1000, 400, 300
    d, a = _state(n_total)
    store = _Store(d[lo:lo + n_local], a[lo:lo + n_local])
    b.dump_outputs(str(tmp_path), store, np.array([0]), np.array([np.inf], np.float32),
                   lo, n_local, n_total, False, 0)
    fi = np.load(os.path.join(str(tmp_path), "frame_index.npy")).astype(np.int64)
    mine = fi[(fi >= lo) & (fi < lo + n_local)]
    assert 0 < len(mine) < len(fi)
    np.testing.assert_array_equal(np.load(os.path.join(str(tmp_path), "labels.npy")), a[mine])
    np.testing.assert_array_equal(np.load(os.path.join(str(tmp_path), "distances.npy")),
                                  d[mine])
