"""The MSM count and row-normalise operations in plain numpy, written as the
reference's documentation describes them (enspara/msm/transition_matrices.py:113-170
and :310-321, builders.py:171-204), not as enspara_amd/csrc/ek_msm.hip computes them:
a Python loop over the trajectories, slices, one bincount.  tests/test_msm_reference.py
pins this file to the real reference's recorded outputs and to scipy;
tests/test_gpu_msm_oracle.py then compares the kernels with it.

Also the named case grid both of those files walk.  Every case is seeded and is
(name, flat int32 labels, int64 lengths, lag, sliding, K)."""
import collections

import numpy as np

LD = np.longdouble


# ---- transition counts ----------------------------------------------------------------
def _cell_ids(flat, lengths, lag, sliding, K):
    """int64 ids from * K + to of every transition, trajectory by trajectory"""
    flat = np.asarray(flat)
    lag = int(lag)
    ids = []
    pos = 0
    for n in np.asarray(lengths, dtype=np.int64):
        a = flat[pos:pos + n]
        pos += int(n)
        a = a[a != -1].astype(np.int64)
        if sliding:
            start, end = a[:-lag], a[lag:]
        else:
            every = a[::lag]
            start, end = every[:-1], every[1:]
        assert len(start) == len(end)
        ids.append(start * K + end)
    assert pos == len(flat)
    return np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)


def counts_ref(flat, lengths, lag, sliding, K):
    """-> COO (rows, cols, counts), int64, sorted by (row, col), duplicates summed"""
    ids = _cell_ids(flat, lengths, lag, sliding, K)
    table = np.bincount(ids, minlength=K * K).astype(np.int64)
    cells = np.flatnonzero(table)
    return cells // K, cells % K, table[cells]


def counts_ref_sparse(flat, lengths, lag, sliding, K):
    """counts_ref without the dense K x K table (for a K whose table is gigabytes)"""
    ids = _cell_ids(flat, lengths, lag, sliding, K)
    cells, counts = np.unique(ids, return_counts=True)
    return cells // K, cells % K, counts.astype(np.int64)


# ---- row normalisation ----------------------------------------------------------------
def rowsums_ref(indptr, data):
    """per row the float64 sum taken left to right in storage order"""
    data = np.asarray(data, dtype=np.float64)
    w = np.zeros(len(indptr) - 1, dtype=np.float64)
    for r in range(len(w)):
        row = data[indptr[r]:indptr[r + 1]]
        if len(row):
            w[r] = np.cumsum(row)[-1]
    return w


def rownorm_ref(indptr, data):
    """-> (bit reference, truth), both [nnz].
    Bit reference: w = sequential float64 row sum, inv = 1 / w if w > 0 else 0,
    out = inv * data (builders.py:190-195).  Truth: the same row sum in long double,
    then data / w, in long double."""
    data = np.asarray(data, dtype=np.float64)
    w = rowsums_ref(indptr, data)
    bit = np.zeros(len(data), dtype=np.float64)
    truth = np.zeros(len(data), dtype=LD)
    for r in range(len(w)):
        lo, hi = indptr[r], indptr[r + 1]
        row = data[lo:hi]
        if not len(row):
            continue
        inv = np.float64(1.0) / w[r] if w[r] > 0 else np.float64(0.0)
        bit[lo:hi] = inv * row
        wl = np.cumsum(row.astype(LD))[-1]
        truth[lo:hi] = row.astype(LD) / wl if wl > 0 else LD(0)
    return bit, truth


# ---- the case grid ----------------------------------------------------------------------
Case = collections.namedtuple("Case", "name flat lengths lag sliding K")
_MAKERS = collections.OrderedDict()
#: cases whose numpy / scipy construction takes seconds or whose table takes gigabytes
LARGE = ("scan_two_batches", "one_state_3e6", "K46341")
K_HUGE = 46341          # the first K with K * K > 2^31
#: the cases without a single transition (tests/test_msm_reference.py holds the list
#: to the reference)
NO_TRANSITIONS = ("compact_n1", "all_minus1", "only_empty")


def _case(name, lag=1, sliding=True, K=7):
    def deco(fn):
        def make():
            out = fn(np.random.RandomState(abs(hash_name(name)) % (2 ** 31)))
            flat, lengths = out[0], out[1]
            k = out[2] if len(out) > 2 else K
            flat = np.ascontiguousarray(flat, dtype=np.int32)
            lengths = np.ascontiguousarray(lengths, dtype=np.int64)
            assert lengths.sum() == len(flat) and (lengths >= 0).all()
            assert flat.size == 0 or (flat.min() >= -1 and flat.max() < k)
            return Case(name, flat, lengths, lag, sliding, k)
        assert name not in _MAKERS
        _MAKERS[name] = make
        return fn
    return deco


def hash_name(name):
    """a seed from the case's name that does not change between processes"""
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def case_names(large=True):
    return [n for n in _MAKERS if large or n not in LARGE]


def make_case(name):
    return _MAKERS[name]()


def reference_of(case):
    fn = counts_ref_sparse if case.K >= 10000 else counts_ref
    return fn(case.flat, case.lengths, case.lag, case.sliding, case.K)


def _uniform(rng, n, K, gaps=0.0):
    a = rng.randint(K, size=n)
    if gaps:
        a[rng.rand(n) < gaps] = -1
    return a


def _walk(rng, n, K, band=2, gaps=0.0):
    a = (rng.randint(K) + np.cumsum(rng.randint(-band, band + 1, size=n))) % K
    if gaps:
        a[rng.rand(n) < gaps] = -1
    return a


def _with_gaps(rng, live, n_gaps):
    """the labels `live` with n_gaps frames of -1 put in at random places"""
    out = np.full(len(live) + n_gaps, -1, dtype=np.int64)
    keep = np.sort(rng.choice(len(out), size=len(live), replace=False))
    out[keep] = live
    return out


# -- compaction: the frame count round the 1024 frames of a workgroup, the -1 frames
for _n in (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 1024 * 1024 - 1, 1024 * 1024 + 1):
    @_case("compact_n%d" % _n)
    def _(rng, n=_n):
        return _uniform(rng, n, 7, 0.1), [n // 3, n - n // 3]


@_case("minus1_first")
def _(rng):
    a = _uniform(rng, 3000, 7)
    a[0] = -1
    return a, [3000]


@_case("minus1_last")
def _(rng):
    a = _uniform(rng, 3000, 7)
    a[-1] = -1
    return a, [1700, 1300]


@_case("minus1_run_across_1024")
def _(rng):
    a = _uniform(rng, 3000, 7)
    a[1000:1051] = -1
    return a, [3000]


@_case("minus1_whole_block")
def _(rng):
    a = _uniform(rng, 4096, 7)
    a[1024:2048] = -1
    return a, [4096]


@_case("all_minus1")
def _(rng):
    return np.full(2500, -1), [1000, 0, 1500]


@_case("no_minus1")
def _(rng):
    return _uniform(rng, 5000, 7), [5000]


@_case("scan_two_batches", K=300)
def _(rng):
    # 17 * 2^20 + 5 frames: 17409 workgroups of the squeeze, 18 counts per thread of
    # the scan -- one batch of sixteen and two of the next
    n = 17 * 1024 * 1024 + 5
    a = _walk(rng, n, 300, band=3, gaps=0.001)
    return a, [n // 2 + 77, n - n // 2 - 77]


# -- trajectory starts
@_case("start_on_1024_4096", lag=2)
def _(rng):
    lengths = [1024, 3072, 4096, 500]
    return _uniform(rng, sum(lengths), 7), lengths


@_case("start_on_1024_with_gaps", lag=2)
def _(rng):
    lengths = [1024, 1024, 2048, 4096, 500]
    return _uniform(rng, sum(lengths), 7, 0.05), lengths


@_case("empty_leading", lag=2)
def _(rng):
    return _uniform(rng, 900, 7, 0.05), [0, 0, 400, 500]


@_case("empty_trailing", lag=2)
def _(rng):
    return _uniform(rng, 900, 7, 0.05), [400, 500, 0, 0]


@_case("empty_middle", lag=2)
def _(rng):
    return _uniform(rng, 900, 7, 0.05), [400, 0, 0, 0, 500]


@_case("only_empty")
def _(rng):
    return np.zeros(0), [0, 0, 0, 0, 0]


@_case("dead_between_live", lag=2)
def _(rng):
    a = _uniform(rng, 1300, 7, 0.02)
    a[500:800] = -1
    return a, [500, 300, 500]


for _sl in (True, False):
    @_case("squeezed_lengths_round_lag_sw%d" % _sl, lag=5, sliding=_sl)
    def _(rng):
        # squeezed lengths lag - 1, lag, lag + 1, 2 lag + 1, each behind some -1 frames
        rows = [_with_gaps(rng, _uniform(rng, m, 7), 3) for m in (4, 5, 6, 11, 6, 4)]
        return np.concatenate(rows), [len(r) for r in rows]


@_case("one_trajectory", lag=3)
def _(rng):
    return _walk(rng, 7000, 7, gaps=0.01), [7000]


for _starts in (15, 16, 17, 18):
    for _sl in (True, False):
        @_case("starts_%d_in_one_block_sw%d" % (_starts, _sl), lag=3, sliding=_sl, K=11)
        def _(rng, starts=_starts):
            # positions [4096, 8192) are one workgroup's: its first lies in trajectory
            # 0, and exactly `starts` trajectories begin inside it (sixteen starts are
            # staged in LDS; a position behind them searches)
            lengths = [4196] + list(rng.randint(150, 200, size=starts - 1)) + [3000]
            assert 4096 < sum(lengths[:-1]) < 8192 < sum(lengths)
            return _uniform(rng, sum(lengths), 11), lengths


for _lag in (2, 40):
    @_case("trj_4000_short_lag%d" % _lag, lag=_lag, K=50)
    def _(rng):
        lengths = rng.randint(0, 90, size=4000)
        lengths[::17] = 0
        return _uniform(rng, int(lengths.sum()), 50, 0.05), lengths


@_case("block_starts_behind_empty_run", lag=2)
def _(rng):
    # position 4096 is the first of a workgroup and of trajectory 6
    lengths = [4096, 0, 0, 0, 0, 0, 3000]
    return _uniform(rng, sum(lengths), 7), lengths


@_case("block_inside_trajectory_behind_empty_run", lag=2, sliding=False)
def _(rng):
    lengths = [4001, 0, 0, 0, 3000]
    return _uniform(rng, sum(lengths), 7), lengths


# -- lag and window: position + lag leaves the workgroup's 4096 positions
for _lag in (1, 2, 7, 40, 4095, 4096, 4097):
    for _sl in (True, False):
        @_case("lag%d_sw%d" % (_lag, _sl), lag=_lag, sliding=_sl, K=20)
        def _(rng):
            lengths = [9000, 5000, 12001]
            return _walk(rng, sum(lengths), 20, gaps=0.01), lengths


@_case("stride_lag_does_not_divide_length", lag=5, sliding=False)
def _(rng):
    return _uniform(rng, 54, 7), [23, 31]


@_case("stride_starts_off_multiples_of_lag", lag=4, sliding=False)
def _(rng):
    return _uniform(rng, 99, 7), [13, 29, 17, 40]


@_case("stride_last_pair_ends_on_last_frame", lag=6, sliding=False)
def _(rng):
    return _uniform(rng, 50, 7), [25, 25]


@_case("stride_last_pair_ends_one_frame_short", lag=6, sliding=False)
def _(rng):
    return _uniform(rng, 52, 7), [26, 26]


# -- states and cells
for _K in (1, 2, 31, 32, 33):
    @_case("states_%d" % _K, K=_K)
    def _(rng, K=_K):
        return _uniform(rng, 5000, K, 0.01), [2000, 3000], K


@_case("corner_cells", K=33)
def _(rng):
    return rng.choice([0, 32], size=3000), [3000]


@_case("one_state_3e6", K=3)
def _(rng):
    # every addition on one cell
    return np.zeros(3000000), [3000000]


@_case("uniform_300", lag=3, K=300)
def _(rng):
    # transitions all over the table: nothing for an LDS table to gather
    return _uniform(rng, 600000, 300), [100000] * 6


@_case("K46341", K=K_HUGE)
def _(rng):
    # cells beyond 2^31: 46340 * 46341 + 41708 = 2^31 is the first of them
    K = K_HUGE
    assert 46340 * K + 41707 == 2 ** 31 - 1
    a = [46340, 41707, 46340, 41708, 46340, 46340, 0, 46340, 0, -1, 46340, 41708,
         46340, 41707, 46340, 46340, 46340, 0, 0, 46340, 41708]
    b = [0, 46340, 0, 46340, 46340, 41708, 46340, 41707, 46340]
    return np.array(a + b), [len(a), len(b)]


def _cells_on_last_slots(K, per_slot):
    """cells of a K x K table whose hash (cell * 2654435761 mod 2^32) >> 19 is the
    LDS table's slot 8190 or 8191"""
    cells = np.arange(K * K, dtype=np.uint64)
    slot = ((cells * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(19)
    out = []
    for s in (8190, 8191):
        hit = np.flatnonzero(slot == s)
        assert len(hit) >= per_slot
        out.extend(hit[:per_slot].tolist())
    return out


@_case("lds_probe_wraps", K=300)
def _(rng):
    # ten different cells on the last two of 8192 slots, all inside one workgroup's
    # stretch: the probes run over the end of the table to slot 0, and past six
    # probes the addition goes to the global table
    cells = _cells_on_last_slots(300, 5)
    pick = rng.randint(len(cells), size=2000)
    rows = np.array([[cells[i] // 300, cells[i] % 300] for i in pick])
    return rows.reshape(-1), [2] * len(rows)
