"""euclidean / manhattan / hamming distance of one point to a set of points,
on the device.

Same call surface, validation errors and float64 output as the reference's
Cython module enspara/geometry/libdist.pyx (:148-203; checks :31-74).
``euclidean.bind(X)`` keeps the sample matrix resident on the GPU, so that
clustering loops which call ``metric(X, y)`` once per center upload X once.
"""
import ctypes as C

import numpy as np

from .. import _lib
from ..exception import DataInvalid

_KIND = {"float32": 0, "float64": 1, "int64": 2}


def _check(X, y, out):
    """reference libdist.pyx:31-74"""
    if len(X.shape) != 2:
        raise DataInvalid(
            "Data array dimension must be two, got shape %s." % str(X.shape))
    if len(y.shape) != 1:
        raise DataInvalid(
            "Target point dimension must be one, got shape %s." % str(y.shape))
    if X.shape[1] != y.shape[0]:
        raise DataInvalid(
            ("Target data point dimension (%s) must match data "
             "array dimension (%s)") % (y.shape[0], X.shape[1]))
    if out is None:
        return np.zeros((X.shape[0]), dtype=np.float64)
    if out.dtype != np.float64:
        raise DataInvalid(
            "In-place output array must be np.float64, got '%s'." % out.dtype)
    if out.shape[0] != X.shape[0]:
        raise DataInvalid(
            ("In-place output array dimension (%s) must match number of "
             "samples in data array (%s)") % (out.shape[0], X.shape[0]))
    if len(out.shape) != 1:
        raise DataInvalid(
            "In-place output array must be one-dimensional, got shape %s"
            % (out.shape,))
    return out


class _Resident:
    """One sample matrix on the device (ek_feat)."""

    def __init__(self, Xc, kind, device):
        self.L = _lib.load()
        self.kind = kind
        self.n = int(Xc.shape[0])
        h = C.c_void_p()
        _lib.check(self.L.ek_feat_create(int(device), Xc.shape[0], Xc.shape[1],
                                         kind, C.byref(h)))
        self._h = h
        try:
            _lib.check(self.L.ek_feat_load(self._h, Xc.ctypes.data_as(C.c_void_p),
                                           0, Xc.shape[0]))
        except BaseException:       # (nobody gets the object: give the handle back now)
            self.L.ek_feat_destroy(self._h)
            self._h = None
            raise

    def distance(self, metric, yc, out):
        _lib.check(self.L.ek_feat_distance(
            self._h, int(metric), yc.ctypes.data_as(C.c_void_p),
            _lib.f64p(out)))

    def kcenters(self, metric, first_label, max_new, cutoff, dist, assign):
        """ek_feat_kcenters on this matrix; dist (float64) / assign (int32) are
        updated in place.  -> (center samples int64 [k], distances.max())"""
        centers = np.empty(max(int(max_new), 1), dtype=np.int64)
        k = C.c_int32()
        fmax = C.c_double()
        _lib.check(self.L.ek_feat_kcenters(
            self._h, int(metric), int(first_label), int(max_new), float(cutoff),
            _lib.f64p(dist), _lib.i32p(assign), _lib.i64p(centers), C.byref(k),
            C.byref(fmax)))
        return centers[:k.value].copy(), fmax.value

    def assign_nearest(self, metric, centers):
        """ek_feat_assign_nearest: every sample against ``centers`` ([K, F] in
        this matrix's working dtype) in one launch; the result is the handle's
        resident state.  -> (distances float64 [n], labels int32 [n])"""
        n = int(self.n)
        cc = np.ascontiguousarray(centers)
        _lib.check(self.L.ek_feat_assign_nearest(
            self._h, int(metric),
            cc.ctypes.data_as(C.c_void_p) if len(cc) else None, len(cc)))
        d = np.empty(n, dtype=np.float64)
        a = np.empty(n, dtype=np.int32)
        if n:
            _lib.check(self.L.ek_feat_state_download(self._h, _lib.f64p(d),
                                                     _lib.i32p(a)))
        return d, a

    def pam_sweep(self, metric, medoids, proposals, raw, pos, dist, assign, accept,
                  cid):
        """ek_feat_pam_sweep on this matrix from cluster `cid` on; medoids
        (int64), dist (float64), assign (int32) and accept (int32) are updated
        in place.  -> (status, cid, pos)"""
        p = C.c_int64(int(pos))
        c = C.c_int32(int(cid))
        st = C.c_int32(0)
        props = None
        if proposals is not None:
            props = np.ascontiguousarray(proposals, dtype=np.int64)
        _lib.check(self.L.ek_feat_pam_sweep(
            self._h, int(metric), len(medoids), _lib.i64p(medoids),
            _lib.i64p(props) if props is not None else None,
            raw.ctypes.data_as(C.POINTER(C.c_uint32)), len(raw), C.byref(p),
            _lib.f64p(dist), _lib.i32p(assign), _lib.i32p(accept), C.byref(c),
            C.byref(st)))
        return st.value, c.value, p.value

    def close(self):
        if getattr(self, "_h", None):
            self.L.ek_feat_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FeatureStore(_Resident):
    """One shard of a sample set on the device for the k-centers loop over
    several shards (ek_feat_create_sharded, ek_feat_kcenters_step): this
    handle's samples are [global_offset, global_offset + n) of the whole set,
    its float64 distances and int32 labels stay on the device.  ``stream``: a
    hipStream_t handle (e.g. ``torch.cuda.Stream().cuda_stream``) the launches
    go to, so that a caller's collectives on that stream are ordered with them;
    0 / None: a stream of the handle's own.  Counterpart of
    :class:`enspara_amd.device.FrameStore` for feature metrics."""

    def __init__(self, Xc, kind, device=0, global_offset=0, stream=None):
        self.L = _lib.load()
        self.kind = int(kind)
        self.device = int(device)
        self.n, self.F = int(Xc.shape[0]), int(Xc.shape[1])
        self.global_offset = int(global_offset)
        h = C.c_void_p()
        _lib.check(self.L.ek_feat_create_sharded(
            self.device, self.n, self.F, self.kind, self.global_offset,
            C.c_void_p(int(stream) if stream else None), C.byref(h)))
        self._h = h
        try:
            _lib.check(self.L.ek_feat_load(
                self._h, Xc.ctypes.data_as(C.c_void_p) if self.n else None, 0,
                self.n))
        except BaseException:       # (nobody gets the object: give the handle back now)
            self.close()
            raise
        self.record_bytes = int(self.L.ek_feat_record_bytes(self.F, self.kind))
        self.dtype = Xc.dtype

    def distance(self, metric, y, out):
        """metric(X_local, y) into ``out`` (float64 [n]); y in any dtype"""
        y = np.ascontiguousarray(y, dtype=self.dtype)
        if y.shape != (self.F,):
            raise DataInvalid("Target data point dimension (%s) must match data "
                              "array dimension (%s)" % (y.shape, self.F))
        if self.n:
            super().distance(metric, y, out)

    def assign_nearest(self, metric, centers):
        """every local sample against ``centers`` ([K, F], any dtype) in one
        launch on this store's stream; the state on the device becomes the
        result (lowest index among equal distances, label 0 / +inf where no
        distance is below +inf), ready for ``local_candidate`` /
        ``kcenters_step``.  -> (distances float64 [n], labels int32 [n])"""
        c = _centers_array(centers, self.F, self.dtype)
        return super().assign_nearest(metric, c)

    @classmethod
    def from_array(cls, X, metric, device=0, global_offset=0, stream=None):
        """X in the dtype ``metric`` (0 euclidean, 1 manhattan, 2 hamming)
        computes in: float32 stays, int64 for hamming, float64 otherwise"""
        Xa = np.asarray(X)
        dt = _working_dtype(Xa, metric == 2)
        return cls(np.ascontiguousarray(Xa, dtype=dt), _KIND[np.dtype(dt).name],
                   device, global_offset, stream)

    def reset_state(self):
        _lib.check(self.L.ek_feat_state_reset(self._h))

    def upload_state(self, distances, assignments):
        d = np.ascontiguousarray(distances, dtype=np.float64)
        a = np.ascontiguousarray(assignments, dtype=np.int32)
        if len(d) != self.n or len(a) != self.n:
            raise DataInvalid("state of %d / %d entries for %d samples"
                              % (len(d), len(a), self.n))
        _lib.check(self.L.ek_feat_state_upload(self._h, _lib.f64p(d),
                                               _lib.i32p(a)))

    def download_state(self):
        """-> (distances float64 [n], labels int32 [n]) on the host"""
        d = np.empty(self.n, dtype=np.float64)
        a = np.empty(self.n, dtype=np.int32)
        _lib.check(self.L.ek_feat_state_download(self._h, _lib.f64p(d),
                                                 _lib.i32p(a)))
        return d, a

    def local_candidate(self, rec_ptr):
        _lib.check(self.L.ek_feat_local_candidate(self._h, C.c_void_p(rec_ptr)))

    def kcenters_step(self, metric, recs_ptr, n_recs, label, cutoff, own_ptr):
        _lib.check(self.L.ek_feat_kcenters_step(
            self._h, int(metric), C.c_void_p(recs_ptr), int(n_recs), int(label),
            float(cutoff), C.c_void_p(own_ptr)))

    def history(self, first, count):
        """-> (global indices int64 [count], distances float64 [count], n_done)"""
        idx = np.empty(max(int(count), 1), dtype=np.int64)
        cd = np.empty(max(int(count), 1), dtype=np.float64)
        n_done = C.c_int32()
        _lib.check(self.L.ek_feat_history_download(
            self._h, int(first), int(count), _lib.i64p(idx), _lib.f64p(cd),
            C.byref(n_done)))
        return idx[:count], cd[:count], n_done.value

    def reset_history(self):
        _lib.check(self.L.ek_feat_history_reset(self._h))

    # the PAM sweep over several shards (include/enspara_hip.h, "the same sweep
    # over several shards"): counts / members / rows of THIS shard's samples
    def pam_count_members_batch(self, cid0, count):
        """-> int64 [count]: local members of clusters cid0 ..; synchronises"""
        out = np.zeros(int(count), dtype=np.int64)
        _lib.check(self.L.ek_feat_pam_count_batch(self._h, int(cid0), int(count),
                                                  _lib.i64p(out)))
        return out

    def pam_select_members_batch(self, cid0, js):
        """-> int64 [len(js)]: the js[j]-th local member of cluster cid0 + j
        (-1 where js[j] < 0), after the count of the same clusters"""
        js = np.ascontiguousarray(js, dtype=np.int64)
        out = np.full(len(js), -1, dtype=np.int64)
        _lib.check(self.L.ek_feat_pam_select_batch(
            self._h, int(cid0), len(js), _lib.i64p(js), _lib.i64p(out)))
        return out

    def pam_gather_rows(self, samples, rows, table_ptr):
        """table[rows[i]] = features of local sample samples[i] (device table
        [*, F] in this store's dtype)"""
        s = np.ascontiguousarray(samples, dtype=np.int64)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if len(s) != len(r):
            raise DataInvalid("%d samples for %d table rows" % (len(s), len(r)))
        _lib.check(self.L.ek_feat_pam_gather_rows(
            self._h, len(s), _lib.i64p(s), _lib.i64p(r), C.c_void_p(table_ptr)))

    def pam_begin(self, metric, table_ptr, n_medoids):
        _lib.check(self.L.ek_feat_pam_begin(self._h, int(metric),
                                            C.c_void_p(table_ptr), int(n_medoids)))

    def pam_propose(self, cid, row_ptr, win_lo, win_count, out_ptr):
        _lib.check(self.L.ek_feat_pam_propose(
            self._h, int(cid), C.c_void_p(row_ptr), int(win_lo), int(win_count),
            C.c_void_p(out_ptr)))

    def pam_commit(self, accept):
        _lib.check(self.L.ek_feat_pam_commit(self._h, 1 if accept else 0))

    def close(self):
        if self._h:
            self.L.ek_feat_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _working_dtype(X, hamming):
    if hamming:
        if not np.issubdtype(X.dtype, np.integer):
            raise TypeError("hamming distance needs integer data, got %s"
                            % X.dtype)
        return np.int64
    if X.dtype == np.float32:
        return np.float32
    # integers and float64 are computed in float64 (exact for integer inputs
    # below 2**26, the range where the reference's integer arithmetic is too)
    return np.float64


def _centers_array(centers, F, dt):
    """centers -> contiguous [K, F] in the working dtype (as ``y`` is converted)"""
    if isinstance(centers, np.ndarray):
        c = centers
    else:                   # row by row, as the per-center loop converts them
        rows = [np.ascontiguousarray(r, dtype=dt) for r in centers]
        c = np.stack(rows) if rows else np.zeros((0, F), dtype=dt)
    if c.ndim != 2 or c.shape[1] != F:
        raise DataInvalid("Cluster centers of shape %s do not match data array "
                          "dimension (%s)" % (c.shape, F))
    return np.ascontiguousarray(c, dtype=dt)


class Bound:
    """``metric`` bound to one sample matrix that stays resident on the GPU:
    ``bound(X, y)`` costs one kernel and one read-back when ``X`` is the bound
    array, and falls back to a fresh upload for any other array.  The
    clustering loops bind their data once per fit (the caller must not modify
    the array in place while it is bound)."""

    def __init__(self, metric, X, device=0):
        self.metric = metric
        self.device_metric_id = metric      # (what the unbound callables carry)
        self.X = X
        self.device = device
        Xa = np.asarray(X)
        self.dt = _working_dtype(Xa, metric == 2)
        self.res = None
        if Xa.ndim == 2 and Xa.shape[0] > 0:
            self.res = _Resident(np.ascontiguousarray(Xa, dtype=self.dt),
                                 _KIND[np.dtype(self.dt).name], device)

    def bind(self, X, device=None):
        """The loops bind on entry; a metric already bound to this very array
        is handed on as it is (one upload per fit, not one per sweep)."""
        if X is self.X and (device is None or device == self.device):
            return self
        return Bound(self.metric, X, self.device if device is None else device)

    def assign_nearest(self, centers):
        """the nearest of ``centers`` for every row of the bound matrix, one
        launch (:func:`assign_nearest_resident` without the upload of X)
        -> (assignments int64, distances float64)"""
        if self.res is None:
            return assign_nearest_resident(self.X, self.metric, centers,
                                           self.device)
        Xa = np.asarray(self.X)
        d, a = self.res.assign_nearest(
            self.metric, _centers_array(centers, Xa.shape[1], self.dt))
        return a.astype(np.int64), d

    def __call__(self, X, y, out=None):
        if X is not self.X or self.res is None:
            return _run(self.metric, X, y, out, self.device)
        y = np.asarray(y)
        out = _check(np.asarray(X), y, out)
        self.res.distance(self.metric, np.ascontiguousarray(y, dtype=self.dt),
                          out)
        return out


def _run(metric, X, y, out, device):
    X = np.asarray(X) if not isinstance(X, np.ndarray) else X
    y = np.asarray(y)
    out = _check(X, y, out)
    if X.shape[0] == 0:
        return out
    dt = _working_dtype(X, metric == 2)
    res = _Resident(np.ascontiguousarray(X, dtype=dt),
                    _KIND[np.dtype(dt).name], device)
    try:        # (not left to __del__: a raise keeps this frame, and the handle, alive)
        res.distance(metric, np.ascontiguousarray(y, dtype=dt), out)
    finally:
        res.close()
    return out


def euclidean(X, y, out=None, device=0):
    """sqrt(sum_j (X[i, j] - y[j])**2) for every row i -> float64 [n]
    (reference libdist.pyx:148-165)."""
    return _run(0, X, y, out, device)


euclidean.bind = lambda X, device=0: Bound(0, X, device)
euclidean.device_metric_id = 0


def manhattan(X, y, out=None, device=0):
    """sum_j |X[i, j] - y[j]| for every row i -> float64 [n]
    (reference libdist.pyx:167-184)."""
    return _run(1, X, y, out, device)


manhattan.bind = lambda X, device=0: Bound(1, X, device)
manhattan.device_metric_id = 1


def hamming(X, y, out=None, device=0):
    """fraction of features that differ, for every row i -> float64 [n]
    (reference libdist.pyx:187-203)."""
    return _run(2, X, y, out, device)


hamming.bind = lambda X, device=0: Bound(2, X, device)
hamming.device_metric_id = 2


def kcenters_resident(X, metric_id, first_label, max_new, cutoff, distances,
                      assignments, device=0):
    """The k-centers loop (reference kcenters.py:217-231, :243-311) for one of
    the metrics above with X, the float64 distances and the labels resident on
    the device for the whole run: no metric call, numpy pass or arg-max on the
    host per center.  ``distances`` (float64) and ``assignments`` (any integer
    dtype) are the state on entry; returns (center sample indices, distances,
    assignments, distances.max()), the arrays in the dtypes they came in."""
    Xa = np.asarray(X)
    dt = _working_dtype(Xa, metric_id == 2)
    res = _Resident(np.ascontiguousarray(Xa, dtype=dt),
                    _KIND[np.dtype(dt).name], device)
    d = np.ascontiguousarray(distances, dtype=np.float64).copy()
    a = np.ascontiguousarray(assignments, dtype=np.int32).copy()
    try:
        centers, fmax = res.kcenters(metric_id, first_label, max_new, cutoff, d, a)
    finally:
        res.close()
    return centers, d, a.astype(np.asarray(assignments).dtype), fmax


def assign_nearest_resident(X, metric_id, centers, device=0):
    """The nearest-center scan (reference util.py:186-203) for one of the
    metrics above in one launch, X resident on the device: label 0 and +inf to
    begin with, the centers in ascending order, strict < -- the values and
    labels the per-center loop gives, bit for bit.  ``centers``: [K, F], converted
    to the working dtype as ``y`` is.  Returns (assignments int64, distances
    float64).  Counterpart of :func:`kcenters_resident`."""
    Xa = np.asarray(X)
    if Xa.ndim != 2:
        raise DataInvalid(
            "Data array dimension must be two, got shape %s." % str(Xa.shape))
    dt = _working_dtype(Xa, metric_id == 2)
    c = _centers_array(centers, Xa.shape[1], dt)
    if Xa.shape[0] == 0:
        return np.zeros(0, dtype=np.int64), np.full(0, np.inf)
    res = _Resident(np.ascontiguousarray(Xa, dtype=dt),
                    _KIND[np.dtype(dt).name], device)
    try:
        d, a = res.assign_nearest(metric_id, c)
    finally:
        res.close()
    return a.astype(np.int64), d
