"""numpy-backed feature shard for the multi-rank driver tests (TEST CODE).

Implements the one-record shard protocol of enspara_amd/sharded.py
(FeatureShard) on CPU around the oracle's metrics (oracle/features.py), with
the device's record layout (include/enspara_hip.h, ek_feat_record_bytes):
{ double max_dist; int64 global_index; T row[F] }, padded to 16 bytes -- so
that fit_features_sharded's host logic (agreement, offsets, warm start, the
driver loop, the centers' rows) runs with the gloo backend on a machine
without GPUs.  Next to tests/_host_shard.py, which does the same for RMSD."""
import contextlib

import numpy as np
import torch

from oracle import features as of

METRICS = {0: of.euclidean, 1: of.manhattan, 2: of.hamming}


def working_dtype(X, metric_id):
    if metric_id == 2:
        return np.dtype(np.int64)
    return np.dtype(np.float32 if X.dtype == np.float32 else np.float64)


def record_dtype(F, wdt):
    size = (16 + F * wdt.itemsize + 15) // 16 * 16
    return np.dtype({"names": ["maxdist", "gidx", "row"],
                     "formats": ["<f8", "<i8", (wdt, (F,))],
                     "offsets": [0, 8, 16], "itemsize": size})


class HostFeatureShard:
    def __init__(self, X, metric_id, offset):
        self.metric = METRICS[metric_id]
        self.wdt = working_dtype(X, metric_id)
        self.X = np.ascontiguousarray(X, dtype=self.wdt)
        self.n, self.F = self.X.shape
        self.offset = int(offset)
        self.rec = record_dtype(self.F, self.wdt)
        self.dist = np.full(self.n, np.inf)
        self.assign = np.full(self.n, -1, dtype=np.int32)
        self.reset_history()

    @property
    def n_local(self):
        return self.n

    @property
    def record_bytes(self):
        return self.rec.itemsize

    def new_buffer(self, nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8)

    def _records(self, t):
        return t.numpy().view(self.rec)

    def local_candidate(self, rec):
        r = self._records(rec)
        r[0] = np.zeros((), dtype=self.rec)
        if self.n == 0:
            r[0]["maxdist"], r[0]["gidx"] = -np.inf, -1
            return
        i = int(np.argmax(self.dist))
        r[0]["maxdist"], r[0]["gidx"] = self.dist[i], self.offset + i
        r[0]["row"] = self.X[i]

    def step(self, all_recs, n_recs, label, cutoff, own_rec):
        if self.stopped:
            return
        recs = self._records(all_recs)[:n_recs]
        w = int(np.argmax(recs["maxdist"]))          # first index on ties
        mx = float(recs["maxdist"][w])
        if not (mx > cutoff):
            self.stopped = True
            return
        gidx, row = int(recs["gidx"][w]), recs["row"][w].copy()
        if self.n:
            d = self.metric(self.X, row)
            closer = d < self.dist
            self.dist[closer] = d[closer]
            self.assign[closer] = label
        self.hist[label] = (gidx, mx)
        self.n_done = label + 1
        self.local_candidate(own_rec)

    def progress(self):
        return self.n_done

    def history(self, first, count):
        idx = np.full(count, -1, dtype=np.int64)
        cd = np.zeros(count)
        for j in range(count):
            if first + j in self.hist:
                idx[j], cd[j] = self.hist[first + j]
            elif first + j >= self.n_done:
                break
        return idx, cd, self.n_done

    def reset_history(self):
        self.hist, self.n_done, self.stopped = {}, 0, False

    def distance(self, y):
        y = np.asarray(y, dtype=self.wdt)
        return self.metric(self.X, y) if self.n else np.zeros(0)

    def reset_state(self):
        self.dist[:] = np.inf
        self.assign[:] = -1

    def state(self):
        return self.dist.copy(), self.assign.copy()

    def set_state(self, distances, assignments):
        self.dist = np.array(distances, dtype=np.float64)
        self.assign = np.array(assignments, dtype=np.int32)


@contextlib.contextmanager
def make_host_shard(X, metric_id, offset):
    yield HostFeatureShard(X, metric_id, offset)
