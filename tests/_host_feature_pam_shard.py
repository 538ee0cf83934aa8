"""numpy-backed feature shard that also speaks the PAM methods (TEST CODE):
tests/_host_feature_shard.py's HostFeatureShard plus what
enspara_amd.sharded.pam_sweep_sharded drives -- tables of rows as CPU torch
tensors, the 32-byte record of include/enspara_hip.h ("the same sweep over
several shards") -- around the oracle's metrics, so that the drivers run under
gloo on a machine without GPUs."""
import contextlib

import numpy as np
import torch

from oracle import features as of
from _host_feature_shard import HostFeatureShard

PAM_OUT = np.dtype([("sum_old", "<f8"), ("sum_new", "<f8"), ("n", "<i8"),
                    ("n_amb", "<u4"), ("moved", "<u4")])


class HostFeaturePamShard(HostFeatureShard):
    def host_to_buffer(self, arr):
        return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64))

    def new_table(self, rows):
        return (torch.from_numpy(np.zeros((rows, self.F), dtype=self.wdt)),
                torch.zeros(2 * rows, dtype=torch.int64))

    def fill_rows(self, local, rows, table, meta):
        t = table.numpy()
        for f, r in zip(local, rows):
            assert 0 <= f < self.n
            t[r] = self.X[f]

    def pam_begin_table(self, table, meta, n_medoids):
        self.med = table.numpy()[:n_medoids].copy()
        self.trial = None

    def pam_count_batch(self, cid0, count):
        return np.array([int(np.sum(self.assign == cid0 + j))
                         for j in range(count)], dtype=np.int64)

    def pam_select_batch(self, cid0, js):
        out = np.full(len(js), -1, dtype=np.int64)
        for j, want in enumerate(js):
            if want >= 0:
                out[j] = np.flatnonzero(self.assign == cid0 + j)[want]
        return out

    def pam_count(self, cid):
        return self.pam_count_batch(cid, 1)[0]

    def pam_select(self, cid, j):
        return self.pam_select_batch(cid, [j])[0]

    def pam_prefetch_centers(self, table, meta, count, win_lo=0, win_count=0):
        pass

    def pam_propose_center(self, cid, slot, table, meta, row, n_members_local,
                           win_lo, win_count, out):
        assert self.trial is None
        y = table.numpy()[row].copy()
        rec = out.numpy().view(PAM_OUT)
        rec[0] = np.zeros((), dtype=PAM_OUT)
        med = self.med.copy()
        med[cid] = y
        if self.n == 0:
            self.trial = (med, self.dist, self.assign)
            return
        nd = self.metric(self.X, y)
        d, a = self.dist, self.assign
        new_d, new_a = d.copy(), a.copy()
        down = d > nd
        new_d[down], new_a[down] = nd[down], cid
        sub = np.flatnonzero((d <= nd) & (a == cid))
        if len(sub):
            sa, sd = of.assign_to_nearest_center(self.X[sub], med, self.metric)
            new_a[sub], new_d[sub] = sa, sd
        moved = 0
        for lab in set(a[a != new_a]) | set(new_a[a != new_a]):
            if 0 <= lab - win_lo < win_count:
                moved |= 1 << int(lab - win_lo)
        rec[0]["sum_old"] = np.sum(d ** 2)
        rec[0]["sum_new"] = np.sum(new_d ** 2)
        rec[0]["n"], rec[0]["n_amb"], rec[0]["moved"] = self.n, len(sub), moved
        self.trial = (med, new_d, new_a.astype(np.int32))

    def pam_commit(self, accept):
        if accept:
            self.med, self.dist, self.assign = self.trial
        self.trial = None


@contextlib.contextmanager
def make_host_pam_shard(X, metric_id, offset):
    yield HostFeaturePamShard(X, metric_id, offset)
