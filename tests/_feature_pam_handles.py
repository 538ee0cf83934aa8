"""Several ek_feat handles on one device presented to
enspara_amd.sharded.pam_sweep_sharded as ONE shard (TEST / MEASUREMENT HARNESS):
used by tests/test_gpu_feature_pam_sharded.py and, for its 8-handle line, by
tools/feat_pam_shard_probe.py.  It waits for the stream and recombines the
records on the host for every proposal, so its timings say nothing about the
product's path (sharded.FeatureShard)."""
import numpy as np

REC = np.dtype([("sum_old", "<f8"), ("sum_new", "<f8"), ("n", "<i8"),
                ("n_amb", "<u4"), ("moved", "<u4")])


class Handles:
    """len(cuts) - 1 FeatureStores on one device and stream that look like ONE
    shard to pam_sweep_sharded: tables are added up and records combined in
    handle order, the way the driver does it across ranks."""

    def __init__(self, X, mid, cuts):
        import torch
        from enspara_amd import sharded
        from enspara_amd.geometry.libdist import FeatureStore
        self.torch, self.cuts, self.mid = torch, cuts, mid
        self.S = len(cuts) - 1
        self.ts = torch.cuda.Stream(device=0)
        self.stores = [FeatureStore.from_array(
            X[cuts[s]:cuts[s + 1]], mid, device=0, global_offset=cuts[s],
            stream=self.ts.cuda_stream) for s in range(self.S)]
        self.views = [sharded.FeatureShard(st, mid) for st in self.stores]
        self.device = self.views[0].device
        self.offset, self.n_local = 0, int(cuts[-1])
        self.recs = torch.zeros(32 * self.S, dtype=torch.uint8, device="cuda")
        self.max_amb = 0

    def close(self):
        for st in self.stores:
            st.close()

    def set_state(self, d, a):
        for s, st in enumerate(self.stores):
            st.upload_state(d[self.cuts[s]:self.cuts[s + 1]],
                            a[self.cuts[s]:self.cuts[s + 1]].astype(np.int32))

    def state(self):
        parts = [st.download_state() for st in self.stores]
        return (np.concatenate([p[0] for p in parts]),
                np.concatenate([p[1] for p in parts]))

    def host_to_buffer(self, arr):
        return self.views[0].host_to_buffer(arr)

    def new_buffer(self, nbytes):
        return self.views[0].new_buffer(nbytes)

    def new_table(self, rows):
        return self.views[0].new_table(rows)

    def _owner(self, g):
        return max(s for s in range(self.S) if self.cuts[s] <= g and
                   self.cuts[s + 1] > g)

    def fill_rows(self, samples, rows, table, meta):
        for g, r in zip(samples, rows):
            s = self._owner(int(g))
            # every handle writes into a table of its own, the tables are added
            own = self.torch.zeros_like(table)
            self.views[s].fill_rows([int(g) - self.cuts[s]], [r], own, meta)
            table.view(self.torch.int32).add_(own.view(self.torch.int32))

    def pam_begin_table(self, table, meta, K):
        for v in self.views:
            v.pam_begin_table(table, meta, K)

    def pam_count_batch(self, cid0, count):
        self.cnt = np.array([v.pam_count_batch(cid0, count) for v in self.views])
        return self.cnt.sum(axis=0)

    def pam_select_batch(self, cid0, js):
        out = np.full(len(js), -1, dtype=np.int64)
        before = np.cumsum(np.vstack([np.zeros_like(self.cnt[0]), self.cnt]),
                           axis=0)
        for s, v in enumerate(self.views):
            loc = [int(j - before[s][q]) if j >= 0 and
                   0 <= j - before[s][q] < self.cnt[s][q] else -1
                   for q, j in enumerate(js)]
            if max(loc) >= 0:
                got = v.pam_select_batch(cid0, loc)
                for q, f in enumerate(got):
                    if loc[q] >= 0:
                        assert f >= 0
                        out[q] = self.cuts[s] + int(f)
        return out

    def pam_count(self, cid):
        return self.pam_count_batch(cid, 1)[0]

    def pam_select(self, cid, j):
        return self.pam_select_batch(cid, [j])[0]

    def pam_prefetch_centers(self, *a, **k):
        pass

    def pam_propose_center(self, cid, slot, table, meta, row, n_members_local,
                           win_lo, win_count, out):
        for s, v in enumerate(self.views):
            v.pam_propose_center(cid, slot, table, meta, row, 0, win_lo,
                                 win_count, self.recs[32 * s:32 * s + 32])
        self.torch.cuda.current_stream().synchronize()
        recs = self.recs.cpu().numpy().view(REC)
        tot = np.zeros(1, dtype=REC)
        s_old = s_new = 0.0
        for s in range(self.S):                 # handle order = rank order
            assert recs[s]["n"] == self.cuts[s + 1] - self.cuts[s]
            s_old += float(recs[s]["sum_old"])
            s_new += float(recs[s]["sum_new"])
            tot[0]["moved"] |= recs[s]["moved"]
            tot[0]["n_amb"] += recs[s]["n_amb"]
        tot[0]["sum_old"], tot[0]["sum_new"] = s_old, s_new
        tot[0]["n"] = self.n_local
        self.max_amb = max(self.max_amb, int(tot[0]["n_amb"]))
        out.copy_(self.torch.from_numpy(tot.view(np.uint8)))

    def pam_commit(self, accept):
        for v in self.views:
            v.pam_commit(accept)
