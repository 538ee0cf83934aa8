"""Frames with exact ties for the sharded k-centers / PAM paths: n frames drawn
with repeats from a few distinct ones, so that copies of one frame are
bit-identical, their distances to anything are bit-identical, and the maximum
of nearly every k-centers step is tied -- within a shard and across shard
boundaries.  (enspara_amd.synth.synth alone never ties: every frame gets its
own noise and rotation.)  numpy only, seeded, no device.  Shared by
tests/test_tied_cases_host.py (the conditions the data must meet, by the oracle
alone), tests/test_sharded_gloo.py, tests/test_gpu_sharded_ties.py and
tools/fuzz_ms.py (FUZZ_DATA=tiled)."""
import collections

import numpy as np

from enspara_amd import sharded, synth

TILE = 256

# (n, A, n_distinct, world, seed, K): the shapes the sharded tie tests share
MAIN = (1537, 5, 60, 3, 7)          # shards of 768 / 512 / 257 frames
MAIN_K = 40
MORE_THAN_DISTINCT_K = 80           # the 60 distinct frames run out: repeats
TWO_SHARDS = (1000, 7, 48, 2, 7)    # 512 / 488
TWO_SHARDS_K = 40
ONE_EMPTY = (500, 3, 24, 3, 7)      # two tiles over three shards: 256 / 244 / 0
ONE_EMPTY_K = 16
EIGHT_SOME_EMPTY = (1400, 3, 36, 8, 7)   # six tiles over eight shards
EIGHT_K = 30


def live_shards(n, world):
    """[(rank, lo, count)] of the shards that hold frames"""
    out = []
    for r in range(world):
        lo, cnt = sharded.shard_bounds(n, world, r)
        if cnt:
            out.append((r, lo, cnt))
    return out


def tied_frames(n, A, n_distinct, world, seed):
    """-> (x float32 [n, A, 3], ids int64 [n]): x[i] is distinct frame ids[i] of
    synth.synth(n_distinct, A, ...), laid out against shard_bounds(n, world, r):

      ids below n_distinct / 3            occur in every shard that holds frames,
      ids below 2 * n_distinct / 3        are absent from the first shard (with
                                          more than three shards: begin in the
                                          second, third, ... in turn),
      the rest                            occur only in the last shard that holds
                                          frames (at world 2: the second).

    Three of the distinct frames are placed by hand: `specials(...)` names them.
    Every distinct frame occurs at least once.  ValueError if a shard is too
    small for the distinct frames it has to hold."""
    B = int(n_distinct)
    if B < 9 or n < 4 * B:
        raise ValueError("tied_frames needs n_distinct >= 9 and n >= 4 * n_distinct")
    rng = np.random.RandomState(seed)
    base = synth.synth(B, A, max(2, B // 4), seed=seed)
    live = live_shards(n, world)
    sp = specials(n, B, world)
    ids = np.zeros(n, dtype=np.int64)
    # the first shard (of those that hold frames) a distinct frame may occur in
    L = len(live)
    first_shard = np.zeros(B, dtype=np.int64)
    mid = np.arange(B // 3, 2 * B // 3)
    first_shard[mid] = np.minimum(L - 1, 1 + (mid - B // 3) % max(1, L - 2))
    first_shard[2 * B // 3:] = L - 1
    for li, (_, lo, cnt) in enumerate(live):
        allowed = np.flatnonzero(first_shard <= li)
        allowed = allowed[allowed != sp["tail_id"]]
        seg = allowed[rng.randint(0, len(allowed), size=cnt)]
        # the third that occurs everywhere, and every id this shard is the first
        # to hold, do occur in it
        must = allowed[(allowed < B // 3) | ~np.isin(allowed, ids[:lo])]
        if len(must) > cnt:
            raise ValueError("shard %d is too small for its distinct frames" % li)
        seg[rng.choice(cnt, size=len(must), replace=False)] = must
        ids[lo:lo + cnt] = seg
    if len(live) > 1:
        # first copy = the last frame of a shard / the first frame of the next
        # (both ids are of the third that the first shard's draw leaves out)
        ids[sp["last_pos"]] = sp["last_id"]
        ids[sp["first_pos"]] = sp["first_id"]
        # ... and both have copies further on
        later = np.arange(sp["first_pos"] + 1, sp["tail_lo"])
        take = (rng.choice(later, size=min(6, len(later)), replace=False)
                if len(later) else later)
        ids[take[::2]] = sp["last_id"]
        ids[take[1::2]] = sp["first_id"]
    # only copies in the partly filled last tile
    ids[sp["tail_pos"]] = sp["tail_id"]
    # a distinct frame whose copies were all written over comes back in the first
    # shard it may occur in, in place of a frame that has another copy there
    fixed = np.zeros(n, dtype=bool)
    fixed[sp["tail_pos"]] = True
    if L > 1:
        fixed[[sp["last_pos"], sp["first_pos"]]] = True
        fixed[take] = True
    for b in np.setdiff1d(np.arange(B), ids):
        _, lo, cnt = live[first_shard[b]]
        seg = ids[lo:lo + cnt]
        spare = np.flatnonzero(~fixed[lo:lo + cnt] & (np.bincount(seg, minlength=B)[seg] > 1))
        if not len(spare):
            raise ValueError("tied_frames(%d, %d, %d, %d, %d): no room for distinct "
                             "frame %d" % (n, A, B, world, seed, b))
        at = lo + int(spare[rng.randint(len(spare))])
        ids[at] = b
        fixed[at] = True
    return np.ascontiguousarray(base[ids]), ids


def specials(n, n_distinct, world):
    """the distinct frames tied_frames places by hand:
      last_id   first copy at last_pos, the LAST frame of the first shard;
      first_id  first copy at first_pos, the FIRST frame of the second shard;
      tail_id   copies at tail_pos only: in the last tile of 256, partly filled
                unless 256 divides n (then: its last frames)."""
    B = int(n_distinct)
    live = live_shards(n, world)
    tail_lo = (n - 1) // TILE * TILE
    tail_pos = np.arange(max(tail_lo, n - 3), n)
    out = dict(tail_id=B - 1, tail_pos=tail_pos, tail_lo=tail_lo,
               last_id=B // 3, first_id=B // 3 + 1, last_pos=-1, first_pos=-1)
    if len(live) > 1:
        out["last_pos"] = live[0][1] + live[0][2] - 1
        out["first_pos"] = live[1][1]
    return out


Census = collections.namedtuple("Census", "centers maxima n_tied cross")


def tie_census(x, K, world):
    """The oracle's step loop (qcp.Prepared.kcenters_step) over K centers from
    frame 0: per step the float32 maximum the next center is picked at, how
    many frames equal it, and whether those frames lie in more than one shard of
    shard_bounds(len(x), world, r)."""
    from oracle import qcp
    n = len(x)
    lows = np.array([sharded.shard_bounds(n, world, r)[0] for r in range(world)])
    P = qcp.Prepared(x)
    dist = np.full(n, np.inf, dtype=np.float32)
    assign = np.full(n, -1, dtype=np.int32)
    centers, maxima, n_tied, cross = [], [], [], []
    nxt = 0
    for k in range(K):
        centers.append(int(nxt))
        _, nxt = P.kcenters_step(P.c[nxt], P.G[nxt], k, dist, assign)
        t = np.flatnonzero(dist == dist.max())
        assert int(nxt) == int(t[0])
        # (shards without frames share their offset with the next: the last of them)
        s = np.searchsorted(lows, t, side="right") - 1
        maxima.append(np.float32(dist.max()))
        n_tied.append(len(t))
        cross.append(len(set(s.tolist())) > 1)
    return Census(centers, np.array(maxima, dtype=np.float32),
                  np.array(n_tied), np.array(cross))


def shard_of(n, world, frames):
    """the rank that holds each of `frames`"""
    out = np.full(len(frames), -1, dtype=np.int64)
    for r, lo, cnt in live_shards(n, world):
        f = np.asarray(frames)
        out[(f >= lo) & (f < lo + cnt)] = r
    return out


def tied_cutoff(x, K, world):
    """a cut-off that is exactly a float32 maximum of the census, tied across a
    shard boundary and not zero: -> (cutoff, number of centers the fit stops at).
    The stop rule is strict (kcenters.py:217, maxdist > cutoff): the fit ends with
    the step that leaves this maximum, on every rank."""
    c = tie_census(x, K, world)
    for k in range(K // 2, K):
        if c.cross[k] and c.maxima[k] > 0 and np.all(c.maxima[:k] > c.maxima[k]):
            return float(c.maxima[k]), k + 1
    raise ValueError("no step with a cross-shard tied maximum")


def pam_cost_ties(x, K, world, seed, sweeps):
    """The oracle's PAM sweeps after its K-center fit, proposal by proposal: ->
    [(sweep, cluster)] of the proposals whose verdict (kmedoids.py:680-683, new
    cost < cost) hangs on the order of a float64 sum -- the mean over the whole
    array says one thing, the sum of the shards' sums the other.  On tied frames
    a proposal can leave a permutation of the squared distances: the costs are
    equal, and whether they compare equal is the last bit of the sum.  No sharded
    sum -- the reference's own per-rank sums included (kmedoids.py:478-479) --
    reproduces the single-process verdict there, so a bit-for-bit comparison of
    sharded PAM sweeps with the oracle is made where this list is empty."""
    from oracle import cluster as oc
    from oracle import qcp
    n = len(x)
    P = qcp.Prepared(x)
    inds, a, d = oc.kcenters(P, n_clusters=K)
    inds = [int(i) for i in inds]
    rs = np.random.RandomState(seed)
    spans = [(lo, lo + cnt) for _, lo, cnt in live_shards(n, world)]

    def sharded_sum(v):
        return sum(float(np.square(v[lo:hi]).sum()) for lo, hi in spans)

    out = []
    metric = oc._metric_on(P)
    for sweep in range(sweeps):
        for cid in range(len(inds)):
            # one proposal of oracle.cluster.pam_update_numpy (kmedoids.py:611-683)
            prop = int(rs.choice(np.flatnonzero(a == cid)))
            m = metric(P.xyz[prop])
            down = d > m
            trial_d = np.where(down, m, d).astype(np.float64)
            trial_a = np.where(down, cid, a)
            sub = np.flatnonzero((d <= m) & (a == cid))
            if len(sub):
                tr = [P.xyz[i] for i in inds]
                tr[cid] = P.xyz[prop]
                trial_a[sub], trial_d[sub] = oc.assign_to_nearest_center(P.xyz[sub], tr)
            whole = bool(oc.msq(trial_d) < oc.msq(d))
            if whole != (sharded_sum(trial_d) / n < sharded_sum(d) / n):
                out.append((sweep, cid))
            if whole:
                d, a = trial_d, trial_a
                inds[cid] = prop
    # (the replay is the oracle's sweep)
    want = oc.kcenters(P, n_clusters=K)
    rs2, wi, wa, wd = np.random.RandomState(seed), want[0], want[1], want[2]
    for sweep in range(sweeps):
        wi, wd, wa = oc.pam_update(P, wi, wa, wd, random_state=rs2)
    assert [int(i) for i in wi] == inds and np.array_equal(wd, d)
    return out
