"""The RMSD k-centers picks where their reductions change form with the number of
frames, on data whose maxima are tied across the whole shard.

Every bit-exact promise of the k-centers path rests on one property: the next center
is the FIRST-index arg-max of the current distances.  The reductions that find it span
the shard, and their code changes with the frame count:

    more than 1024 block maxima (n > 262 144)   a thread of ek_pick_kernel, ek_block_argmax,
                                                ek_chain_reduce folds several entries, stride 1024
    1024, 2048 ... entries                      ek_pick_top_body reads 1 .. 8 entries per thread
    more than 8192 entries (n > 2 097 152)      its tail: a thread keeps the 8 largest of its share
    n > 524 288                                 maxima per 64 frames -> per 256 (ek_fine_fits);
                                                per-prefix maxima in the pass -> chain-kernel
                                                sweep (ek_sweep_pays)
    n >= 524 161, n >= 1 048 321                frames per lane 1 -> 2 -> 4 (ek_pick_fpl)
    n > 65 536, n > 262 144                     ek_view_scan_kernel: cross-wave offsets, more than
                                                one count per thread

Sizes (none but the thresholds themselves a multiple of 256): 262 401; 524 160 | 524 161;
524 288 | 524 289; 1 048 320 | 1 048 321; 2 098 177 (8197 block maxima).  Atoms 3, 4, 5
(both remainders mod 4; 3 at the largest size), 24 to 32 centers.

Data, all from enspara_amd.synth:
  tiled   n draws (with repeats) from ~4500 distinct frames: every maximum is tied among
          about n / 4500 bit-identical frames scattered over the whole shard
  late    a head of 300 000 frames drawn from 50 of the distinct frames, then a tiled
          tail: the first occurrences -- the centers -- lie deep in the array
  tail    tiled, but every other center of the fit occurs ONLY in the last 1025 frames of
          2 098 177 (twice each): block maxima 8192 .. 8196, which only the tail of
          ek_pick_top_body reads
  walk    synth.walk: all distinct, no gap in the distances

Bars as everywhere: center indices and labels equal, distances equal as float32 bits,
against oracle.cluster.kcenters / pam_update.  No expected value comes from a device
call.  Every case asserts the condition on the data that makes it a test and, through
FrameStore.last_run_form() / view_stats() / ti_stats(), the form it means to reach; the
thresholds are restated here (_expected_form), so a threshold that moves shows.
"""
import numpy as np
import pytest

from enspara_amd import synth

pytestmark = pytest.mark.gpu

FOLD = 1024 * 256           # frames between two entries of one thread's strided fold
M_DISTINCT = 4500

# option defaults, said before every run (a store is shared by the runs of its size)
DEFAULTS = dict(candidates=-1, chained=1, fused_rounds=1, pass_sweep=1, fine_pick=1,
                nontemporal=-1, active_view=1, triangle=0, adaptive=1, fpl=0)


# ---- data ---------------------------------------------------------------------------------
def _fit_of_distinct(base, first_id, k):
    """the distinct frames that k-centers accepts, in order, when the shard starts with
    base[first_id]: copies change no maximum, and ties between DISTINCT frames do not
    occur, so this holds for every arrangement of the copies (check_data holds it to
    the oracle's fit of the whole shard)"""
    from oracle import cluster as oc
    order = np.concatenate([[first_id], np.delete(np.arange(len(base)), first_id)])
    ctr, _, _ = oc.kcenters(np.ascontiguousarray(base[order]), n_clusters=k)
    return order[np.asarray(ctr)]


def _draws(n, A, seed, head=0, fold_k=0, tail_k=0):
    """-> (base [m, A, 3], ids [n]): frame f of the shard is base[ids[f]].
    head: that many leading frames drawn from 50 of the distinct frames only.
    fold_k: the first fold_k centers of the fit are put at positions 0, 5, 10 ... of the
    first block of 256, and the whole block is repeated FOLD frames on -- at 262 401
    frames the only place where one thread's fold sees two entries (0 and 1024).
    tail_k: of the first tail_k centers every other one (not the first) is taken out of
    the shard and put back twice, 37 frames apart, behind frame 8192 * 256."""
    base = synth.synth(M_DISTINCT, A, 40, seed)
    rng = np.random.RandomState(seed)
    ids = rng.randint(0, M_DISTINCT, n)
    if head:
        few = rng.choice(M_DISTINCT, 50, replace=False)
        ids[:head] = few[rng.randint(0, 50, head)]
    if fold_k:
        assert n >= FOLD + 256 and 5 * fold_k <= 256
        ids[5 * np.arange(fold_k)] = _fit_of_distinct(base, ids[0], fold_k)
        ids[FOLD:FOLD + 256] = ids[:256]
    if tail_k:
        t0 = 8192 * 256
        ctr = _fit_of_distinct(base, ids[0], tail_k)
        moved = ctr[1::2]
        assert n - t0 >= 80 * len(moved) + 40
        gone = np.isin(ids, moved)
        ids[gone] = rng.choice(np.setdiff1d(np.arange(M_DISTINCT), ctr), int(gone.sum()))
        for j, cid in enumerate(moved):
            ids[t0 + 80 * j + 3] = ids[t0 + 80 * j + 40] = cid
    return base, ids


class _Case:
    """frames, their oracle fit and their store, made once"""

    def __init__(self, family, n, A, K, seed):
        from oracle import cluster as oc
        from oracle import qcp
        self.family, self.n, self.A, self.K = family, n, A, K
        self.ids = None
        if family == "walk":
            self.x = synth.walk(n, A, seed)
        else:
            head = 0
            if family == "late":
                head = 300000 if n > 400000 else FOLD // 2
            base, self.ids = _draws(n, A, seed, head=head,
                                    fold_k=K if (family == "tiled" and n < 2 * FOLD) else 0,
                                    tail_k=K if family == "tail" else 0)
            self.head = head
            self.x = np.ascontiguousarray(base[self.ids])
        self.P = qcp.Prepared(self.x)
        self.oc = oc
        self.want = oc.kcenters(self.P, n_clusters=K)
        self._cut = None
        self._st = None

    @property
    def st(self):
        if self._st is None:
            from enspara_amd.device import FrameStore
            self._st = FrameStore.from_array(self.x)
        return self._st

    def close(self):
        if self._st is not None:
            self._st.close()

    def want_cut(self):
        """a cut-off 20 % above the K-center fit's last maximum: the stop rule ends the
        run before K centers, between two centers of the same oracle loop"""
        if self._cut is None:
            cut = float(self.want[2].max()) * 1.2
            self._cut = (cut, self.oc.kcenters(self.P, dist_cutoff=cut))
            assert 2 <= len(self._cut[1][0]) < self.K
        return self._cut

    def check_data(self):
        """the conditions that make the family a test, from the data and the oracle"""
        ctr = np.asarray(self.want[0], dtype=np.int64)
        assert len(ctr) == self.K and len(set(ctr.tolist())) == self.K
        if self.family == "walk":
            # all distinct: no two equal maxima, and the centers go deep into the shard
            assert ctr.max() >= self.n // 2, ctr.max()
            return
        ids = self.ids
        present, at = np.unique(ids, return_index=True)
        assert len(present) == M_DISTINCT
        first = at.astype(np.int64)
        last = self.n - 1 - np.unique(ids[::-1], return_index=True)[1].astype(np.int64)
        # every center is the first of its bit-identical copies ...
        np.testing.assert_array_equal(first[ids[ctr]], ctr)
        if self.family == "tiled":
            # ... and has a copy a whole fold (1024 entries of 256 frames) further on:
            # the tie is inside one thread's strided share, not inside one workgroup
            assert (last[ids[ctr]] - ctr >= FOLD).all(), (ctr, last[ids[ctr]])
        elif self.family == "tail":
            # half the centers but one are behind block maximum 8192, each with its copy
            # in the tail as well
            assert int((ctr >= 8192 * 256).sum()) == self.K // 2, ctr
        else:
            # late: the centers lie behind the head
            deep = FOLD if self.n > 400000 else FOLD // 2
            assert 2 * int((ctr >= deep).sum()) >= self.K, ctr


SEEDS = {"tiled": 11, "late": 23, "walk": 37, "tail": 53}
SHAPES = {          # (family, n): (A, K)
    ("tiled", 262401): (4, 32), ("late", 262401): (5, 24), ("walk", 262401): (5, 24),
    ("tiled", 524160): (4, 24), ("tiled", 524161): (4, 24),
    ("tiled", 524288): (5, 24),
    ("tiled", 524289): (5, 32), ("late", 524289): (4, 24), ("walk", 524289): (3, 24),
    ("tiled", 1048320): (4, 24), ("tiled", 1048321): (4, 24),
    ("tiled", 2098177): (3, 24), ("late", 2098177): (3, 24), ("walk", 2098177): (3, 24),
    ("tail", 2098177): (3, 24),
}


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(family, n):
        if (family, n) not in made:
            A, K = SHAPES[(family, n)]
            made[(family, n)] = _Case(family, n, A, K, SEEDS[family] + n % 1000)
        return made[(family, n)]

    yield get
    for c in made.values():
        c.close()


# ---- runs -----------------------------------------------------------------------------------
def _set(st, **opts):
    o = dict(DEFAULTS)
    o.update(opts)
    for k, v in o.items():
        if k == "fpl":
            st.set_frames_per_lane(v)
        else:
            st.set_option(k, v)
    return o


def _expected_form(n, A, o):
    """what last_run_form() must say: the thresholds, restated"""
    nb = -(-n // 256)
    fpl = o["fpl"] or (4 if n >= 1048321 else (2 if n >= 524161 else 1))
    fused = bool(o["fused_rounds"] and o["chained"])
    T = 16 if o["candidates"] == -1 else o["candidates"]
    if T == 32 and not fused:
        T = 16
    sweep = fused and T == 16 and (o["pass_sweep"] == 2 or
                                   (o["pass_sweep"] == 1 and n <= 524288))
    fine = fused and T > 1 and bool(o["fine_pick"]) and 4 * nb <= 8192
    nt = o["nontemporal"]
    if nt < 0:
        nt = 1 if nb * 3 * A * 256 * 4 > (192 << 20) else 0
    return {"frames_per_lane": fpl, "nontemporal": nt, "sweep_in_pass": int(sweep),
            "fine_pick": int(fine), "coarse_entries": nb,
            "pick_entries": (4 * nb if fine else nb) if T > 1 else -(-n // (256 * fpl))}


def _same(got, want):
    idx, d, a = got
    assert [int(i) for i in idx] == [int(i) for i in want[0]]
    np.testing.assert_array_equal(a, want[1])
    np.testing.assert_array_equal(d.view(np.uint32),
                                  want[2].astype(np.float32).view(np.uint32))


def _fit(c, cutoff=0.0, max_new=None, **opts):
    """one fit on the case's store -> ((center indices, distances, labels), form)"""
    st = c.st
    o = _set(st, **opts)
    st.reset_state()
    idx, _, _ = st.kcenters_run(0, c.K if max_new is None else max_new, cutoff)
    d, a = st.download_state()
    form = st.last_run_form()
    assert form == _expected_form(c.n, c.A, o), (opts, form)
    return (idx, d, a), form


# the matrix of test_candidates_per_pass_do_not_change_results,
# test_per_prefix_maxima_in_the_pass_or_in_the_chain_kernel and test_gpu_active_view.py
FULL = ([dict()] +
        [dict(candidates=t) for t in (1, 8, 16, 32)] +
        [dict(candidates=t, chained=0) for t in (8, 16, -1)] +
        [dict(candidates=t, fused_rounds=0) for t in (8, 16, 32, -1)] +
        [dict(candidates=t, pass_sweep=s) for t in (16, -1) for s in (0, 2)] +
        [dict(candidates=t, fine_pick=0) for t in (16, -1)] +
        [dict(candidates=t, fpl=f) for t in (1, -1) for f in (1, 2, 4)] +
        [dict(candidates=16, fused_rounds=0, fine_pick=0, pass_sweep=0, fpl=2)])
REDUCED = [dict(), dict(candidates=1), dict(candidates=16), dict(candidates=32),
           dict(candidates=16, fused_rounds=0), dict(candidates=8, chained=0),
           dict(candidates=16, pass_sweep=0), dict(candidates=16, pass_sweep=2),
           dict(candidates=16, fine_pick=0)]


def _far_side(n, form, opts):
    """the form a size is in the file for, under automatic options"""
    if n > FOLD:
        assert form["coarse_entries"] > 1024
    if n == 2098177:
        assert form["coarse_entries"] == 8197
        if opts.get("candidates", -1) != 1:
            # the tail of ek_pick_top_body: more entries than 8 per thread
            assert form["pick_entries"] == 8197 and form["fine_pick"] == 0


@pytest.mark.parametrize("family,n", [("tiled", 262401), ("tiled", 524289),
                                      ("tiled", 2098177), ("tail", 2098177)])
def test_every_form_on_tied_maxima(cases, family, n):
    c = cases(family, n)
    c.check_data()
    for opts in FULL:
        got, form = _fit(c, **opts)
        _same(got, c.want)
        _far_side(n, form, opts)
    if n == 524289:     # non-temporal loads by option, at one size
        for nt in (0, 1):
            for t in (1, 16):
                got, form = _fit(c, candidates=t, nontemporal=nt)
                _same(got, c.want)
                assert form["nontemporal"] == nt


@pytest.mark.parametrize("family,n", [("late", 262401), ("walk", 262401),
                                      ("late", 524289), ("walk", 524289),
                                      ("late", 2098177), ("walk", 2098177)])
def test_centers_deep_in_the_shard(cases, family, n):
    c = cases(family, n)
    c.check_data()
    for opts in REDUCED:
        got, form = _fit(c, **opts)
        _same(got, c.want)
        _far_side(n, form, opts)


@pytest.mark.parametrize("lo,hi,what", [(524160, 524161, "frames_per_lane"),
                                        (524288, 524289, "fine_and_sweep"),
                                        (1048320, 1048321, "frames_per_lane")])
def test_both_sides_of_a_threshold(cases, lo, hi, what):
    """automatic options on both sides, then every single forced flip"""
    auto = {}
    for n in (lo, hi):
        c = cases("tiled", n)
        c.check_data()
        for cands in (-1, 16, 1):
            got, form = _fit(c, candidates=cands)
            _same(got, c.want)
            auto[(n, cands)] = form
    if what == "frames_per_lane":
        below, above = (1, 2) if lo < 600000 else (2, 4)
        for cands in (-1, 16, 1):
            assert auto[(lo, cands)]["frames_per_lane"] == below
            assert auto[(hi, cands)]["frames_per_lane"] == above
        # the one-center pick's list: 256 x frames-per-lane frames an entry
        assert auto[(lo, 1)]["pick_entries"] == -(-lo // (256 * below))
        assert auto[(hi, 1)]["pick_entries"] == -(-hi // (256 * above))
        flips = [dict(fpl=f, candidates=t) for f in (1, 2, 4) for t in (1, -1)]
    else:
        assert auto[(lo, 16)]["fine_pick"] == 1 and auto[(hi, 16)]["fine_pick"] == 0
        assert auto[(lo, 16)]["sweep_in_pass"] == 1 and auto[(hi, 16)]["sweep_in_pass"] == 0
        assert auto[(lo, 16)]["pick_entries"] == 8192 and auto[(hi, 16)]["pick_entries"] == 2049
        assert auto[(lo, -1)]["fine_pick"] == 1 and auto[(hi, -1)]["fine_pick"] == 0
        flips = [dict(candidates=16, pass_sweep=0), dict(candidates=16, pass_sweep=2),
                 dict(candidates=16, fine_pick=0), dict(candidates=-1, fine_pick=0),
                 dict(candidates=-1, pass_sweep=2), dict(candidates=32)]
    for n in (lo, hi):
        c = cases("tiled", n)
        for opts in flips:
            got, _ = _fit(c, **opts)
            _same(got, c.want)


@pytest.mark.parametrize("family", ["tiled", "late"])
@pytest.mark.parametrize("n", [262401, 524289])
def test_active_view(cases, family, n):
    """the view's select (ek_view_count / scan / write kernels) over 257 and 513 counts:
    more than one count per thread of the scan, offsets across its waves"""
    c = cases(family, n)
    c.check_data()
    assert -(-n // 1024) > 256
    for view in (0, 1, 2):
        for cands in (16, 8, -1, 1):
            got, _ = _fit(c, candidates=cands, active_view=view)
            _same(got, c.want)
            vs = c.st.view_stats()
            if view == 0 or cands == 1:     # (key 4 = 1: the plain loop, which has no view)
                assert vs["views"] == 0 and vs["left_out"] == 0, (view, cands, vs)
            elif view == 2:
                assert vs["views"] > 0 and vs["left_out"] > 0, (cands, vs)


@pytest.mark.parametrize("family", ["tiled", "walk"])
def test_view_layout(cases, family):
    """ek_view_layout_check at 262 401 frames: more than 65 536 frames active, and one to
    three frames in the view's last group of four"""
    c = cases(family, 262401)
    got, _ = _fit(c)
    d = got[1]
    sd = np.sort(d)
    theta = None
    for cnt in range(c.n // 2, 65536, -1):      # frames strictly above theta
        if cnt % 4 and sd[c.n - cnt - 1] < sd[c.n - cnt]:
            theta = float(sd[c.n - cnt - 1])
            break
    assert theta is not None
    want = int((d > np.float32(theta)).sum())
    assert want > 65536 and want % 4 != 0
    for cands in (16, 8):       # with and without a quad copy to build from
        _fit(c, candidates=cands)
        frames, dq, dt, da = c.st.view_layout_check(theta)
        assert frames == want
        assert (dq, dt, da) == (0, 0, 0)


def test_triangle_inequality(cases):
    """time-ordered frames at 262 401: tiles are left out, one center per pass and in
    rounds, and nothing changes"""
    c = cases("walk", 262401)
    for cands in (1, 16, -1):
        got, _ = _fit(c, candidates=cands, triangle=1)
        _same(got, c.want)
        tiles, skipped = c.st.ti_stats()
        assert tiles > 0 and skipped > 0, (cands, tiles, skipped)


@pytest.mark.parametrize("family,n", [("tiled", 2098177), ("late", 524289),
                                      ("walk", 262401), ("tail", 2098177)])
def test_cutoff_stops_on_the_far_side(cases, family, n):
    c = cases(family, n)
    cut, want = c.want_cut()
    for opts in (dict(), dict(candidates=1), dict(candidates=16),
                 dict(candidates=16, fused_rounds=0), dict(candidates=8, chained=0)):
        got, form = _fit(c, cutoff=cut, max_new=c.K + 8, **opts)
        _same(got, want)
        _far_side(n, form, opts)


def test_continuation_past_8192_entries(cases):
    c = cases("tail", 2098177)
    st = c.st
    k1 = 11
    for cands in (-1, 16, 1):
        o = _set(st, candidates=cands)
        st.reset_state()
        i1, _, _ = st.kcenters_run(0, k1, 0.0)
        i2, _, _ = st.kcenters_run(k1, c.K - k1, 0.0)
        d, a = st.download_state()
        assert st.last_run_form() == _expected_form(c.n, c.A, o)
        _same((list(i1) + list(i2), d, a), c.want)


def test_one_pam_sweep_on_tied_proposals():
    """hybrid(..., n_iters=1) as test_one_pam_sweep, on tiled data at 300 001 x 4, K = 12:
    clusters of more than 32 768 members (numpy's pairwise summation goes deeper than in
    any other sweep of the suite), and proposals with bit-identical copies, which put
    equal costs in front of the strict <"""
    from enspara_amd.cluster import kcenters as kc
    from enspara_amd.cluster import kmedoids as km
    from enspara_amd.device import FrameStore
    from oracle import cluster as oc
    from oracle import qcp
    n, A, K = 300001, 4, 12
    base, ids = _draws(n, A, 5)
    x = np.ascontiguousarray(base[ids])
    P = qcp.Prepared(x)
    inds, a, d = oc.kcenters(P, n_clusters=K)
    med, wd, wa = oc.pam_update(P, list(inds), a, d, random_state=np.random.RandomState(3))
    assert sum(int(p) != int(q) for p, q in zip(med, inds)) >= 1
    assert np.bincount(wa, minlength=K).max() > 32768
    assert np.bincount(a, minlength=K).max() > 32768
    with FrameStore.from_array(x) as st:
        r = kc._kcenters_device(x, K, 0, None, 0, store=st)
        assert list(r.center_indices) == [int(i) for i in inds]
        r = km._kmedoids_iterations_device(x, st, 1, r.center_indices, None,
                                           np.random.RandomState(3))
    assert list(r.center_indices) == [int(i) for i in med]
    np.testing.assert_array_equal(r.assignments, wa)
    np.testing.assert_array_equal(r.distances.astype(np.float32).view(np.uint32),
                                  wd.astype(np.float32).view(np.uint32))
