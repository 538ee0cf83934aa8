"""What tests/_tied_cases.py promises, asserted by the oracle alone (no device):
the layout against the shard bounds, and that the oracle's k-centers loop on
these frames really picks at tied maxima -- within shards and across shard
boundaries -- with centers in every shard.  A later change of the generator
cannot quietly remove the ties that tests/test_sharded_gloo.py and
tests/test_gpu_sharded_ties.py rely on."""
import numpy as np
import pytest

import _tied_cases as tc
from enspara_amd import sharded

SHAPES = [(tc.MAIN, tc.MAIN_K), (tc.TWO_SHARDS, tc.TWO_SHARDS_K),
          (tc.ONE_EMPTY, tc.ONE_EMPTY_K), (tc.EIGHT_SOME_EMPTY, tc.EIGHT_K)]


def test_shard_shapes():
    def counts(shape):
        return tuple(sharded.shard_bounds(shape[0], shape[3], r)[1]
                     for r in range(shape[3]))
    assert counts(tc.MAIN) == (768, 512, 257)
    assert counts(tc.TWO_SHARDS) == (512, 488)
    assert counts(tc.ONE_EMPTY) == (256, 244, 0)
    assert counts(tc.EIGHT_SOME_EMPTY) == (256, 256, 256, 256, 256, 120, 0, 0)


@pytest.mark.parametrize("shape,K", SHAPES)
def test_layout(shape, K):
    n, A, B, world, seed = shape
    x, ids = tc.tied_frames(n, A, B, world, seed)
    x2, ids2 = tc.tied_frames(n, A, B, world, seed)
    assert x.dtype == np.float32 and x.shape == (n, A, 3)
    np.testing.assert_array_equal(x, x2)            # seeded
    np.testing.assert_array_equal(ids, ids2)
    assert sorted(set(ids.tolist())) == list(range(B))
    # copies are bit-identical, distinct frames are not
    first = np.array([np.flatnonzero(ids == b)[0] for b in range(B)])
    np.testing.assert_array_equal(x, x[first][ids])
    flat = x[first].reshape(B, -1)
    assert len(np.unique(flat, axis=0)) == B
    live = tc.live_shards(n, world)
    held = [set(ids[lo:lo + cnt].tolist()) for _, lo, cnt in live]
    sp = tc.specials(n, B, world)
    everywhere = {b for b in range(B) if all(b in h for h in held)}
    not_in_first = {b for b in range(B) if b not in held[0]}
    only_last = {b for b in range(B) if not any(b in h for h in held[:-1])}
    # a third in every shard, a third absent from the first (but for the one
    # placed on its last frame), the rest in the last alone
    assert set(range(B // 3)) <= everywhere
    assert not_in_first == set(range(B // 3, B)) - {sp["last_id"]}
    if len(live) >= 3:
        assert only_last == set(range(2 * B // 3, B))
    # which shard holds a distinct frame's first copy varies: every one does
    first_in = tc.shard_of(n, world, first)
    assert set(first_in.tolist()) == {r for r, _, _ in live}
    # the three placed by hand
    lo1 = live[1][1]
    assert sp["last_pos"] == lo1 - 1 and sp["first_pos"] == lo1
    assert first[sp["last_id"]] == sp["last_pos"]
    assert first[sp["first_id"]] == sp["first_pos"]
    assert np.count_nonzero(ids == sp["last_id"]) > 1
    assert np.count_nonzero(ids == sp["first_id"]) > 1
    tail = np.flatnonzero(ids == sp["tail_id"])
    assert len(tail) and tail.min() >= (n - 1) // 256 * 256 and n % 256 != 0
    np.testing.assert_array_equal(tail, sp["tail_pos"])


@pytest.mark.parametrize("shape,K", SHAPES)
def test_the_oracle_picks_at_tied_maxima(shape, K):
    from oracle import cluster as oc
    n, A, B, world, seed = shape
    x, ids = tc.tied_frames(n, A, B, world, seed)
    c = tc.tie_census(x, K, world)
    inds, _, _ = oc.kcenters(x, n_clusters=K)
    assert [int(i) for i in inds] == c.centers and len(set(c.centers)) == K
    tied = int(np.count_nonzero(c.n_tied > 1))
    cross = int(np.count_nonzero(c.cross))
    assert 2 * tied >= K, (tied, K)
    assert 4 * cross >= K, (cross, K)
    # ... and not the trivial ties of an all-zero state
    assert np.all(c.maxima[c.cross][: K // 4] > 1e-3)
    own = tc.shard_of(n, world, c.centers)
    live = [r for r, _, _ in tc.live_shards(n, world)]
    assert set(own.tolist()) == set(live), np.bincount(own, minlength=world)
    # every center is the first of its copies
    for i in c.centers:
        assert int(np.flatnonzero(ids == ids[i])[0]) == i
    later = sum(bool(np.any(tc.shard_of(n, world, np.flatnonzero(ids == ids[i])) > s))
                for i, s in zip(c.centers, own))
    assert 3 * later >= K, (later, K)


def test_main_shape_is_what_the_sharded_tests_were_sized_for():
    """the figures the GPU and gloo tests were chosen by: nearly every step tied,
    most of them across shards; more centers than distinct frames goes on with
    repeats of frames that are centers already"""
    from oracle import cluster as oc
    n, A, B, world, seed = tc.MAIN
    x, ids = tc.tied_frames(n, A, B, world, seed)
    c = tc.tie_census(x, tc.MAIN_K, world)
    assert np.count_nonzero(c.n_tied > 1) >= 36 and np.count_nonzero(c.cross) >= 20
    inds, a, d = oc.kcenters(x, n_clusters=tc.MORE_THAN_DISTINCT_K)
    assert len(inds) == tc.MORE_THAN_DISTINCT_K
    assert len(set(ids[[int(i) for i in inds]].tolist())) == B
    # two PAM sweeps on tied data move medoids
    rs = np.random.RandomState(5)
    inds, a, d = oc.kcenters(x, n_clusters=tc.MAIN_K)
    moved = []
    for _ in range(2):
        ni, d, a = oc.pam_update(x, inds, a, d, random_state=rs)
        moved.append(sum(int(p) != int(q) for p, q in zip(ni, inds)))
        inds = ni
    assert moved[0] > 0


@pytest.mark.parametrize("shape,K", SHAPES)
def test_tied_cutoff_stops_the_oracle_exactly_there(shape, K):
    from oracle import cluster as oc
    n, A, B, world, seed = shape
    x, _ = tc.tied_frames(n, A, B, world, seed)
    cutoff, k = tc.tied_cutoff(x, K, world)
    assert cutoff == float(np.float32(cutoff)) and cutoff > 1e-3
    inds, a, d = oc.kcenters(x, dist_cutoff=cutoff)
    assert len(inds) == k and d.max() == cutoff
    assert np.count_nonzero(d == cutoff) > 1
    # a hair below: the fit goes on
    more, _, _ = oc.kcenters(x, dist_cutoff=float(np.nextafter(np.float32(cutoff),
                                                               np.float32(0))))
    assert len(more) > k
