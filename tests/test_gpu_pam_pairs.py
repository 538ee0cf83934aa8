"""The distance kernels of a large shard's PAM window, where they actually run.

Part 1 -- ek_pam_pairs_kernel<0/1> (LDS slices of 48 atoms) and ek_pam_pairs16_kernel<0/1>
(matrix cores: trips of 4 atoms, a load ring of 8 trips) through ek_pam_pairs_probe, which
calls the launchers the sweep calls.  Every expected distance is
oracle.qcp.rmsd_centered of the same centred arrays, compared as float32 bits; dmin is
the float32 minimum over each group of 8 live columns; in bounds mode T = max(O - dprop,
0) in float32; in list mode every entry the list does not name still holds the caller's
NaN pattern.  No expected value comes from a device call.  Both forms run everywhere.
One dimension is swept at a time against two fixed settings of the others (BASES).

Part 2 -- whole sweeps at the size where ek_pam_prefetch_vectors first takes that form
(16384 frames, K well above 128: 512), one per class of atom count, against
oracle.cluster.pam_update: medoids, labels and distances (float32 bits).  Each case
first asserts, from the oracle's values alone, that its data can reach the form (the
listing rule restated in numpy leaves at most a fifth of the frames; the device's limit
is a quarter) and that the sweep decides something (accepts, rejects, moves a frame);
then that the device really took the form (restricted prefetches, windows in one
workgroup) and returns the oracle's state, also in three launches per proposal and with
the LDS-staged pairs kernels.
"""
import functools

import numpy as np
import pytest

import _pam_probe as pp
from _structure_cases import family_cases, structure_family

pytestmark = pytest.mark.gpu

FORMS = ((1, "mfma"), (0, "lds"))


# =============================================================================================
# Part 1: the pairs kernels alone
# =============================================================================================
@functools.lru_cache(maxsize=None)
def _random(n, A, seed):
    """centred structures and traces (shared, never written to)"""
    from oracle import qcp
    x = np.random.RandomState(1000 * seed + A).normal(size=(n, A, 3)).astype(np.float32)
    c, G = qcp.center_and_trace(x)
    c.setflags(write=False)
    G.setflags(write=False)
    return c, G


def _held_of(name, K, old_lo, n_old):
    """-1, 0, K - 1, the middle of the table, one of the old columns"""
    return {"none": -1, "first": 0, "last": K - 1, "middle": K // 2,
            "old": old_lo + n_old // 2 if n_old else K // 2}[name]


def _check_tables(A, K, n_col, old_lo, n_old, held, bounds=False, rows=None, cols=None):
    """one shape, both forms, exact tables or the bounds from O"""
    rc, rG = rows if rows is not None else _random(K + 1, A, 1)
    cc, cG = cols if cols is not None else _random(max(n_col, 1), A, 2)
    rc, rG, cc, cG = rc[:K + 1], rG[:K + 1], cc[:n_col], cG[:n_col]
    dprop = None
    if bounds:
        assert n_old == n_col
        # some bounds positive, some cut off at zero (the self-distance of an old
        # column's own medoid always is)
        _, O, _ = pp.want_tables(rc, rG, cc, cG, held, old_lo, n_old)
        dprop = (np.random.RandomState(K + n_col).uniform(0.0, 1.5, size=n_col) *
                 np.median(O)).astype(np.float32)
    wT, wO, wmin = pp.want_tables(rc, rG, cc, cG, held, old_lo, n_old, dprop)
    if bounds and K > 2 and rows is None:
        assert (wT == 0).any() and (wT > 0).any()
    for form, fname in FORMS:
        T, O, dmin = pp.tables(form, rc, rG, cc, cG, held, old_lo, n_old, dprop)
        what = "%s A=%d K=%d n_col=%d old=[%d,+%d) held=%d bounds=%d" % (
            fname, A, K, n_col, old_lo, n_old, held, bounds)
        pp.same_bits(O, wO, what + " O")
        pp.same_bits(T, wT, what + " T")
        pp.same_bits(dmin, wmin, what + " dmin")


# (K, n_col, old_lo, n_old, held by name): two settings every sweep below runs against
BASES = ((65, 17, 3, 9, "old"), (16, 8, 1, 15, "middle"))
ATOMS = (2, 3, 4, 5, 7, 31, 32, 33, 47, 48, 49, 63, 65, 97)
ROWS = (1, 15, 16, 17, 63, 64, 65, 130)
COLS = (1, 7, 8, 9, 15, 16, 17, 32)
# (A for the sweeps that do not sweep it: a last trip of one atom after a full ring of
# 32, a second LDS slice of one atom; and one short of a trip)
FIXED_A = (49, 7)


def _fit(K, old_lo, n_old):
    """the old columns of a base inside a table of K rows"""
    old_lo = min(old_lo, K - 1)
    return old_lo, min(n_old, K - old_lo)


@pytest.mark.parametrize("A", ATOMS)
def test_tables_atom_counts(A):
    """the trip of 4 (A mod 4 in 0..3, one live atom in the last trip), the ring of 32
    (31, 32, 33), the LDS slice of 48 (47, 48, 49, 97: a third slice of one atom)"""
    for K, n_col, old_lo, n_old, held in BASES:
        _check_tables(A, K, n_col, old_lo, n_old, _held_of(held, K, old_lo, n_old))
    K, n_col, old_lo, n_old, held = BASES[0]
    _check_tables(A, K, n_col, old_lo, n_col, _held_of(held, K, old_lo, n_col), bounds=True)


@pytest.mark.parametrize("K", ROWS)
def test_tables_rows(K):
    """a wave's 16 rows, a workgroup's 64, a second workgroup with dead waves"""
    for (_, n_col, old_lo, n_old, held), A in zip(BASES, FIXED_A):
        old_lo, n_old = _fit(K, old_lo, n_old)
        _check_tables(A, K, n_col, old_lo, n_old, _held_of(held, K, old_lo, n_old))
        old_lo, n_b = _fit(K, old_lo, n_col)
        _check_tables(A, K, n_b, old_lo, n_b, _held_of(held, K, old_lo, n_b), bounds=True)


@pytest.mark.parametrize("n_col", COLS)
def test_tables_columns(n_col):
    """the groups of 8 behind dmin, the 16 columns of a wave: proposals' columns, and
    proposals' and old medoids' together as the bounds mode has them"""
    for (K, _, old_lo, n_old, held), A in zip(BASES, FIXED_A):
        _check_tables(A, K, n_col, old_lo, n_old, _held_of(held, K, old_lo, n_old))
    K, _, old_lo, _, held = BASES[0]
    for A in FIXED_A:
        _check_tables(A, K, n_col, old_lo, n_col, _held_of(held, K, old_lo, n_col),
                      bounds=True)


@pytest.mark.parametrize("n_old", (0,) + COLS)
def test_tables_old_columns(n_old):
    """the old medoids' columns (rows of the table itself, one of them the held row)"""
    for (K, n_col, old_lo, _, held), A in zip(BASES, FIXED_A):
        lo, n = _fit(K, old_lo, n_old)
        _check_tables(A, K, n_col, lo, n, _held_of(held, K, lo, n))
    # old_lo = 0, and the old columns up to the table's last row
    K, n_col = 65, 9
    _check_tables(5, K, n_col, 0, min(n_old, K), -1)
    _check_tables(5, K, n_col, K - n_old, n_old, K - 1)


@pytest.mark.parametrize("held", ["none", "first", "last", "middle", "old"])
def test_tables_held_row(held):
    """the medoid a rejected proposal still occupies is read from row K: as a row, and
    as the old column old_lo + j == held"""
    for (K, n_col, old_lo, n_old, _), A in zip(BASES, FIXED_A):
        h = _held_of(held, K, old_lo, n_old)
        if held == "old":
            assert old_lo <= h < old_lo + n_old
        _check_tables(A, K, n_col, old_lo, n_old, h)
        _check_tables(A, K, n_col, old_lo, n_col, _held_of(held, K, old_lo, n_col),
                      bounds=True)


def test_tables_no_proposals_only_old_columns():
    """n_col = 0 without bounds: O alone, no dmin row exists"""
    for A in FIXED_A:
        _check_tables(A, 65, 0, 3, 9, 5)


# ---- list mode --------------------------------------------------------------------------
STORE = 300
LISTS = (1, 15, 16, 17, 63, 64, 65, 200)


def _check_listed(A, n_list, n_col, n_pad, seed=0, rows=None, cols=None):
    rc, rG = rows if rows is not None else _random(STORE, A, 3)
    cc, cG = cols if cols is not None else _random(32, A, 4)
    cc, cG = cc[:n_col], cG[:n_col]
    # without order, without repeats
    lst = np.random.RandomState(n_list + 7 * seed).permutation(len(rc))[:n_list]
    if n_list > 2:
        assert (np.diff(lst) < 0).any()
    want = pp.want_listed(rc, rG, cc, cG, lst, n_pad)
    assert (want.view(np.uint32) == pp.FILL).sum() == n_col * (n_pad - n_list)
    for form, fname in FORMS:
        got = pp.listed(form, rc, rG, cc, cG, lst, n_pad)
        pp.same_bits(got, want, "%s A=%d list of %d, %d columns, n_pad=%d" % (
            fname, A, n_list, n_col, n_pad))


@pytest.mark.parametrize("n_list", LISTS)
def test_list_lengths(n_list):
    """lists drawn without order from a store of 300 rows, vectors longer than the
    store: what the list names is the oracle's, everything else was left alone"""
    for A, n_col in zip(FIXED_A, (17, 8)):
        _check_listed(A, n_list, n_col, STORE + 20)


@pytest.mark.parametrize("A", ATOMS)
def test_list_atom_counts(A):
    for n_list, n_col in ((65, 17), (16, 8)):
        _check_listed(A, n_list, n_col, STORE + 4)


@pytest.mark.parametrize("n_col", COLS)
def test_list_columns(n_col):
    for A, n_list in zip(FIXED_A, (65, 17)):
        _check_listed(A, n_list, n_col, STORE)


# ---- the structure families ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family(family, A):
    """70 rows; 20 columns, half of them rows of the same set (in no order: the
    self-distances are among the pairs), half from the family under another seed"""
    from oracle import qcp
    x = structure_family(family, 70, A)
    other = structure_family(family, 10, A, seed=1)
    own = np.random.RandomState(A).permutation(70)[:10]
    cols = np.concatenate([x[own], other])[np.random.RandomState(A + 1).permutation(20)]
    return qcp.center_and_trace(x), qcp.center_and_trace(np.ascontiguousarray(cols))


@pytest.mark.parametrize("family,A", family_cases())
def test_structure_families(family, A):
    """collinear, planar, mirrored, identical, rank-one and extreme-scale structures
    through the MFMA accumulation and the LDS slices: tables (69 medoids and the held
    one), the bounds from O, and a list of 41 of the 70 rows"""
    rows, cols = _family(family, A)
    assert np.isfinite(rows[0]).all() and np.isfinite(cols[0]).all()
    _check_tables(A, 69, 20, 40, 20, 47, rows=rows, cols=cols)
    _check_tables(A, 69, 20, 40, 20, 47, bounds=True, rows=rows, cols=cols)
    _check_listed(A, 41, 20, 72, rows=rows, cols=cols)


# =============================================================================================
# Part 2: whole sweeps where the restricted form begins
# =============================================================================================
N_BIG, K_BIG, WIN = 16384, 512, 32
# how far apart the two siblings of a template are drawn: close enough that proposals
# are accepted and frames change cluster, far enough (the bounds loosen with fewer
# atoms) that a window's proposals reach no more than a fifth of the frames
SPREAD = {3: 0.03, 4: 0.03, 5: 0.03, 7: 0.03, 16: 0.012,
          31: 0.006, 33: 0.006, 49: 0.006, 65: 0.006, 67: 0.006}
SEED = 11       # of the sweeps' draws


@functools.lru_cache(maxsize=None)
def _big(A, n=N_BIG, crowd=0):
    """256 templates, each split into two siblings, frames scattered 0.01 around the 512
    in no order; crowd > 0: that many of the frames, frame 0 among them and half again
    as far out as the others, around ONE sibling.  -> frames, Prepared, the oracle's k-centers to 512 (shared, not written to)"""
    from oracle import cluster as oc
    from oracle import qcp
    rng = np.random.RandomState(100 + A)
    tmpl = rng.normal(size=(K_BIG // 2, A, 3))
    sib = np.concatenate([tmpl + rng.normal(scale=SPREAD[A], size=tmpl.shape),
                          tmpl + rng.normal(scale=SPREAD[A], size=tmpl.shape)])
    labels = rng.permutation(np.arange(n) % K_BIG)
    if crowd:
        labels[rng.permutation(n)[:crowd]] = labels[0]
    noise = rng.normal(scale=0.01, size=(n, A, 3))
    if crowd:
        noise[0] *= 1.5         # k-centers starts from frame 0: the crowd's medoid is an outlier
    x = (sib[labels] + noise).astype(np.float32)
    x.setflags(write=False)
    P = qcp.Prepared(x)
    inds, a, d = oc.kcenters(P, n_clusters=K_BIG)
    a.setflags(write=False)
    d.setflags(write=False)
    return x, P, tuple(int(i) for i in inds), a, d


def _members_drawn(a, rs, upto):
    """kmedoids.py:514 for clusters [0, upto) of the state `a`"""
    return [int(rs.choice(np.flatnonzero(a == cid))) for cid in range(upto)]


@functools.lru_cache(maxsize=None)
def _explicit(A):
    """explicit proposals: one member of every cluster of the opening state (a window
    of proposals from anywhere reaches more than a quarter of the frames)"""
    _, _, _, a, _ = _big(A)
    return tuple(_members_drawn(a, np.random.RandomState(A), K_BIG))


@functools.lru_cache(maxsize=None)
def _oracle_sweeps(A, explicit, n_sweeps, n=N_BIG, crowd=0):
    """oracle.cluster.pam_update n_sweeps times, the draws going on from sweep to sweep
    -> (medoids, distances, labels) after each"""
    from oracle import cluster as oc
    _, P, inds, a, d = _big(A, n, crowd)
    props = list(_explicit(A)) if explicit else None
    rs = np.random.RandomState(SEED)
    out, state = [], (list(inds), d, a)
    for _ in range(n_sweeps):
        state = oc.pam_update(P, state[0], state[2], state[1], proposals=props,
                              random_state=rs)
        out.append(state)
    return out


def _listed_share(P, inds, a, d, props, bounds):
    """the share of the frames ek_pam_active_kernel lists for the first window on the
    opening state: a frame of the window's own clusters, or one whose medoid is not
    farther from every proposal than 2 d 1.001f + 1e-3f (float32, as the kernel
    evaluates it); the proposal-to-medoid table exact, or the lower bounds from the
    medoid-to-medoid table"""
    from oracle import qcp
    inds = np.asarray(inds, dtype=np.int64)
    med, med_G = np.ascontiguousarray(P.c[inds]), np.ascontiguousarray(P.G[inds])
    d32 = d.astype(np.float32)
    T = np.empty((WIN, len(inds)), dtype=np.float32)
    for j in range(WIN):
        if bounds:
            T[j] = np.maximum(qcp.rmsd_centered(med, med_G, med[j], med_G[j]) -
                              d32[props[j]], np.float32(0))
        else:
            T[j] = qcp.rmsd_centered(med, med_G, P.c[props[j]], P.G[props[j]])
    reach = np.float32(2) * d32 * np.float32(1.001) + np.float32(1e-3)
    assert reach.dtype == np.float32
    listed = (a < WIN) | ~(T.min(axis=0)[a] > reach)
    return float(listed.mean())


def _conditions(A, explicit, n=N_BIG, crowd=0, limit=0.20, need_moved=True):
    """what the data must be for the case to test anything, from the oracle alone"""
    _, P, inds, a, d = _big(A, n, crowd)
    if explicit:
        shares = [_listed_share(P, inds, a, d, _explicit(A), False)]
    else:
        props = _members_drawn(a, np.random.RandomState(SEED), WIN)
        shares = [_listed_share(P, inds, a, d, props, b) for b in (False, True)]
    wi, wd, wa = _oracle_sweeps(A, explicit, 1, n, crowd)[0]
    accepted = sum(int(i) != j for i, j in zip(wi, inds))
    moved = int((wa != a).sum())
    print("A=%d explicit=%d n=%d crowd=%d: listed share %s, accepted %d of %d, labels "
          "changed %d" % (A, explicit, n, crowd, ["%.4f" % s for s in shares], accepted,
                          K_BIG, moved))
    assert max(shares) <= limit
    assert 1 <= accepted < K_BIG
    assert moved >= 1 or not need_moved


def _device_sweeps(x, inds, props, n_sweeps, mfma, one_wg):
    """k-centers to the oracle's medoids, then the sweeps on one store -> (medoids,
    distances, labels, restricted prefetches, windows in one workgroup, ended early)"""
    from enspara_amd.cluster import kmedoids as km
    from enspara_amd.device import FrameStore
    with FrameStore.from_array(x) as st:
        try:
            # (process-wide: always said, and put back)
            st.set_option("pam_pairs_mfma", mfma)
            st.set_option("pam_one_workgroup", one_wg)
            st.reset_state()
            idx, _, _ = st.kcenters_run(0, len(inds), 0.0)
            assert [int(i) for i in idx] == list(inds)
            r = km._kmedoids_iterations_device(x, st, n_sweeps, list(inds), props,
                                               np.random.RandomState(SEED))
            restricted, _ = st.pam_prefetch_passes()
            windows, early = st.pam_sparse_stats()
        finally:
            st.set_option("pam_pairs_mfma", 1)
    return r, restricted, windows, early


def _assert_state(r, want, what):
    wi, wd, wa = want
    assert list(r.center_indices) == [int(i) for i in wi], what
    np.testing.assert_array_equal(r.assignments, wa, err_msg=what)
    np.testing.assert_array_equal(r.distances.astype(np.float32).view(np.uint32),
                                  wd.astype(np.float32).view(np.uint32), err_msg=what)


def _check_sweeps(A, explicit, n_sweeps, n=N_BIG, crowd=0):
    x, _, inds, _, _ = _big(A, n, crowd)
    want = _oracle_sweeps(A, explicit, n_sweeps, n, crowd)[-1]
    props = list(_explicit(A)) if explicit else None
    out = {}
    for mfma, one_wg in ((1, 1), (1, 0), (0, 1)):
        r, restricted, windows, early = _device_sweeps(x, inds, props, n_sweeps, mfma,
                                                       one_wg)
        what = "A=%d pam_pairs_mfma=%d pam_one_workgroup=%d" % (A, mfma, one_wg)
        _assert_state(r, want, what)
        assert restricted >= 1, what
        if one_wg:
            assert windows >= 1, what
        else:
            assert windows == 0, what
        out[mfma, one_wg] = (restricted, windows, early)
    return out


SWEEP_CASES = ([(A, False, 1) for A in (3, 4, 5, 7, 16, 31, 33, 49, 65, 67)] +
               [(A, True, 1) for A in (5, 33, 65)] + [(A, False, 2) for A in (5, 33)])


@pytest.mark.parametrize("A,explicit,n_sweeps", SWEEP_CASES)
def test_sweeps_at_the_threshold(A, explicit, n_sweeps):
    """16384 frames, 512 medoids: tables, list, listed distances and the window in one
    workgroup, at every class of atom count (remainders mod 4, a second turn of the
    load ring at 33, a second LDS slice at 49, a second slice of the one-workgroup
    search at 65 and 67); explicit proposals give exact tables and no bounds; a second
    sweep opens on the state PAM left"""
    _conditions(A, explicit)
    _check_sweeps(A, explicit, n_sweeps)


def test_sweep_below_the_threshold():
    """one frame fewer: the same data rule, the streaming form, the same equality"""
    A, n = 5, N_BIG - 1
    x, _, inds, _, _ = _big(A, n)
    want = _oracle_sweeps(A, False, 1, n)[-1]
    assert sum(int(i) != j for i, j in zip(want[0], inds)) >= 1
    for mfma, one_wg in ((1, 1), (0, 0)):
        r, restricted, windows, _ = _device_sweeps(x, inds, None, 1, mfma, one_wg)
        _assert_state(r, want, "n=%d" % n)
        assert restricted == 0 and windows == 0


CROWD = 2550


def test_sweep_window_hands_back_a_proposal_that_changes_too_many_frames():
    """One cluster of about 2600 members, cluster 0 (3000 would put the first window's
    list over the quarter at which the device gives the form up): its proposal brings
    2543 frames closer, more than
    EK_SP_CAP_CHG = 2048 frames closer and is accepted (the oracle's first proposal
    alone says so).  The one-workgroup window cannot hold that many changes, ends early
    (counted) and the launches take the proposal: same state as the oracle's."""
    from oracle import cluster as oc
    A = 7
    x, P, inds, a, d = _big(A, N_BIG, CROWD)
    assert (a == 0).sum() > 2048
    # (the crowd alone is 0.16 of the frames and the window's other clusters 0.05: the
    # list cannot stay under a fifth here, only under the device's quarter; the crowd's
    # frames change distance, not label)
    _conditions(A, False, N_BIG, CROWD, limit=0.24, need_moved=False)
    wi, wd, _ = oc.pam_update(P, list(inds), a, d, stop_after=1,
                              random_state=np.random.RandomState(SEED))
    assert int(wi[0]) != inds[0], "the first proposal was not accepted"
    assert (wd < d).sum() > 2048
    out = _check_sweeps(A, False, 1, N_BIG, CROWD)
    for key in ((1, 1), (0, 1)):
        assert out[key][2] >= 1, "no window ended early"
