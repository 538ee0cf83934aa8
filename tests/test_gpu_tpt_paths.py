"""enspara_amd.tpt.path on the device (csrc/ek_tpt_path.hip): paths and fluxes are held
to the real reference's (tests/golden/tpt_paths_golden.npz) and to the numpy restatement
(tests/_numpy_tpt_paths.py, which tests/test_tpt_paths_host.py pins to the same goldens)
bit for bit: integers compared with array_equal, fluxes as bytes.  No expected value comes
from a device call, and nothing has a tolerance.

Shapes: the goldens (n = 2 to 300; ties at every pop; stars whose hub has 63, 64, 65 and
SEARCH_WG + 1 leaves; a path through all 300 states; 274 paths, more than one batch); 50
random graphs of n <= 60; rows whose degrees sit on both sides of the wave and the
workgroup; LDS_STATES and LDS_STATES + 1 states (the per-state arrays in the LDS, and in
global memory through the same code)."""
import gc
import os

import numpy as np
import pytest
import scipy.sparse

import _numpy_tpt as nt
import _numpy_tpt_paths as npp
from enspara_amd import _lib, tpt
from enspara_amd.tpt import path as tp

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "tpt_paths_golden.npz"))
CASES = [str(c) for c in G["cases"]]


def both_modes(c, F, **kw):
    for _, how in npp.MODES:
        got = tp.paths(c["src"], c["snk"], F, remove_path=how, num_paths=c["num_paths"],
                       flux_cutoff=c["cut"][how], **kw)
        npp.assert_same_paths(got, c["want"][how], how)


@pytest.mark.parametrize("name", CASES)
def test_golden(name):
    c = npp.golden_case(G, name)
    path, flux = tp.top_path(c["src"], c["snk"], c["F"])
    assert isinstance(flux, float)
    npp.assert_same_paths(([path], np.array([flux])), ([c["top"][0]], [c["top"][1]]), "top")
    both_modes(c, c["F"])


@pytest.mark.parametrize("name", CASES)
def test_golden_sparse_input(name):
    c = npp.golden_case(G, name)
    for kind in (scipy.sparse.csr_matrix, scipy.sparse.lil_matrix):
        S = kind(c["F"])
        path, flux = tp.top_path(c["src"], c["snk"], S)
        npp.assert_same_paths(([path], np.array([flux])), ([c["top"][0]], [c["top"][1]]),
                              "top")
        both_modes(c, S)


@pytest.mark.parametrize("caps", [(0, 3), (0, 7), (1, 0), (2, 11)])
def test_small_batches_change_nothing(caps):
    """a batch of a few nodes: a path that does not fit opens the next batch, and with 3
    nodes every batch is a single path"""
    for name in ("table6", "ties40", "ties40_np3", "ties40_cut", "chain300", "star65",
                 "flux17"):
        both_modes(npp.golden_case(G, name), npp.golden_case(G, name)["F"],
                   _batch_paths=caps[0], _batch_nodes=caps[1])


def random_problem(seed):
    rng = np.random.RandomState(1000 + seed)
    n = int(rng.randint(3, 61))
    kind = ('int', 'tenths', 'uniform')[seed % 3]
    density = (0.1, 0.3, 0.8)[(seed // 3) % 3]
    F = npp.random_fluxes(n, density, kind, seed)
    src = rng.randint(0, n, size=rng.randint(1, 4))
    snk = rng.randint(0, n, size=rng.randint(1, 4))
    return F, src, snk


def test_fifty_random_graphs_against_the_restatement():
    n_paths = 0
    for seed in range(50):
        F, src, snk = random_problem(seed)
        got = tp.top_path(src, snk, F)
        want = npp.top_path(src, snk, F)
        npp.assert_same_paths(([got[0]], np.array([got[1]])), ([want[0]], [want[1]]),
                              "seed %d top" % seed)
        for _, how in npp.MODES:
            want = npp.paths(src, snk, F, remove_path=how)
            npp.assert_same_paths(tp.paths(src, snk, F, remove_path=how), want,
                                  "seed %d %s" % (seed, how))
            n_paths += len(want[0])
    print("%d paths" % n_paths)
    assert n_paths > 500


def test_dense_and_sparse_input_agree():
    for seed in (1, 4, 8, 17, 30):
        F, src, snk = random_problem(seed)
        want = npp.paths(src, snk, F)
        for kind in (scipy.sparse.csr_matrix, scipy.sparse.csc_matrix, scipy.sparse.coo_matrix,
                     scipy.sparse.lil_matrix):
            npp.assert_same_paths(tp.paths(src, snk, kind(F)), want, kind.__name__)
        npp.assert_same_paths(tp.paths(src, snk, F), want, "dense")
    # stored zeros, negative entries and a cell given twice: the dense equivalent counts
    i = np.array([0, 0, 0, 1, 1, 2, 2, 3, 0])
    j = np.array([1, 2, 1, 3, 2, 3, 0, 0, 3])
    v = np.array([0.5, 1.0, 0.25, 2.0, 0.0, 1.0, -1.0, 3.0, -0.5])
    S = scipy.sparse.coo_matrix((v, (i, j)), shape=(4, 4))
    D = S.toarray()
    assert D[0, 1] == 0.75 and D[0, 3] == -0.5
    for how in ("subtract", "bottleneck"):
        want = npp.paths([0], [3], D, remove_path=how)
        assert [list(p) for p in want[0]] == [[0, 2, 3], [0, 1, 3]]
        npp.assert_same_paths(tp.paths([0], [3], S, remove_path=how), want, how)
        npp.assert_same_paths(tp.paths([0], [3], D, remove_path=how), want, how)


def test_row_degrees_around_the_wave_and_the_workgroup():
    """rows with 0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257 and 299 entries > 0 among
    negative ones, every one of them a source (so each is relaxed): the compaction's
    counts, its scan and its fill, and a relaxation wider than the workgroup"""
    n = 300
    rng = np.random.RandomState(7)
    degrees = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 299]
    F = -rng.rand(n, n) * (rng.rand(n, n) < 0.2)
    rows = np.arange(len(degrees)) * 20 + 3
    for r, d in zip(rows, degrees):
        cols = rng.permutation(np.delete(np.arange(n), r))[:d]
        F[r, :] = np.minimum(F[r, :], 0.0)
        F[r, cols] = rng.randint(1, 5, size=d)
    others = np.setdiff1d(np.arange(n), rows)
    for r in others:                    # a few edges out of everything else
        F[r, rng.randint(0, n, size=3)] = rng.randint(1, 5, size=3)
    np.fill_diagonal(F, 0.0)
    assert [(F[r] > 0).sum() for r in rows] == degrees
    snk = [int(others[-1]), int(others[5])]
    for src in (rows, rows[::-1]):
        got = tp.top_path(src, snk, F)
        want = npp.top_path(src, snk, F)
        npp.assert_same_paths(([got[0]], np.array([got[1]])), ([want[0]], [want[1]]), "top")
        for _, how in npp.MODES:
            want = npp.paths(src, snk, F, remove_path=how, num_paths=12)
            assert len(want[0]) == 12
            npp.assert_same_paths(tp.paths(src, snk, F, remove_path=how, num_paths=12), want,
                                  how)


@pytest.mark.parametrize("n", [tp.LDS_STATES, tp.LDS_STATES + 1])
def test_states_around_the_lds_constant(n):
    S = npp.sparse_fluxes(n, 4, seed=n)
    src, snk = [0, 5], [n - 1, n // 2]
    want = npp.paths(src, snk, S, num_paths=5, return_pops=True)
    want, want_pops = want[:2], want[2]
    assert len(want[0]) == 5 and min(want_pops) > 500
    npp.assert_same_paths(tp.paths(src, snk, S, num_paths=5), want, "n = %d" % n)
    F = tp._flux_matrix(S)
    with tp._Search(F, np.array(src, dtype=np.int32), np.array(snk, dtype=np.int32), 1, 1,
                    1.0, 1.0, 0) as search:
        found, _, done = search.next()
        (nnz, pops, n_paths, in_lds), _ = search.stats()
    assert done and n_paths == 1 and np.array_equal(found[0], want[0][0])
    assert nnz == F.nnz and in_lds == (n <= tp.LDS_STATES)
    assert pops == want_pops[0]


def test_callable_remove_path():
    def bottleneck(net_flux, path):
        out = net_flux.copy()
        k = out[path[:-1], path[1:]].argmin()
        out[path[k], path[k + 1]] = 0.0
        return out

    for name in ("table6", "ties40_np3", "flux17"):
        c = npp.golden_case(G, name)
        got = tp.paths(c["src"], c["snk"], c["F"], remove_path=bottleneck,
                       num_paths=c["num_paths"])
        npp.assert_same_paths(got, c["want"]["bottleneck"], name)
    F = npp.golden_case(G, "table6")["F"]
    before = F.copy()
    tp.paths([0], [4, 5], F, remove_path=bottleneck)
    tp.paths([0], [4, 5], F)
    assert np.array_equal(F, before)


def test_end_to_end_from_net_fluxes():
    tg = np.load(os.path.join(HERE, "golden", "tpt_golden.npz"))
    C = tg["C_n65"]
    T, pops = nt.tprob_from_counts(C), nt.pops_from_counts(C)
    src, snk = [0], [64]
    for Tin in (T, scipy.sparse.csr_matrix(T)):
        net = tpt.net_fluxes(Tin, src, snk, populations=pops)
        assert scipy.sparse.issparse(net) == scipy.sparse.issparse(Tin)
        for _, how in npp.MODES:
            want = npp.paths(src, snk, net, remove_path=how)
            assert len(want[0]) > 10
            npp.assert_same_paths(tp.paths(src, snk, net, remove_path=how), want, how)


# ---- what a call leaves behind on the device (the three properties of
# tests/test_gpu_lifetime.py) ---------------------------------------------------------------
def live():
    return tuple(_lib.live_resources())[:6]


def baseline():
    gc.collect()
    return live()


def _calls():
    c = npp.golden_case(G, "flux17")
    S = scipy.sparse.lil_matrix(c["F"])
    return [
        lambda: tp.paths(c["src"], c["snk"], c["F"]),
        lambda: tp.paths(c["src"], c["snk"], S, remove_path='bottleneck', _batch_nodes=5),
        lambda: tp.top_path(c["src"], c["snk"], c["F"]),
        lambda: tp.top_path(c["src"], c["snk"], S),
    ]


def _bytes(result):
    found, fluxes = result
    if isinstance(found, np.ndarray):       # top_path
        return found.tobytes() + np.float64(fluxes).tobytes()
    return b"".join(p.tobytes() for p in found) + fluxes.tobytes()


def test_resources_balance():
    for call in _calls():
        first = _bytes(call())                                  # warm-up
        before = baseline()
        for _ in range(3):
            assert _bytes(call()) == first
        assert live() == before


def test_resources_injected_allocation_failure():
    for call in _calls():
        want = _bytes(call())                                   # warm-up, the bytes to return
        base = baseline()
        failed = 0
        for k in range(64):
            assert _lib.fail_alloc_at(k) == -1
            try:
                got = _bytes(call())
            except _lib.HipError:
                got = None
            finally:
                pending = _lib.fail_alloc_at(-1)
            assert live() == base, "allocation %d" % k
            if got is not None:
                # the call made fewer than k + 1 allocations: the arm is still set
                assert pending >= 0 and got == want
                break
            assert pending == -1, "allocation %d: the arm is still set" % k
            failed += 1
        else:
            raise AssertionError("64 allocations failed one after the other")
        print("%d device allocations" % failed)
        assert 10 <= failed <= 20
        assert _bytes(call()) == want
