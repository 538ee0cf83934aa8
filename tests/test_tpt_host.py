"""enspara_amd.tpt without a device: the argument checks (they run before any
device call), and the numpy restatement the GPU tests lean on (tests/_numpy_tpt.py)
against the goldens made from the real reference (tests/golden/make_tpt_golden.py)
and against the known answers of the reference's own test_tpt_fluxes.py."""
import os

import numpy as np
import pytest
import scipy.sparse

import _numpy_tpt as nt
from enspara_amd import _lib
from enspara_amd.exception import DataInvalid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "tpt_golden.npz")

T3 = np.array([[0.5, 0.4, 0.1], [0.25, 0.5, 0.25], [0.1, 0.5, 0.4]])
T4 = np.array([[0.5, 0.4, 0.1, 0.], [0.25, 0.5, 0.2, 0.05], [0.1, 0.15, 0.5, 0.25],
               [0., 0.1, 0.4, 0.5]])
TFLUX = np.array([[0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
TCOUNTS = np.array([[2, 1, 1], [2, 1, 2], [3, 2, 1]])
MFPT_ALL = np.array([[0., 3.71428571, 3.5], [2.3125, 0., 3.], [2.125, 3.42857143, 0.]])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_package_surface():
    import enspara_amd.tpt as tpt
    assert sorted(tpt.__all__) == ["committors", "mfpts", "net_fluxes",
                                   "reactive_fluxes", "reactive_populations"]
    assert "top_path" in tpt.__doc__ and not hasattr(tpt, "paths")
    from enspara_amd.tpt import core
    assert core.LU_PANEL == 64


@pytest.mark.parametrize("call", [
    lambda t: t.committors(np.zeros((3, 4)), 0, 2),
    lambda t: t.committors(np.zeros(3), 0, 2),
    lambda t: t.committors(np.full((3, 3), np.nan), 0, 2),
    lambda t: t.committors(T3, [], 2),
    lambda t: t.committors(T3, 0, []),
    lambda t: t.committors(T3, 0, 3),
    lambda t: t.committors(T3, -1, 2),
    lambda t: t.committors(T3, [0, 1], [1, 2]),
    lambda t: t.committors(scipy.sparse.csr_matrix(T3), 0, 5),
    lambda t: t.mfpts(np.zeros((2, 3))),
    lambda t: t.mfpts(T3, sinks=[3]),
    lambda t: t.mfpts(T3, sinks=[]),
    lambda t: t.mfpts(T3, populations=np.ones(4) / 4),
    lambda t: t.mfpts(T3, populations=np.array([np.inf, 0, 0])),
    lambda t: t.reactive_fluxes(T3, 0, 0, populations=np.ones(3) / 3),
    lambda t: t.net_fluxes(T3, 0, 7, populations=np.ones(3) / 3),
    lambda t: t.reactive_populations(np.inf * T3, 0, 2, populations=np.ones(3) / 3),
    lambda t: t.core._solve(np.zeros((3, 2)), np.zeros(3)),
    lambda t: t.core._solve(np.eye(3), np.zeros((3, 4))),
    lambda t: t.core._solve(np.eye(3), np.array([0, np.nan, 0])),
])
def test_argument_errors_raise_before_any_device_call(call):
    import enspara_amd.tpt as tpt
    with pytest.raises(DataInvalid):
        call(tpt)


def test_c_abi_argument_errors():
    L = _lib.load()
    assert L.ek_tpt_committors(0, 0, None, None, 0, None, 0, None, None) == _lib.EK_EARG
    assert L.ek_tpt_mfpts_all(0, 3, None, None, 1.0, None, None) == _lib.EK_EARG
    assert L.ek_lu_solve(0, 3, None, 1, None, None, None, None) == _lib.EK_EARG
    T = np.ascontiguousarray(T3)
    q = np.zeros(3)
    info = np.zeros(1, dtype=np.int32)
    both = np.array([1], dtype=np.int32)
    assert L.ek_tpt_committors(0, 3, _lib.f64p(T), _lib.i32p(both), 1, _lib.i32p(both), 1,
                               _lib.f64p(q), _lib.i32p(info)) == _lib.EK_EARG
    assert b"both source and sink" in L.ek_last_error()
    far = np.array([3], dtype=np.int32)
    assert L.ek_tpt_mfpts_sinks(0, 3, _lib.f64p(T), _lib.i32p(far), 1, 1.0, _lib.f64p(q),
                                _lib.i32p(info)) == _lib.EK_EARG


# ---- the restatement against the reference's own known answers --------------------------
def test_restatement_committors_known_answers():
    for src, snk in ((0, 2), ([0], [2])):
        np.testing.assert_allclose(nt.committors(T3, src, snk), [0, 0.5, 1.], atol=1e-15)
    assert np.array_equal(np.around(nt.committors(T4, 0, 3), 5), [0, 0.34091, 0.60227, 1.])
    np.testing.assert_allclose(nt.committors(T4, [0, 2], [3]), [0, 0.1, 0, 1.], atol=1e-15)


def test_restatement_mfpts_known_answers():
    T = TCOUNTS / TCOUNTS.sum(axis=1)[:, None]
    # (the stationary distribution, by the restatement's own solver)
    A = np.vstack([(T.T - np.eye(3))[:2], np.ones(3)])
    pops = nt.solve(A, np.array([0., 0., 1.]))
    np.testing.assert_allclose(pops @ T, pops, atol=1e-15)
    np.testing.assert_array_almost_equal(nt.mfpts(T, populations=pops), MFPT_ALL, 5)
    np.testing.assert_array_almost_equal(nt.mfpts(T, sinks=[0]), [0., 2.3125, 2.125], 5)
    np.testing.assert_array_almost_equal(nt.mfpts(T, sinks=[0, 1]), [0., 0., 1.2], 5)
    assert np.array_equal(nt.mfpts(T, sinks=[0, 1], lagtime=4.0),
                          4.0 * nt.mfpts(T, sinks=[0, 1]))


def test_restatement_fluxes_known_answers():
    pops = np.zeros(3) + 1 / 3.
    true = np.zeros((3, 3))
    true[0, 1] = true[1, 2] = np.around(1 / 12., 5)
    f = nt.reactive_fluxes(TFLUX, 0, 2, pops)
    assert np.array_equal(np.around(f, 5), true)
    assert np.array_equal(np.around(nt.net_fluxes(TFLUX, 0, 2, pops), 5), true)
    rp = nt.reactive_populations(TFLUX, 0, 2, pops)
    np.testing.assert_allclose(rp, [0, 1, 0], atol=1e-15)


# ---- the restatement against the goldens -------------------------------------------------
def _restated(g, chain, what):
    C = g["C_" + chain]
    T, pops = nt.tprob_from_counts(C), nt.pops_from_counts(C)
    r = "%s_%s" % (chain, what)
    if what[0] == "q":
        return nt.committors(T, g["src_" + r], g["snk_" + r])
    if what in ("t1", "t3"):
        return nt.mfpts(T, sinks=g["snk_" + r])
    if what == "tall":
        return nt.mfpts(T, populations=pops)
    rq = chain + "_qA"
    fn = nt.reactive_fluxes if what == "fA" else nt.net_fluxes
    return fn(T, g["src_" + rq], g["snk_" + rq], pops)


def test_restatement_passes_the_forward_criterion_on_every_golden(golden):
    g = golden
    results = [k[3:] for k in g.files if k.startswith("hp_")]
    assert len(results) == 7 * 4 + 4 + 2 * 3
    for r in results:
        chain, what = r.split("_")
        x = _restated(g, chain, what)
        hp, err = g["hp_" + r], float(g["err_" + r])
        assert x.shape == hp.shape and x.dtype == np.float64
        got = np.abs(x - hp).max()
        bound = nt.forward_bound(err, hp)
        print("%-12s restatement %.2e  reference %.2e  ratio to the bound %.3f"
              % (r, got, err, got / bound))
        assert got <= bound, r
        if "ref_" + r in g.files:
            # the reference itself lies as close to x_hp as the file says
            assert abs(np.abs(g["ref_" + r] - hp).max() - err) <= nt.U * np.abs(hp).max()


def test_golden_chains_are_what_the_docstring_says(golden):
    g = golden
    assert list(g["chains"]) == ["n17", "n63", "n64", "n65", "n130", "n130x", "n300"]
    for chain in g["chains"]:
        C = g["C_" + chain]
        n = C.shape[0]
        assert chain == "n%d" % n or chain == "n%dx" % n
        assert np.array_equal(C, C.T) and C.dtype == np.int32
        T, pops = nt.tprob_from_counts(C), nt.pops_from_counts(C)
        assert np.abs(T.sum(axis=1) - 1).max() < 1e-15
        assert np.abs(pops @ T - pops).max() < 1e-15
        assert list(g["src_%s_qA" % chain]) == [0] and list(g["snk_%s_qA" % chain]) == [n - 1]
        assert list(g["snk_%s_t3" % chain]) == [0, n // 2, n - 1]
    assert os.path.getsize(GOLDEN) < 600 * 1024


def test_lu_restatement_pivots_and_singularity():
    # first index on ties; exact on integers
    A = np.array([[1., 2., 0.], [-1., 1., 3.], [1., 0., 1.]])
    X, piv, info = nt.lu_solve(A, np.eye(3))
    assert info == -1 and piv[0] == 0
    np.testing.assert_allclose(A @ X, np.eye(3), atol=1e-15)
    S = np.array([[2., 1., 1.], [2., 1., 1.], [0., 1., 3.]])
    assert nt.lu_solve(S, np.ones(3))[2] == 2
    # high precision: refinement reaches long-double accuracy
    rng = np.random.RandomState(0)
    M = rng.rand(12, 12) + 3 * np.eye(12)
    xt = rng.rand(12)
    X, steps = nt.solve_hp(M, M @ xt)
    assert steps <= 3
    R = nt.exact_residual(M, X, M @ xt)
    assert np.abs(R).max() < 1e-17


# ---- what tests/test_gpu_lu_large.py leans on ----------------------------------------------
def test_lu_constants_are_those_of_the_kernels():
    import re
    from enspara_amd.tpt import core
    src = open(os.path.join(os.path.dirname(os.path.abspath(core.__file__)), os.pardir, "csrc",
                            "ek_lu.hip")).read()
    for name in ("LU_PANEL_WG", "LU_SUB_RPT", "LU_COL_WG"):
        defs = re.findall(r"^#define %s (\d+)\b" % name, src, flags=re.M)
        assert defs == [str(getattr(core, name))], name
    assert (core.LU_PANEL_WG, core.LU_SUB_RPT, core.LU_COL_WG) == (1024, 4, 256)
    assert (nt.LU_N_SLOTS, nt.LU_N_TAIL) == (1100, 4200)


def test_exchanged_pairs_give_the_predicted_pivots():
    """the constructor of the large GPU test at n = 200, pairs scaled to fit (both
    edges, neighbours, a k late in the matrix)"""
    n = 200
    pairs = [(0, 64), (1, 199), (2, 127), (3, 128), (8, 100), (9, 110), (63, 65), (70, 198),
             (120, 121), (150, 197)]
    A, want = nt.swapped_dominant(n, pairs, seed=n)
    assert [int(want[k]) for k, _ in pairs] == [r for _, r in pairs]
    assert int(np.sum(want != np.arange(n))) == len(pairs)
    B = np.random.RandomState(1).rand(n, 3)
    X, piv, info, gaps = nt.lu_solve(A, B, return_gaps=True)
    assert info == -1 and np.array_equal(piv, want)
    # (nowhere near a tie: the diagonal's n against entries of about 1)
    assert gaps[:-1].min() > 0.9 and gaps[-1] == np.inf
    assert nt.backward_error(A, X, B) <= 4 * nt.U
    with pytest.raises(AssertionError):
        nt.swapped_dominant(n, [(0, 64), (64, 70)])
    with pytest.raises(AssertionError):
        nt.swapped_dominant(n, [(5, 3)])


def test_tie_system_gives_the_predicted_pivots_and_an_integer_solution():
    n = 200
    triples = [(0, 100, 129, 1), (10, 28, 152, -1), (3, 50, 196, -1), (26, 175, 195, 1),
               (70, 111, 161, -1), (130, 198, 199, 1)]
    A, want = nt.tie_system(n, triples)
    assert set(np.unique(A)) == {-1.0, 0.0, 1.0}
    for k, r1, r2, s in triples:
        assert list(np.flatnonzero(A[:, k])) == [r1, r2] and A[r1, k] == -A[r2, k] == s
        assert want[k] == r1
    B = nt.small_integer_rhs(n)
    X, piv, info, gaps = nt.lu_solve(A, B, return_gaps=True)
    assert info == -1 and np.array_equal(piv, want)
    assert sorted(np.flatnonzero(gaps == 0)) == sorted(t[0] for t in triples)
    assert np.array_equal(X, np.round(X)) and np.array_equal(A @ X, B)
    for k, r1, r2, s in triples:
        assert np.array_equal(X[r1], B[k]) and np.array_equal(X[k], s * B[r1])
        assert np.array_equal(X[r2], B[r2] + B[r1])
    with pytest.raises(AssertionError):
        nt.tie_system(n, [(0, 5, 9, 1), (1, 9, 12, 1)])


def test_lu_gaps_against_a_direct_computation():
    # every intermediate a small dyadic rational: the elimination below is exact
    A = np.array([[2, 1, 0, 1, 0, 3], [-4, 1, 2, 0, 1, 0], [4, 3, 1, 1, 0, 2],
                  [1, 0, -2, 4, 1, 1], [0, 2, 1, 0, -3, 1], [2, 0, 1, 1, 1, 4]], dtype=np.float64)
    X, piv, info, gaps = nt.lu_solve(A, np.eye(6), return_gaps=True)
    M = A.copy()
    want_piv, want_gaps = [], []
    for k in range(6):
        cand = sorted(((abs(M[r, k]), -r) for r in range(k, 6)), reverse=True)
        p = -cand[0][1]
        want_piv.append(p)
        want_gaps.append((cand[0][0] - cand[1][0]) / cand[0][0] if k < 5 else np.inf)
        M[[k, p]] = M[[p, k]]
        for r in range(k + 1, 6):
            M[r, k:] -= (M[r, k] / M[k, k]) * M[k, k:]
    assert info == -1 and list(piv) == want_piv
    assert want_gaps[0] == 0.0 and want_piv[0] == 1     # -4 and 4 tie: the first row
    assert np.array_equal(gaps, want_gaps)
    assert np.array_equal(nt.lu_solve(A, np.eye(6))[0], X)
    # the first columns alone give the first pivots
    piv3, info3, gaps3 = nt.leading_pivots(A, 3)
    assert info3 == -1 and list(piv3) == want_piv[:3] and np.array_equal(gaps3, want_gaps[:3])
    # a column of zeros below the diagonal: gap 0, and the zero pivot reported
    S = np.array([[2., 1., 1.], [2., 1., 1.], [0., 1., 3.]])
    _, _, infoS, gapsS = nt.lu_solve(S, np.ones(3), return_gaps=True)
    assert infoS == 2 and gapsS[0] == 0.0


def test_weighted_chain_is_a_reversible_chain():
    T, pops = nt.weighted_chain(120, seed=3)
    assert np.abs(T.sum(axis=1) - 1).max() < 1e-14 and abs(pops.sum() - 1) < 1e-14
    assert np.abs(pops @ T - pops).max() < 1e-15
    F = pops[:, None] * T
    assert np.abs(F - F.T).max() < 1e-15
    block = np.arange(120) * 10 // 120
    assert T[block[:, None] != block[None, :]].max() < 1e-3
