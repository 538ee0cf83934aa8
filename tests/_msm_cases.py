"""Matrices and assertions that the host tests of the eigensolver
(tests/test_msm_host.py, numpy stand-ins) and the device tests
(tests/test_gpu_krylov.py) share (TEST CODE)."""
import numpy as np
import scipy.sparse

from enspara_amd.msm import transition_matrices as tm


def _rowstoch(n, density, seed):
    rng = np.random.RandomState(seed)
    C = scipy.sparse.random(n, n, density=density, random_state=rng,
                            format="csr")
    C = C + scipy.sparse.diags(np.ones(n)) + \
        scipy.sparse.diags(np.ones(n - 1) * 0.5, 1) + \
        scipy.sparse.diags(np.ones(n - 1) * 0.5, -1)
    C = scipy.sparse.csr_matrix(C)
    w = np.asarray(C.sum(axis=1)).ravel()
    return scipy.sparse.diags(1.0 / w) @ C


def _breakdown_matrix(kind):
    """1500-state chains whose Krylov space closes after a few steps, so that the
    sub-diagonal entry is an exact (or 1e-17) zero and not rounding noise: the
    permutation of 375 four-cycles (eigenvalues 1, i, -1, -i, 375 times each), all
    rows equal to one distribution (1, then 0), and 500 copies of a 3-state chain
    (1, 0.5, 0, 500 times each)."""
    n = 1500
    if kind == "four_cycles":
        i = np.arange(n)
        return scipy.sparse.csr_matrix((np.ones(n), (i, 4 * (i // 4) + (i + 1) % 4)),
                                       shape=(n, n))
    if kind == "rank_one":
        p = np.random.RandomState(7).uniform(0.5, 1.5, size=n)
        return scipy.sparse.csr_matrix(np.tile(p / p.sum(), (n, 1)))
    assert kind == "kron"
    B = np.array([[.5, .5, 0], [.25, .5, .25], [0, .5, .5]])
    return scipy.sparse.kron(scipy.sparse.identity(n // 3), B, format="csr")


def _counting(cls):
    """cls with the fresh directions it is asked to orthogonalise counted
    (step(j, apply=False): transition_matrices._expand after a breakdown)"""
    class Counting(cls):
        fresh = 0

        def step(self, j, apply=True):
            if not apply:
                type(self).fresh += 1
            return super().step(j, apply)
    return Counting


def _check_solver_case(case, space_cls, **kw):
    """The assertions of the solver's cases, shared with tests/test_gpu_krylov.py
    (there space_cls is the device's space).  1e-9 is the project's figure for
    eigenvalues against LAPACK (test_small_dense_all_eigs_matches_reference)."""
    counting = _counting(space_cls)
    if isinstance(case, str):
        T, n_eigs = _breakdown_matrix(case), 4
    else:
        T = _rowstoch(case, min(1, 6 / case), case)
        n_eigs = None if case <= 1000 else 8
    vals, vecs = tm.eigenspectrum(T, n_eigs=n_eigs,
                                  _space_factory=lambda A, m: counting(A, m, **kw))
    w = np.sort(np.linalg.eigvals(T.toarray()).real)[::-1]
    np.testing.assert_allclose(vals, w[:len(vals)], rtol=0, atol=1e-9)
    assert len(vals) == (T.shape[0] if n_eigs is None else n_eigs)
    pi = vecs[:, 0]
    assert np.abs(T.T @ pi - pi).max() <= 1e-9
    assert abs(pi.sum() - 1.0) <= 1e-12
    if isinstance(case, str):
        # the test reached the path it is named for
        assert counting.fresh > 0, "no fresh direction was asked for"
    return counting.fresh
