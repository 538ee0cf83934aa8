#!/usr/bin/env python3
"""Generate tests/golden/bootstrap_golden.npz by running the REAL reference's
bootstrap(MSM.from_assignments, ...) (bowman-lab/enspara, msm/bootstrap.py:10-48) under
np.random.seed on two fixtures.

Run it where make_golden.py runs (it imports the reference the same way, through
make_golden.import_reference):

    python tests/golden/make_bootstrap_golden.py

Fixtures:
  a  the three 60-frame trajectories with -1 gaps over 4 states of the reference's own
     test (test/msm_data.py TRIMMABLE, test/test_msm_bootstrap.py), builders.transpose,
     100 trials, seed 0; with the table of mean probabilities that test compares with.
  b  12 seeded trajectories of 40 frames over 5 states, each visiting every state and
     returning to its first, builders.normalize, 65 trials, seed 1.  One such trajectory
     alone connects all five states strongly, so every resample is strongly connected
     and no trial has to be left out of the population comparison; the generator checks
     that with scipy.sparse.csgraph and refuses otherwise.

Per fixture the file holds the input `<f>_assigns`, `<f>_seed`, the draws `<f>_draws`
[trials, trajectories] (numpy's generator replayed: the draws are the first thing the
reference takes from it), and per trial the dense `<f>_tcounts`, `<f>_tprobs` and
`<f>_eq_probs` of the reference's MSMs.  Only inputs and outputs are stored; no
reference source is copied.
"""
import os
import sys

import numpy as np
import scipy.sparse
from scipy.sparse.csgraph import connected_components

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402

# the reference's test/test_msm_bootstrap.py compares the mean of fixture a's
# probabilities with this table, rtol = 0.2
A_MEAN_TABLE = np.array([[0.93871, 0.03128, 0.00000, 0.00000],
                         [0.01297, 0.97553, 0.01149, 0.00000],
                         [0.00000, 0.02470, 0.91199, 0.01330],
                         [0.00000, 0.00000, 0.72000, 0.00000]])


def fixture_a():
    return np.array([([0] * 30 + [1] * 20 + [-1] * 10),
                     ([2] * 20 + [-1] * 5 + [1] * 35),
                     ([0] * 10 + [1] * 30 + [2] * 19 + [3])])


def fixture_b():
    rng = np.random.RandomState(2024)
    rows = []
    for _ in range(12):
        order = rng.permutation(5)
        cuts = np.sort(rng.choice(np.arange(1, 39), 4, replace=False))
        dwell = np.diff(np.concatenate([[0], cuts, [39]]))
        rows.append(np.concatenate([np.repeat(order, dwell), order[:1]]))
    return np.array(rows)


def dense(m):
    return np.asarray(m.todense()) if scipy.sparse.issparse(m) else np.asarray(m)


def run(name, assigns, seed, method, n_trials, n_states, out):
    from enspara.msm import MSM
    from enspara.msm.bootstrap import bootstrap
    from enspara.msm.transition_matrices import assigns_to_counts
    np.random.seed(seed)
    draws = np.array([np.random.choice(np.arange(len(assigns)), len(assigns))
                      for _ in range(n_trials)], dtype=np.int64)
    np.random.seed(seed)
    msms = bootstrap(MSM.from_assignments, assigns, lag_time=1, method=method,
                     n_trials=n_trials, max_n_states=n_states, n_procs=1)
    assert len(msms) == n_trials
    for r, m in enumerate(msms):
        # the replayed draws are the reference's: its counts of exactly these rows
        C = dense(assigns_to_counts(assigns[draws[r]], lag_time=1, max_n_states=n_states))
        _, _, eq = method(scipy.sparse.coo_matrix(C))
        assert np.array_equal(dense(method(scipy.sparse.coo_matrix(C))[0]), dense(m.tcounts_)), r
        assert np.array_equal(eq, m.eq_probs_, equal_nan=True), r
    out[name + "_assigns"] = assigns.astype(np.int32)
    out[name + "_seed"] = np.int64(seed)
    out[name + "_draws"] = draws
    out[name + "_tcounts"] = np.array([dense(m.tcounts_) for m in msms])
    out[name + "_tprobs"] = np.array([dense(m.tprobs_) for m in msms], dtype=np.float64)
    out[name + "_eq_probs"] = np.array([m.eq_probs_ for m in msms], dtype=np.float64)
    return msms


def main():
    import_reference()
    import logging
    logging.disable(logging.CRITICAL)
    from enspara.msm import builders
    out = {}
    run("a", fixture_a(), 0, builders.transpose, 100, 4, out)
    np.testing.assert_allclose(out["a_tprobs"].mean(axis=0), A_MEAN_TABLE, rtol=0.2)
    out["a_mean_table"] = A_MEAN_TABLE
    b = fixture_b()
    assert b.shape == (12, 40)
    for row in b:
        assert set(row.tolist()) == set(range(5)) and row[0] == row[-1]
    run("b", b, 1, builders.normalize, 65, 5, out)
    for r, C in enumerate(out["b_tcounts"]):
        n, _ = connected_components(scipy.sparse.csr_matrix(C), connection="strong")
        if n != 1:
            sys.exit("fixture b, trial %d: %d strongly connected components" % (r, n))
    path = os.path.join(HERE, "bootstrap_golden.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 600 * 1024, size
    print("wrote %s (%d bytes)" % (path, size))


if __name__ == "__main__":
    main()
