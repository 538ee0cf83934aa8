"""Bootstrapped transition counts and their two batched builders in plain numpy, written
as the reference does them trial by trial (enspara/msm/bootstrap.py:35-37 and :84-87,
transition_matrices.py:156 and :310-321, builders.py:83-155 and :171-204), not as
enspara_amd/csrc/ek_msm_boot.hip computes them: a Python loop over the trials and the
units each drew, slices, dense matrices.  tests/test_bootstrap_host.py pins this file to
the real reference's recorded outputs; tests/test_gpu_bootstrap.py compares the device
with it."""
import numpy as np


def units_of(assigns, chunk_by=None):
    """The resampling units as a list of 1-D arrays: the trajectories, or with
    ``chunk_by`` their consecutive blocks of that many frames (a shorter last block is
    kept)."""
    rows = [np.asarray(r) for r in assigns]
    if chunk_by is None:
        return rows
    return [r[i:i + chunk_by] for r in rows for i in range(0, len(r), chunk_by)]


def counts_of(units, idx, lag, sliding, n):
    """Dense int64 [n, n] counts of the trial that drew ``units[i] for i in idx``, with
    the reference's slicing: per unit drop the -1 frames, then pair."""
    C = np.zeros((n, n), dtype=np.int64)
    for i in idx:
        a = np.asarray(units[i])
        a = a[a != -1]
        if sliding:
            start, end = a[:-lag], a[lag:]
        else:
            every = a[::lag]
            start, end = every[:-1], every[1:]
        np.add.at(C, (start, end), 1)
    return C


def _row_normalize(C):
    """inv = 1 / rowsum where the row has counts, else 0; T = inv * C: two roundings"""
    w = C.sum(axis=1).astype(np.float64)        # exact: integers below 2^53
    inv = np.zeros_like(w)
    inv[w > 0] = 1.0 / w[w > 0]
    return inv[:, None] * C.astype(np.float64)


def normalize(C):
    """-> (counts, probabilities); the populations are an eigenvector, not restated"""
    return C, _row_normalize(C)


def transpose(C):
    """-> (counts, probabilities, populations) of builders.transpose"""
    S = C + C.T
    return S / 2, _row_normalize(S), S.sum(axis=1) / S.sum()
