#!/usr/bin/env python3
"""Generate tests/golden/mle_golden.npz by running the REAL reference's
builders.mle (bowman-lab/enspara, builders.py:24-80 with the pure-Python
iteration :215-318) on seeded count matrices.

Run it where make_golden.py runs (it imports the reference the same way, through
make_golden.import_reference), and with asserts off:

    python -O tests/golden/make_mle_golden.py

-O is needed: the reference closes its iteration with
`assert np.all(T.sum(axis=1) == 1)` (:315-316), which compares rounded row sums
for equality and fails on ordinary inputs; without -O the reference aborts there.

Per case the file holds the input counts `C_<case>`, the reference's `T_<case>` and
`pi_<case>` at its default tol = 1e-10, and `atol_<case>` =
max |T(tol=1e-10) - T(tol=1e-11)|: how far the reference itself still moves in the
sweeps after its stop.  A stop that falls a sweep or two earlier or later -- logl,
which decides it, is summed in another order on the device -- stays inside that.
The generator refuses an atol of 1e-9 or more, so the tolerance cannot become
vacuous.  Only inputs and outputs are stored; no reference source is copied.
"""
import os
import sys
import warnings

import numpy as np
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


def cases():
    out = {"n3_dense": np.array([[0, 2, 8], [4, 2, 4], [7, 3, 0]]),
           "n3_sparse": scipy.sparse.csr_matrix(
               np.array([[5, 1, 0], [2, 0, 3], [0, 4, 6]]))}
    for n, fill in ((12, 0.4), (40, 0.15)):
        rng = np.random.RandomState(100 + n)
        out["n%d_dense" % n] = rng.randint(1, 60, size=(n, n))
        C = rng.randint(1, 40, size=(n, n)) * (rng.rand(n, n) < fill)
        C[np.arange(n), (np.arange(n) + 1) % n] += 1 + rng.randint(0, 4, size=n)
        out["n%d_sparse" % n] = scipy.sparse.csr_matrix(C)
    return out


def main():
    if __debug__:
        sys.exit("run with python -O: the reference's closing asserts "
                 "(builders.py:315-316) fail on ordinary inputs")
    import_reference()
    import logging
    logging.disable(logging.CRITICAL)
    from enspara.msm import builders as rbuilders
    out = {}
    worst = 0.0
    for name, C in cases().items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            Cout, T, pi = rbuilders.mle(C)
            assert_type = type(T) is type(C)
            dense = np.asarray(C.todense()) if scipy.sparse.issparse(C) else C
            T11, _ = rbuilders._prinz_mle_py(dense, tol=1e-11)
        if not assert_type:
            sys.exit("%s: the reference returned %s for %s" % (name, type(T), type(C)))
        T = np.asarray(T.todense()) if scipy.sparse.issparse(T) else np.asarray(T)
        atol = float(np.abs(T - np.asarray(T11)).max())
        if not atol < 1e-9:
            sys.exit("%s: the reference moves by %g after its stop" % (name, atol))
        worst = max(worst, atol)
        out["C_" + name] = dense
        out["T_" + name] = T
        out["pi_" + name] = np.asarray(pi, dtype=np.float64).ravel()
        out["atol_" + name] = np.array(atol)
        print(name, "atol", atol, flush=True)
    out["cases"] = np.array(sorted(cases()))
    path = os.path.join(HERE, "mle_golden.npz")
    np.savez_compressed(path, **out)
    print("mle_golden.npz", os.path.getsize(path) // 1024, "KiB; largest atol", worst)


if __name__ == "__main__":
    main()
