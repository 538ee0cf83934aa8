#!/usr/bin/env python3
"""Generate tests/golden/mi_golden.npz by running the REAL reference's
enspara/info_theory/mutual_info.py (joint_counts on libinfo.matrix_bincount2d,
mutual_information, mi_matrix, the mi_to_* conversions) on seeded data.

    python tests/golden/make_mi_golden.py

make_golden.import_reference() builds the reference's extensions (libinfo among
them) in a temporary directory.  Only inputs and outputs are stored; no
reference source is copied.

  rag_X [3637, 6] / rag_Y [3637, 7] int8, rag_lengths (1000, 137, 2500): three
      ragged trajectories, n_x = 3, n_y = 5, feature i biased towards state i % n,
      column 2 of Y a noisy copy of column 4 of X
      rag_jc      the sum of the reference's joint_counts over the trajectories
      rag_mi      mutual_information(rag_jc)
      rag_mimat   mi_matrix(list, list, 3, 5, normalize=False)
  self_X [5000, 24] int8, n = 3: X against itself, column 7 a noisy copy of column 1
      self_jc, self_mi   joint_counts(X, n_x=3), mutual_information of it
      self_mimat         mi_matrix([X], [X], 3, 3)  (normalised by channel capacity)
  conv_mi [24, 24]: (self_mi + self_mi.T) / 2, symmetric as the conversions demand
      conv_apc, conv_nmi, conv_nmi_apc   mi_to_apc, mi_to_nmi, mi_to_nmi_apc of it

The generator checks the numpy restatement the GPU tests expect from
(tests/_numpy_mi.py) against the reference: counts equal, mutual information
equal bit for bit (both are numpy, in the same order, on the same libm).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import import_reference  # noqa: E402
import _numpy_mi as nm  # noqa: E402

RAG_LENGTHS = (1000, 137, 2500)


def main():
    import_reference()
    from enspara.info_theory import mutual_info as rmi

    out = {}
    rng = np.random.RandomState(20)
    T = sum(RAG_LENGTHS)
    X = nm.biased_codes(rng, T, 6, 3, np.int8)
    Y = nm.noisy_copy(rng, nm.biased_codes(rng, T, 7, 5, np.int8), X, 2, 4, 5)
    Y = Y.astype(np.int8)
    ends = np.cumsum(RAG_LENGTHS)
    Xs = [X[e - n:e] for e, n in zip(ends, RAG_LENGTHS)]
    Ys = [Y[e - n:e] for e, n in zip(ends, RAG_LENGTHS)]
    jc = sum(rmi.joint_counts(a, b, 3, 5).astype(np.uint64) for a, b in zip(Xs, Ys))
    assert jc.dtype == np.uint64 and jc.shape == (6, 7, 3, 5)
    assert np.array_equal(jc, rmi.joint_counts(X, Y, 3, 5))
    out["rag_X"], out["rag_Y"] = X, Y
    out["rag_lengths"] = np.array(RAG_LENGTHS)
    out["rag_jc"] = jc.astype(np.uint32)
    out["rag_mi"] = rmi.mutual_information(out["rag_jc"])
    out["rag_mimat"] = rmi.mi_matrix(Xs, Ys, 3, 5, normalize=False)
    assert np.array_equal(out["rag_mi"], out["rag_mimat"])

    rng = np.random.RandomState(21)
    X = nm.biased_codes(rng, 5000, 24, 3, np.int8)
    X = nm.noisy_copy(rng, X, X, 7, 1, 3).astype(np.int8)
    out["self_X"] = X
    out["self_jc"] = rmi.joint_counts(X, n_x=3)
    assert out["self_jc"].dtype == np.uint32
    out["self_mi"] = rmi.mutual_information(out["self_jc"])
    out["self_mimat"] = rmi.mi_matrix([X], [X], 3, 3)
    asym = out["self_mi"] != out["self_mi"].T
    print("self_mi: %d of %d entries differ from their transpose, by at most %.1e"
          % (asym.sum(), asym.size, np.abs(out["self_mi"] - out["self_mi"].T).max()))

    sym = (out["self_mi"] + out["self_mi"].T) / 2
    out["conv_mi"] = sym
    out["conv_apc"] = rmi.mi_to_apc(sym)
    out["conv_nmi"] = rmi.mi_to_nmi(sym)
    out["conv_nmi_apc"] = rmi.mi_to_nmi_apc(sym)

    # the restatement against the reference
    for tag, (a, b, nx, ny) in {"rag": (out["rag_X"], out["rag_Y"], 3, 5),
                                "self": (out["self_X"], None, 3, 3)}.items():
        jc_np = nm.joint_counts(a, b, nx, ny)
        assert jc_np.dtype == np.uint32
        assert np.array_equal(jc_np, out[tag + "_jc"]), tag
        mi_np, S = nm.mutual_information(jc_np)
        assert np.array_equal(mi_np, out[tag + "_mi"]), tag
        # how far a log that is one ulp off carries, against the tests' bound
        mi_p, _ = nm.mutual_information(jc_np, perturb=np.random.RandomState(5))
        ratio = np.abs(mi_p - mi_np) / nm.mi_bound(nx, ny, S)
        print("%s: restatement == reference; logs moved by 1 ulp reach %.2f of the bound"
              % (tag, ratio.max()))
        assert ratio.max() <= 1

    path = os.path.join(HERE, "mi_golden.npz")
    np.savez_compressed(path, **out)
    print("mi_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
