#!/usr/bin/env python3
"""Generate tests/golden/entropy_golden.npz by running the REAL reference's
enspara/info_theory/entropy.py and the functions of its
enspara/apps/compute-shannon-entropy.py on fixed and seeded data.

    python -O tests/golden/make_entropy_golden.py

With asserts off, as for make_mle_golden.py: the reference's mle builder closes with
`assert np.all(T.sum(axis=1) == 1)`, which compares rounded row sums for equality and
fails on ordinary counts.  This script's own checks do not use `assert`.  Only inputs and outputs are stored; no reference source is copied.

  ts_*   the three-state cases of the reference's own test_entropy.py
      ts_P, ts_assignments
      ts_Q_{raw,prior,transpose}     Q_from_assignments(prior_counts=0 / default /
                                     builder=transpose)
      ts_per_{raw,prior,transpose}   relative_entropy_per_state(P, assignments=...) (row 0
                                     of raw is +inf)
      ts_msm_{raw,prior,transpose}   relative_entropy_msm(P, assignments=...)
      ts_pops                        eq_probs(P), what relative_entropy_msm weighted by
  kl_*   kl_P, kl_Q and kl_base_{2,e,10} = kl_divergence of them
  js_p, js_q [4, 7], js_out = js_divergence(p, q)
  sh_p [37], sh_H = shannon_entropy(p), sh_H_raw = shannon_entropy(p / p.sum(), False)
  chain{n}_* for n = 5, 17, 40: a seeded metastable chain T, assignments [4, 400] drawn
      from it, and per builder b in normalize, transpose, mle
      chain{n}_Q_{b}, chain{n}_per_{b}, chain{n}_msm_{b}   as above, default prior, with
      populations = chain{n}_pops (eq_probs(T))
  rot_*  rotamer codes: rot_X [1118, 9] int8 in three ragged trajectories rot_lengths
      (300, 41, 777), rot_n_states (2- and 3-state features mixed), rot_atom_indices
      [9, 4], rot_atom_residue [40] (the residue of every atom; residue 2 of 5 has no
      dihedral)
      rot_counts        the app's compute_rotamer_counts
      rot_H             compute_dihedral_shannon_entropy(counts / counts.sum(-1))
      rot_residue_H     compute_residue_shannon_entropies (NaN for residue 2)

The generator checks the numpy restatement the tests expect from
(tests/_numpy_entropy.py) against the reference as it goes.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import import_reference  # noqa: E402
import _numpy_entropy as ne  # noqa: E402

ROT_LENGTHS = (300, 41, 777)


def check(ok, what):
    if not ok:
        sys.exit("check failed: " + what)


def load_app(tmp):
    """the app as a module; its package (enspara.apps imports every app, one of which
    needs pytables) is stood in for by an empty one with the one name the app takes"""
    apps = types.ModuleType("enspara.apps")
    apps.util = types.ModuleType("enspara.apps.util")
    apps.util.readable_dir = str
    sys.modules.setdefault("enspara.apps", apps)
    sys.modules.setdefault("enspara.apps.util", apps.util)
    path = os.path.join(tmp, "enspara", "apps", "compute-shannon-entropy.py")
    spec = importlib.util.spec_from_file_location("compute_shannon_entropy", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if __debug__:
        sys.exit("run with python -O: the reference's mle builder closes with asserts that "
                 "fail on ordinary counts")
    tmp = import_reference()
    from enspara.info_theory import entropy as rent
    from enspara.msm import builders as rbuilders
    from enspara.msm.transition_matrices import eq_probs

    out = {}
    # ---- the reference's own three-state cases ------------------------------------------
    P = np.array([[0.5, 0.5, 0], [0.25, 0.25, 0.5], [0, 0.25, 0.75]])
    A = np.array([[0, 1, 1, 0, 1, 0, 2, 2, 0, 1, 1, 1], [0, 2, 2, 1, 2, 0, 2, 1, 0, 1, 2, 1]])
    out["ts_P"], out["ts_assignments"] = P, A
    out["ts_pops"] = eq_probs(P)
    for tag, kw, mine in (("raw", {"prior_counts": 0}, {"prior_counts": 0}),
                          ("prior", {}, {}),
                          ("transpose", {"builder": rbuilders.transpose},
                           {"builder": "transpose"})):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out["ts_Q_" + tag] = rent.Q_from_assignments(A, **kw)
            out["ts_per_" + tag] = rent.relative_entropy_per_state(P, assignments=A, **kw)
            out["ts_msm_" + tag] = rent.relative_entropy_msm(P, assignments=A, **kw)
        np.testing.assert_array_almost_equal(
            ne.Q_from_assignments(A, **mine), out["ts_Q_" + tag], 12)
    check(np.isposinf(out["ts_per_raw"][0]) and np.isposinf(out["ts_msm_raw"]), "inf row")

    out["kl_P"] = P
    out["kl_Q"] = np.array([[0.25, 0.25, 0.5], [0.25, 0.25, 0.5], [0.1, 0.65, 0.25]])
    for tag, base in (("2", 2), ("e", np.e), ("10", 10)):
        out["kl_base_" + tag] = rent.kl_divergence(out["kl_P"], out["kl_Q"], base=base)
        check(np.array_equal(ne.kl_divergence(out["kl_P"], out["kl_Q"], base)[0],
                             out["kl_base_" + tag]), "kl restatement, base " + tag)

    rng = np.random.RandomState(30)
    out["js_p"], out["js_q"] = ne.random_rows(rng, 4, 7), ne.random_rows(rng, 4, 7)
    out["js_p"][1, 2] = 0.0
    out["js_out"] = rent.js_divergence(out["js_p"], out["js_q"])
    check(np.array_equal(ne.js_divergence(out["js_p"], out["js_q"])[0], out["js_out"]),
          "js restatement")
    out["sh_p"] = rng.rand(37)
    out["sh_p"][5] = 0.0
    out["sh_H"] = rent.shannon_entropy(out["sh_p"])
    out["sh_H_raw"] = rent.shannon_entropy(out["sh_p"] / out["sh_p"].sum(), normalize=False)
    np.testing.assert_allclose(ne.shannon_entropy(out["sh_p"])[0], out["sh_H"], rtol=1e-13)

    # ---- seeded chains, the three builders ---------------------------------------------
    for n in (5, 17, 40):
        rng = np.random.RandomState(100 + n)
        T = ne.metastable_chain(rng, n)
        A = ne.sample_chain(rng, T, 4, 400)
        k = "chain%d_" % n
        out[k + "T"], out[k + "assignments"] = T, A.astype(np.int32)
        pops = eq_probs(T)
        out[k + "pops"] = pops
        for b in ("normalize", "transpose", "mle"):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                kw = {"builder": getattr(rbuilders, b)}
                out[k + "Q_" + b] = rent.Q_from_assignments(A, n_states=n, **kw)
                out[k + "per_" + b] = rent.relative_entropy_per_state(T, assignments=A, **kw)
                out[k + "msm_" + b] = rent.relative_entropy_msm(
                    T, assignments=A, populations=pops, **kw)
            if b != "mle":
                np.testing.assert_array_almost_equal(
                    ne.Q_from_assignments(A, n_states=n, builder=b), out[k + "Q_" + b], 12)
            np.testing.assert_array_almost_equal(
                ne.kl_divergence(T, out[k + "Q_" + b])[0], out[k + "per_" + b], 12)

    # ---- rotamer codes through the app's functions -------------------------------------
    app = load_app(tmp)
    rng = np.random.RandomState(31)
    n_states = np.array([3, 2, 3, 3, 2, 2, 3, 2, 3])
    T = sum(ROT_LENGTHS)
    X = np.stack([rng.choice(n, size=T, p=rng.dirichlet(np.ones(n) * 0.7))
                  for n in n_states], axis=1).astype(np.int8)
    X[:, 4] = 1                                     # a dihedral that never moves: H = 0
    ends = np.cumsum(ROT_LENGTHS)
    trajs = [X[e - m:e] for e, m in zip(ends, ROT_LENGTHS)]
    atom_residue = np.repeat(np.arange(5), 8)       # 40 atoms, 5 residues
    residue_of = np.array([0, 0, 1, 1, 1, 3, 3, 4, 4])     # residue 2: no dihedral
    quads = np.stack([residue_of * 8, residue_of * 8 + 1,
                      residue_of * 8 + 2, residue_of * 8 + 3], axis=1)
    check(np.array_equal(atom_residue[quads[:, 1]], residue_of), "residue of atom 1")
    rot = types.SimpleNamespace(feature_trajectories_=trajs, n_feature_states_=n_states,
                                atom_indices_=quads)
    counts = app.compute_rotamer_counts(rot)
    H = app.compute_dihedral_shannon_entropy(counts / counts.sum(axis=-1)[..., None])

    class _Top:
        n_residues = 5

        @staticmethod
        def atom(i):
            return types.SimpleNamespace(
                residue=types.SimpleNamespace(resSeq=int(atom_residue[i]) + 1))

    app.md.load = lambda f: types.SimpleNamespace(top=_Top)
    with np.errstate(all="ignore"):
        res_H, _ = app.compute_residue_shannon_entropies(H, "topology", quads, n_states)
    out.update(rot_X=X, rot_lengths=np.array(ROT_LENGTHS), rot_n_states=n_states,
               rot_atom_indices=quads, rot_atom_residue=atom_residue,
               rot_counts=np.asarray(counts).astype(np.int64), rot_H=H, rot_residue_H=res_H)
    check(np.isnan(res_H[2]) and np.isfinite(np.delete(res_H, 2)).all() and H[4] == 0,
          "NaN for the residue without dihedrals, 0 for the fixed dihedral")
    mine = ne.state_counts(trajs, 3)
    check(np.array_equal(mine, out["rot_counts"]), "count restatement")
    np.testing.assert_allclose(ne.dihedral_entropies(mine)[0], H, rtol=0, atol=1e-14)
    np.testing.assert_allclose(ne.residue_entropies(H, n_states, residue_of, 5), res_H,
                               rtol=1e-14, equal_nan=True)

    path = os.path.join(HERE, "entropy_golden.npz")
    np.savez_compressed(path, **out)
    print("entropy_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
