#!/usr/bin/env python3
"""Generate tests/golden/kmc_golden.npz by running the REAL reference's
enspara/msm/synthetic_data.py and the array-only functions of its
enspara/geometry/dyes_from_expt_dist.py (mdtraj stubbed, as for the other goldens).

    python tests/golden/make_kmc_golden.py

Only inputs and outputs are stored; no reference source is copied.

The reference seeds its generators from the OS (``np.random.default_rng()`` in
synthetic_trajectory and _sample_FRET_histograms, ``np.random.seed()`` per photon in
sample_FE_probs), so nothing of its sampling can be recorded as it stands.  This script
replaces ``np.random.default_rng`` and ``np.random.seed`` by ones that seed with known
numbers while the reference runs, and stores next to every output the doubles those
generators hand out, in the order the reference consumes them, replayed from the same
seeds afterwards:
  default_rng call 1 of a burst   1 double (the initial state's choice), then n_photons
                                  (the coins, rng.random(n))
  default_rng call 2 of a burst   n_frames - 1 doubles, one per rng.choice(n, 1, p=row)
  np.random.seed call k           2 doubles: np.random.choice's, np.random.random()'s
Every part of the consumption order is reproduced this way and checked below: the model
(tests/_numpy_kmc.py) fed these doubles must give the recorded outputs.  What is pinned
by formula only: the value of E, where the model's d^6 = (d d)(d d)(d d) differs from the
reference's d ** 6 by rounding (fe_E is stored; the host test bounds the gap).

  ens_T [5, 5], ens_p0, ens_obs; ens_{dense,sparse}_{p,all,pobs,obs}: synthetic_ensemble
      of 30 steps without (p, all) and with (pobs, obs) the observable
  fe_dists, fe_r0, fe_offset, fe_out            FRET_efficiency
  md_probs, md_edges (flat), md_lengths, md_out, md_out_lengths   make_distribution
  cp_times (flat), cp_lengths, cp_lagtime, cp_slowing, cp_out (flat)  convert_photon_times
  kmc_T [6, 6] with zeros; traj_{dense,sparse}, traj_start, traj_u_{dense,sparse}
      synthetic_trajectory of 300 steps and its 299 doubles
  dd (flat [bins, 2]), dd_lengths; pops; R0
  fe_states, fe_E, fe_u [n, 2]                  sample_FE_probs and (bin, jitter) doubles
  burst_frames (flat), burst_lengths, burst_std (n_photon_std, 0 = None)
  burst_val, burst_sd (NaN = None), burst_trj (flat), burst_trj_lengths
  burst_u_init [n_bursts], burst_u_trans (flat, per burst n_frames - 1),
  burst_u_bin, burst_u_jitter, burst_u_coin (flat, per burst n_photons)
"""
import os
import sys

import numpy as np
import scipy.sparse
import scipy.sparse.linalg  # noqa: F401  (the reference uses it without importing it)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import import_reference  # noqa: E402
import _numpy_kmc as nk  # noqa: E402

REAL_RNG, REAL_SEED = np.random.default_rng, np.random.seed


def check(ok, what):
    if not ok:
        sys.exit("check failed: " + what)


class Seeded(object):
    """stands in for np.random.default_rng / np.random.seed and remembers the seeds"""

    def __init__(self):
        self.rng_seeds, self.legacy_seeds = [], []

    def default_rng(self, *args):
        self.rng_seeds.append(1000 + len(self.rng_seeds))
        return REAL_RNG(self.rng_seeds[-1])

    def seed(self, *args):
        self.legacy_seeds.append(5000 + len(self.legacy_seeds))
        REAL_SEED(self.legacy_seeds[-1])

    def __enter__(self):
        np.random.default_rng, np.random.seed = self.default_rng, self.seed
        return self

    def __exit__(self, *exc):
        np.random.default_rng, np.random.seed = REAL_RNG, REAL_SEED


def legacy_doubles(seeds):
    return np.array([np.random.RandomState(s).random_sample(2) for s in seeds]).reshape(-1, 2)


def main():
    import_reference()
    from enspara import ra as rra
    from enspara.msm import synthetic_data as rsd
    from enspara.geometry import dyes_from_expt_dist as rdyes

    out = {}
    rng = np.random.RandomState(40)

    # ---- ensemble ------------------------------------------------------------------------
    T = nk.random_T(rng, 5, 4)
    p0, obs = rng.dirichlet(np.ones(5)), rng.randn(5)
    out.update(ens_T=T, ens_p0=p0, ens_obs=obs)
    for tag, M in (("dense", T), ("sparse", scipy.sparse.csr_matrix(T))):
        out["ens_%s_p" % tag], out["ens_%s_all" % tag] = rsd.synthetic_ensemble(M, p0, 30)
        out["ens_%s_pobs" % tag], out["ens_%s_obs" % tag] = rsd.synthetic_ensemble(
            M, p0, 30, observable_per_state=obs)
        gap = np.abs(nk.ensemble(M, p0, 30)[1] - out["ens_%s_all" % tag]).sum(axis=1)
        check(np.all(gap <= nk.ensemble_bound(T, p0, 30)), "ensemble model, " + tag)

    # ---- the numpy helpers ---------------------------------------------------------------
    out["fe_dists"], out["fe_r0"], out["fe_offset"] = rng.rand(50) * 10, 5.4, 0.3
    out["fe_out"] = rdyes.FRET_efficiency(out["fe_dists"], 5.4, offset=0.3)
    lengths = [4, 1, 7]
    probs = [rng.rand(k) for k in lengths]
    edges = [np.sort(rng.rand(k + 1)) * 8 for k in lengths]
    made = rdyes.make_distribution(rra.RaggedArray(probs), rra.RaggedArray(edges))
    out.update(md_probs=np.concatenate(probs), md_edges=np.concatenate(edges),
               md_lengths=np.array(lengths), md_out=np.asarray(made._data),
               md_out_lengths=np.asarray(made.lengths))
    times = [rng.rand(k) * 30 for k in (5, 1, 12)]
    conv = rdyes.convert_photon_times(times, 5.0, 1.7)
    out.update(cp_times=np.concatenate(times), cp_lengths=np.array([5, 1, 12]),
               cp_lagtime=5.0, cp_slowing=1.7,
               cp_out=np.concatenate([np.asarray(c, dtype=np.int64) for c in conv]))

    # ---- one chain -----------------------------------------------------------------------
    T = nk.random_T(rng, 6, 4)
    out["kmc_T"], out["traj_start"] = T, 2
    for tag, M in (("dense", T), ("sparse", scipy.sparse.csr_matrix(T))):
        with Seeded() as sd:
            traj = rsd.synthetic_trajectory(M, 2, 300)
        check(len(sd.rng_seeds) == 1, "one generator per trajectory")
        u = REAL_RNG(sd.rng_seeds[0]).random(299)
        out["traj_" + tag], out["traj_u_" + tag] = traj, u
        model = nk.chains(T, [2], 300, nk.RecordedUniforms({(nk.TRANS, 0): u}))[0]
        check(np.array_equal(model, traj), "chain model, " + tag)

    # ---- photons ---------------------------------------------------------------------------
    bins = [3, 2, 9, 1, 5, 4]
    dd = []
    for s, k in enumerate(bins):
        p = rng.dirichlet(np.ones(k))
        if k > 3:
            p[2] = 0.0
            p /= p.sum()
        dd.append(np.stack([1.5 + 0.4 * np.arange(k) + 0.05 * s, p], axis=1))
    pops = rng.dirichlet(np.ones(6))
    R0 = 5.4
    out.update(dd=np.concatenate(dd), dd_lengths=np.array(bins), pops=pops, R0=R0)

    states = rng.randint(0, 6, size=40)
    with Seeded() as sd:
        E = rdyes.sample_FE_probs(dd, states, R0)
    u2 = legacy_doubles(sd.legacy_seeds)
    check(len(u2) == 40, "one seed per photon")
    out.update(fe_states=states, fe_E=E, fe_u=u2)
    model = nk.fret_probs(dd, states, R0, nk.RecordedUniforms(
        {(nk.BIN, 0): u2[:, 0], (nk.JITTER, 0): u2[:, 1]}))
    check(np.allclose(model, E, rtol=2.0 ** -49, atol=0), "E model")

    frames = [np.sort(rng.randint(0, last + 1, size=k))
              for k, last in ((1, 0), (9, 30), (16, 200), (17, 90), (40, 400), (2, 1))]
    stds = [0, 4, 4, 4, 7, 0]
    rec = {k: [] for k in ("val", "sd", "trj", "init", "trans", "bin", "jitter", "coin")}
    for b, (f, std) in enumerate(zip(frames, stds)):
        with Seeded() as sd:
            val, dev, trj = rdyes._sample_FRET_histograms(f, T, pops, dd, R0, std or None)
        check(len(sd.rng_seeds) == 2 and len(sd.legacy_seeds) == len(f), "generators of a burst")
        a = REAL_RNG(sd.rng_seeds[0])
        init, coin = a.random(), a.random(len(f))
        trans = REAL_RNG(sd.rng_seeds[1]).random(len(trj) - 1)
        u2 = legacy_doubles(sd.legacy_seeds)
        m_val, m_dev, m_trj, _ = nk.burst(T, pops, dd, f, R0, std or None, nk.RecordedUniforms({
            (nk.INIT, b): [init], (nk.TRANS, b): trans, (nk.BIN, b): u2[:, 0],
            (nk.JITTER, b): u2[:, 1], (nk.COIN, b): coin}), chain=b)
        check(np.array_equal(m_trj, trj) and m_val == val and
              (m_dev == dev if std else dev is None), "burst model, burst %d" % b)
        for k, v in (("val", val), ("sd", np.nan if dev is None else dev), ("trj", trj),
                     ("init", init), ("trans", trans), ("bin", u2[:, 0]), ("jitter", u2[:, 1]),
                     ("coin", coin)):
            rec[k].append(v)
    out.update(burst_frames=np.concatenate(frames),
               burst_lengths=np.array([len(f) for f in frames]), burst_std=np.array(stds),
               burst_val=np.array(rec["val"], dtype=np.float64),
               burst_sd=np.array(rec["sd"], dtype=np.float64),
               burst_trj=np.concatenate(rec["trj"]).astype(np.int64),
               burst_trj_lengths=np.array([len(t) for t in rec["trj"]]),
               burst_u_init=np.array(rec["init"]))
    for k in ("trans", "bin", "jitter", "coin"):
        out["burst_u_" + k] = np.concatenate(rec[k])

    path = os.path.join(HERE, "kmc_golden.npz")
    np.savez_compressed(path, **out)
    print("kmc_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
