#!/usr/bin/env python3
"""Generate tests/golden/dye_bursts_golden.npz by running the REAL reference's burst-level
functions of enspara/geometry/dye_lifetimes.py and enspara/geometry/explicit_r0_calc.py
(mdtraj stubbed, as for the other goldens).

    python tests/golden/make_dye_bursts_golden.py

Only inputs and outputs are stored; no reference source is copied.

The reference draws with a generator and redraws non-radiative events; the library draws once
among the photon events.  Next to every sampled output this script therefore stores doubles
that make the library's pick land on what the reference accepted: it replays the reference's
generator (the replay is checked against the outputs), turns every accepted event into its rank
rho among the state's m photon events (or every drawn row into its index among the state's m
rows) and stores u = (rho + 1/2) / m.  The model (tests/_numpy_dye_bursts.py) fed those doubles
must return the reference's outputs; that is checked below as well.

  lt_lengths [6] (events per state: 1, 2, 5, 40, 40, 200), lt_life, lt_codes (flat), lt_states
      [200], lt_seed, lt_photons, lt_lifetimes (the reference's outputs), lt_u [200]
  ex_lengths, ex_photons, ex_life (flat, per burst), ex_FEs, ex_d_lengths, ex_d, ex_a_lengths, ex_a
  rm_lengths (lifetimes per state, some 0), rm_counts, rm_eqs_in, rm_tprobs, rm_eqs
  rd_len1, rd_len2 (conformations per state), rd_counts, rd_eqs_in, rd_eqs, rd_tprobs,
      rd_out_len1, rd_out_len2 (a removed state holds one row of zeros)
  sc_len_d, sc_len_a, sc_d, sc_a (flat [total, 9]), sc_states, sc_seed, sc_k2s, sc_rs, sc_ud,
      sc_ua
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import import_reference  # noqa: E402
import _numpy_dye_bursts as nb  # noqa: E402
import _numpy_dye_lifetimes as nd  # noqa: E402


def check(ok, what):
    if not ok:
        sys.exit("check failed: " + what)


def ragged(flat, lengths):
    off = np.concatenate([[0], np.cumsum(lengths)])
    return [flat[off[i]:off[i + 1]] for i in range(len(lengths))]


def main():
    import_reference()
    from enspara.geometry import explicit_r0_calc as rr0
    from enspara.geometry import dye_lifetimes as rdl
    out = {}
    rng = np.random.RandomState(43)

    # ---- the lifetime draw -------------------------------------------------------------------
    lengths = np.array([1, 2, 5, 40, 40, 200])
    codes = [rng.choice([0, 2], size=k) if k <= 2 else rng.choice(3, size=k, p=[0.3, 0.3, 0.4])
             for k in lengths]
    codes[3] = np.array([1] * 36 + [0, 2, 2, 0])
    rng.shuffle(codes[3])
    life = [np.round(rng.exponential(3.0, size=k), 3) for k in lengths]
    outcomes = [np.array([nd.OUTCOMES[c] for c in row], dtype=object) for row in codes]
    check(all(np.any(row != 1) for row in codes), "a state without a photon event")
    states = rng.randint(0, 6, size=200)
    states[:6] = np.arange(6)
    seed = 1234
    photons, lifetimes = rdl._sample_lifetimes_guarenteed_photon(states, life, outcomes,
                                                                rng_seed=seed)
    replay = np.random.default_rng(seed)
    u, redraws = np.empty(len(states)), 0
    for k, s in enumerate(states):
        e = replay.choice(len(life[s]))
        while codes[s][e] == 1:
            e = replay.choice(len(life[s]))
            redraws += 1
        check(life[s][e] == lifetimes[k] and int(codes[s][e] == 2) == photons[k],
              "the replay of default_rng(seed).choice, entry %d" % k)
        keep = np.flatnonzero(codes[s] != 1)
        u[k] = (int(np.searchsorted(keep, e)) + 0.5) / len(keep)
    check(redraws > 50, "the redraw loop was hardly taken")
    table = nb.event_table(list(zip(life, outcomes)))
    f, l, _ = nb.lifetime_photons(table, states, nb.RecordedUniforms({(nb.EVENT, 0): u}))
    check(np.array_equal(f, photons) and np.array_equal(l, lifetimes), "the lifetime model")
    out.update(lt_lengths=lengths, lt_life=np.concatenate(life),
               lt_codes=np.concatenate(codes).astype(np.int8), lt_states=states, lt_seed=seed,
               lt_photons=photons.astype(np.uint8), lt_lifetimes=lifetimes, lt_u=u)

    # ---- extract_fret_efficiency_lifetimes ---------------------------------------------------
    ex_lengths = np.array([1, 4, 9, 30, 2])
    ex_ph = [rng.randint(0, 2, size=k) for k in ex_lengths]
    ex_ph[0][:] = 1
    ex_lf = [np.round(rng.exponential(2.0, size=k), 3) for k in ex_lengths]
    sampling = np.empty((len(ex_lengths), 3), dtype=object)
    for i in range(len(ex_lengths)):
        sampling[i, 0], sampling[i, 1], sampling[i, 2] = ex_ph[i], ex_lf[i], np.zeros(1)
    FEs, d_l, a_l = rdl.extract_fret_efficiency_lifetimes(sampling)
    out.update(ex_lengths=ex_lengths, ex_photons=np.concatenate(ex_ph).astype(np.uint8),
               ex_life=np.concatenate(ex_lf), ex_FEs=np.asarray(FEs, dtype=np.float64),
               ex_d_lengths=np.array([len(x) for x in d_l]),
               ex_d=np.concatenate([np.asarray(x, dtype=np.float64) for x in d_l]),
               ex_a_lengths=np.array([len(x) for x in a_l]),
               ex_a=np.concatenate([np.asarray(x, dtype=np.float64) for x in a_l]))

    # ---- remake_prot_MSM_from_lifetimes --------------------------------------------------------
    rm_lengths = np.array([3, 0, 5, 2, 0, 4, 1])
    counts = rng.randint(1, 40, size=(7, 7))
    eqs_in = rng.dirichlet(np.ones(7))
    with tempfile.TemporaryDirectory() as tmp:
        tprobs, eqs = rdl.remake_prot_MSM_from_lifetimes(
            [np.ones(k) for k in rm_lengths], counts, (10, 20), ("dye one", "dye two"),
            outdir=tmp, prot_eqs=eqs_in)
    out.update(rm_lengths=rm_lengths, rm_counts=counts, rm_eqs_in=eqs_in,
               rm_tprobs=np.asarray(tprobs), rm_eqs=np.asarray(eqs))

    # ---- remove_dyeless_msm_states -------------------------------------------------------------
    len1, len2 = np.array([2, 3, 0, 1, 4, 2]), np.array([1, 0, 0, 2, 2, 3])
    c1 = [list(rng.randn(k, 9)) for k in len1]
    c2 = [list(rng.randn(k, 9)) for k in len2]
    counts6 = rng.randint(1, 40, size=(6, 6))
    eqs6 = rng.dirichlet(np.ones(6))
    r_eqs, r_tprobs, o1, o2 = rr0.remove_dyeless_msm_states(c1, c2, "one", "two", eqs6, counts6)
    check(all(np.all(np.asarray(o1[i]) == 0) and np.all(np.asarray(o2[i]) == 0)
              for i in (1, 2)), "placeholders")
    out.update(rd_len1=len1, rd_len2=len2, rd_counts=counts6, rd_eqs_in=eqs6,
               rd_eqs=np.asarray(r_eqs), rd_tprobs=np.asarray(r_tprobs),
               rd_out_len1=np.array([len(x) for x in o1]),
               rd_out_len2=np.array([len(x) for x in o2]))

    # ---- sample_dye_coords -----------------------------------------------------------------------
    len_d, len_a = np.array([1, 2, 7, 64, 65, 5]), np.array([1, 7, 2, 65, 64, 5])
    dc = [nd.random_coords(rng, k, (0.0, 0.0, 0.0)) for k in len_d]
    ac = [nd.random_coords(rng, k, (4.5, 1.0, 0.0)) for k in len_a]
    sc_states = rng.randint(0, 6, size=120)
    sc_seed = 99
    np.random.seed(sc_seed)
    k2s, rs = rr0.sample_dye_coords(dc, ac, sc_states)
    np.random.seed(sc_seed)
    ud, ua = np.empty(len(sc_states)), np.empty(len(sc_states))
    for k, s in enumerate(sc_states):
        i = np.random.choice(len(dc[s]))
        j = np.random.choice(len(ac[s]))
        k2, r = rr0.calc_k2_r(dc[s][i], ac[s][j])
        check(k2 == k2s[k] and r == rs[k], "the replay of np.random.choice, entry %d" % k)
        ud[k], ua[k] = (i + 0.5) / len(dc[s]), (j + 0.5) / len(ac[s])
    rec = nb.RecordedUniforms({(nb.DCONF, 0): ud, (nb.ACONF, 0): ua,
                               (nb.COIN, 0): np.zeros(len(sc_states))})
    m = nb.k2_photons(dc, ac, sc_states, 1.0, rec)
    check(np.all(np.abs(m[1] - k2s) <= 2 * nd.K2_ABS) and
          np.all(np.abs(m[2] - rs) <= 2 * nd.R_REL * rs), "the k2 model")
    out.update(sc_len_d=len_d, sc_len_a=len_a, sc_d=np.concatenate(dc), sc_a=np.concatenate(ac),
               sc_states=sc_states, sc_seed=sc_seed, sc_k2s=k2s, sc_rs=rs, sc_ud=ud, sc_ua=ua)

    path = os.path.join(HERE, "dye_bursts_golden.npz")
    np.savez_compressed(path, **out)
    print("dye_bursts_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
