#!/usr/bin/env python3
"""Generate tests/golden/dye_lifetimes_golden.npz by running the REAL reference's
enspara/geometry/dye_lifetimes.py and the array-only functions of its
enspara/geometry/explicit_r0_calc.py (mdtraj stubbed, as for the other goldens).

    python tests/golden/make_dye_lifetimes_golden.py

Only inputs and outputs are stored; no reference source is copied.

The reference's functions take mdtraj trajectories and dye names and turn them into [n, 9]
arrays with ``assemble_dye_r_mu``; here that one function is replaced by the identity while
the reference runs, so the "centres" passed in are those arrays.  Its samplers take an
``rng_seed``; next to every output this script stores the doubles ``default_rng(seed)``
hands out, in the order the reference consumes them, replayed from the same seed:
  resolve_excitation      donor initial state, acceptor initial state, then per step the
                          decay channel, the donor hop, the acceptor hop
  explicit_static_dyes    n donor states, n acceptor states, then a coin per sample
The consumption order is checked below: the model (tests/_numpy_dye_lifetimes.py) fed these
doubles must give the recorded outputs.  fully_averaged_explict_dyes is recorded for its
k2s, FEs and eqs only (its coins are compared with the loop's last FE, not their mean).

  dye_params (J, Qd, Td), lagtime
  mc_{d,a}_coords, mc_{d,a}_T (zeros in the rows), mc_{d,a}_eqs: the 7 x 5 pair
  mc_seeds, mc_steps, mc_outcomes (codes), mc_lengths (steps + 1), mc_dtraj, mc_atraj (flat),
  mc_u (flat, 2 + 3 steps per seed)
  cl_{d,a}_coords: a 3 x 2 pair less than 1 nm apart; cl_pairs [3, 2, 4] = the reference's
      k2, r, R0, kRET of every pair of states; cl_raised [3, 2]: the pairs at which its
      calc_energy_transfer_prob reaches the renormalised branch (see below: it raises there)
  st_d_eqs (one zero), st_a_eqs, st_seed, st_n, st_outcomes (codes), st_u (flat 3 n)
  iso_k2s, iso_FEs, iso_eqs, iso_avg
  k2r_d, k2r_a [n, 9], k2r_k2, k2r_r; r0_k2, r0_out; fr_r, fr_R0, fr_out; rates (Qd, Td, krad,
  knr); etp_in [m, 4], etp_out [m, 4]; rbs_counts, rbs_bad, rbs_out; fds_lengths, fds_out;
  psfe_codes [3, k] (-1 pads; a state without events is all -1), psfe_out
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import import_reference  # noqa: E402
import _numpy_dye_lifetimes as nd  # noqa: E402

PARAMS = (2.5e15, 0.92, 4.1)
LAG = 0.2
CODES = {name: k for k, name in enumerate(nd.OUTCOMES)}


def check(ok, what):
    if not ok:
        sys.exit("check failed: " + what)


def monte_carlo(rdl, tag, d, a, seeds, out):
    (dc, dT, de), (ac, aT, ae) = d, a
    K = nd.consts(PARAMS, LAG)
    rec = {k: [] for k in ("steps", "outcomes", "dtraj", "atraj", "u")}
    for s in seeds:
        steps, outcome, dtrj, atrj = rdl.resolve_excitation(
            "D", "A", dT, aT, de, ae, dc, ac, PARAMS, LAG, None, rng_seed=int(s))
        u = np.random.default_rng(int(s)).random(2 + 3 * steps)
        table = {(nd.DONOR, 0): np.concatenate([u[0:1], u[3::3]]),
                 (nd.ACCEPTOR, 0): np.concatenate([u[1:2], u[4::3]]), (nd.DECAY, 0): u[2::3]}
        m = nd.resolve(dc, dT, de, ac, aT, ae, K, 1, nd.RecordedUniforms(table), block=1)
        check(m[0][0] == steps and nd.OUTCOMES[m[1][0]] == outcome and
              np.array_equal(m[2][0], dtrj) and np.array_equal(m[3][0], atrj),
              "%s model, seed %d" % (tag, s))
        for k, v in (("steps", steps), ("outcomes", CODES[str(outcome)]), ("dtraj", dtrj),
                     ("atraj", atrj), ("u", u)):
            rec[k].append(v)
    out.update({tag + "_d_coords": dc, tag + "_d_T": dT, tag + "_d_eqs": de,
                tag + "_a_coords": ac, tag + "_a_T": aT, tag + "_a_eqs": ae,
                tag + "_seeds": np.asarray(seeds), tag + "_steps": np.array(rec["steps"]),
                tag + "_outcomes": np.array(rec["outcomes"], dtype=np.int8),
                tag + "_lengths": np.array(rec["steps"]) + 1,
                tag + "_dtraj": np.concatenate(rec["dtraj"]).astype(np.int64),
                tag + "_atraj": np.concatenate(rec["atraj"]).astype(np.int64),
                tag + "_u": np.concatenate(rec["u"])})
    return np.array(rec["steps"])


def main():
    import_reference()
    from enspara.geometry import explicit_r0_calc as rr0
    from enspara.geometry import dye_lifetimes as rdl
    rr0.assemble_dye_r_mu = lambda centers, name, library: np.asarray(centers)

    out = {"dye_params": np.array(PARAMS), "lagtime": LAG}
    rng = np.random.RandomState(41)

    # ---- the 7 x 5 pair --------------------------------------------------------------------
    dT, de = nd.random_msm(rng, 7, 4)
    aT, ae = nd.random_msm(rng, 5, 3)
    dc = nd.random_coords(rng, 7, (0.0, 0.0, 0.0), spread=0.5)
    ac = nd.random_coords(rng, 5, (5.2, 0.5, 0.0), spread=0.5)
    steps = monte_carlo(rdl, "mc", (dc, dT, de), (ac, aT, ae), np.arange(100, 140), out)
    print("7 x 5: mean steps %.1f, longest %d" % (steps.mean(), steps.max()))

    # ---- a close pair: the renormalised branch ---------------------------------------------
    # With numpy >= 1.24 the reference cannot leave this branch: it builds an array of three
    # scalars and an np.zeros(1) and numpy raises ValueError.  What is recorded is therefore
    # everything up to the branch, from the reference's own functions (k2, r, R0, kRET per pair
    # of states) and that the branch is reached (the ValueError); its result, [p_rad, p_nonrad,
    # p_RET, 0] / sum, is pinned by formula in the host test.
    cc = nd.random_coords(rng, 3, (0.0, 0.0, 0.0), spread=0.1)
    ec = nd.random_coords(rng, 2, (0.7, 0.0, 0.0), spread=0.1)
    krad, knr = rdl.calc_dye_radiative_rates(PARAMS[1], PARAMS[2])
    pairs, raised = np.zeros((3, 2, 4)), np.zeros((3, 2), dtype=bool)
    for i in range(3):
        for j in range(2):
            k2, r = rr0.calc_k2_r(cc[i], ec[j])
            R0 = rr0.calc_R0(k2, PARAMS[1], PARAMS[0])
            kret = rdl.FRET_rate(r, R0, PARAMS[2])
            pairs[i, j] = k2, r, R0, kret
            try:
                p = rdl.calc_energy_transfer_prob(krad, knr, kret, LAG)
                check(p[3] >= 0, "a negative probability came back")
            except ValueError:
                raised[i, j] = True
    check(raised.any(), "no pair of the close problem takes the renormalised branch")
    out.update(cl_d_coords=cc, cl_a_coords=ec, cl_pairs=pairs, cl_raised=raised)

    # ---- static, with a zero eq prob ---------------------------------------------------------
    se = de.copy()
    se[2] = 0.0
    se /= se.sum()
    n = 50
    events = rdl.explicit_static_dyes("D", "A", se, ae, dc, ac, PARAMS, None, n_samples=n,
                                      rng_seed=77)
    u = np.random.default_rng(77).random(3 * n)
    codes = np.array([CODES[e[1]] for e in events], dtype=np.int8)
    table = {}
    for j in range(n):
        table[(nd.DONOR, j)], table[(nd.ACCEPTOR, j)] = [u[j]], [u[n + j]]
        table[(nd.FRET_COIN, j)] = [u[2 * n + j]]
    acc, ds, _, _ = nd.static(dc, se, ac, ae, nd.consts(PARAMS, LAG), n,
                              nd.RecordedUniforms(table))
    check(np.array_equal(acc * 2, codes) and not np.any(ds == 2), "static model")
    out.update(st_d_eqs=se, st_a_eqs=ae, st_seed=77, st_n=n, st_outcomes=codes, st_u=u)

    # ---- isotropic ---------------------------------------------------------------------------
    _, _, k2s, FEs, eqs = rdl.fully_averaged_explict_dyes("D", "A", se, ae, dc, ac, PARAMS, None,
                                                          n_samples=5, rng_seed=3)
    out.update(iso_k2s=k2s, iso_FEs=FEs, iso_eqs=eqs, iso_avg=np.average(FEs, weights=eqs))
    m = nd.isotropic(dc, se, ac, ae, nd.consts(PARAMS, LAG), 5, nd.PhiloxUniforms(1))
    check(np.allclose(m[1], k2s, rtol=0, atol=2 * nd.K2_ABS) and
          np.allclose(m[2], FEs, rtol=0, atol=1e-12) and np.array_equal(m[3], eqs),
          "isotropic model")

    # ---- the numpy helpers -------------------------------------------------------------------
    kd = nd.random_coords(rng, 12, (0.0, 0.0, 0.0))
    ka = nd.random_coords(rng, 12, (3.0, 1.0, -2.0))
    k2r = np.array([rr0.calc_k2_r(kd[i], ka[i]) for i in range(12)])
    out.update(k2r_d=kd, k2r_a=ka, k2r_k2=k2r[:, 0], k2r_r=k2r[:, 1])
    out["r0_k2"] = rng.rand(9) * 4
    out["r0_out"] = rr0.calc_R0(out["r0_k2"], PARAMS[1], PARAMS[0])
    out["fr_r"], out["fr_R0"] = rng.rand(9) * 8 + 0.5, rng.rand(9) * 3 + 3
    out["fr_out"] = rdl.FRET_rate(out["fr_r"], out["fr_R0"], PARAMS[2])
    out["rates"] = np.array([PARAMS[1], PARAMS[2], krad, knr])
    etp_in = np.array([[krad, knr, kret, LAG] for kret in (0.0, 1e-3, 0.5, 3.0, 4.0)])
    out["etp_in"] = etp_in
    out["etp_out"] = np.array([rdl.calc_energy_transfer_prob(*row) for row in etp_in])
    counts = rng.randint(0, 9, size=(6, 6))
    out.update(rbs_counts=counts, rbs_bad=np.array([1, 4]),
               rbs_out=rr0.remove_bad_states(np.array([1, 4]), counts))
    check(np.array_equal(rr0.remove_bad_states(np.array([]), counts), counts), "no bad state")
    lengths = [2, 0, 3, 0, 0, 1]
    out.update(fds_lengths=np.array(lengths),
               fds_out=rr0.find_dyeless_states([list(range(k)) for k in lengths]))
    codes = np.array([[0, 2, 2, 1, 0, 2], [-1] * 6, [2, 2, 2, 1, 1, 0]])
    events = np.empty((3, 2), dtype="O")
    for i, row in enumerate(codes):
        names = np.array([nd.OUTCOMES[c] for c in row if c >= 0], dtype="O")
        events[i, 0], events[i, 1] = np.zeros(len(names)), names
    out.update(psfe_codes=codes, psfe_out=rdl.calc_per_state_FE(events))

    path = os.path.join(HERE, "dye_lifetimes_golden.npz")
    np.savez_compressed(path, **out)
    print("dye_lifetimes_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
