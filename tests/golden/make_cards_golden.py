#!/usr/bin/env python3
"""Generate tests/golden/cards_golden.npz by running the REAL reference's
enspara/cards/disorder.py (transition_stats, traj_ord_disord_times,
assign_order_disorder), cards.py (cards_matrices) and geometry/rotamer.py
(_rotamers) on seeded data.

    python tests/golden/make_cards_golden.py

make_golden.import_reference() builds the reference's extensions in a temporary
directory.  Only inputs and outputs are stored; no reference source is copied.

  rag_X [2268, 12] int8, rag_lengths (700, 1, 2, 65, 1500), 3 states: five ragged
      trajectories whose features switch in calm and busy stretches, feature j at a
      busy rate of 0.9 j / 11 (feature 0 never), feature 11 mostly every third
      frame with pauses (ord < dis)
      rag_times     [5, 12, 4] traj_ord_disord_times of every trajectory and feature
      rag_tt, rag_tt_counts   the transition times, flat, and how many per (traj, feature)
      rag_mean_ord, rag_mean_dis   transition_stats' means
      rag_D         [2268, 12] int8 assign_order_disorder's trajectories, concatenated
      rag_ss, rag_dd, rag_sd, rag_ds   cards_matrices(trajs, [3] * 12); rag_dd as the
                    reference gives it, divided by log(2) in float32 (its state numbers of
                    the disorder trajectories are int16, and numpy's log of an int16 is a
                    float32): _numpy_cards.dd_in_float64 undoes that
  rot_angles [1500, 3] float32: a random walk for phi, psi (raw, before the shift by
      100) and chi; rot_gates [330, 3]: a series that sits exactly on every gate and
      boundary (for psi: the raw angles whose shifted values do)
      rot_states, rot_gate_states   [3 kinds, 4 widths, frames] int16: _rotamers at the
      widths 0, 15, 15.5, 60 (psi on the angles shifted as psi_rotamers shifts them)

The generator checks the numpy restatement the GPU tests expect from
(tests/_numpy_cards.py) against the reference on all of it.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import import_reference  # noqa: E402
import _numpy_cards as nc  # noqa: E402

RAG_LENGTHS = (700, 1, 2, 65, 1500)
WIDTHS = (0, 15, 15.5, 60)
KINDS = ((nc.PHI, 0), (nc.PSI, 100), (nc.CHI, 0))


def switching(rng, frames, F, n):
    """calm and busy stretches; at a switch the state moves to another one"""
    X = np.zeros((frames, F), dtype=np.int8)
    rate = 0.9 * np.arange(F) / (F - 1)
    for j in range(F):
        busy = np.zeros(frames, dtype=bool)
        t = 0
        while t < frames:
            run = rng.randint(40, 160)
            busy[t:t + run] = rng.rand() < 0.4
            t += run
        p = np.where(busy, rate[j], 0.02 * rate[j])
        sw = rng.rand(frames) < p
        if j == F - 1:      # regular: every third frame, pauses of 20 now and then
            sw[:] = False
            t = 2
            while t < frames:
                sw[t] = True
                t += 20 if rng.rand() < 0.01 else 3
        cur = rng.randint(0, n)
        for t in range(frames):
            if sw[t]:
                cur = (cur + rng.randint(1, n)) % n
            X[t, j] = cur
    return X


def walk(rng, frames, step):
    a = np.cumsum(rng.normal(0, step, frames)) + rng.uniform(0, 360)
    a = np.mod(a, 360).astype(np.float32)
    a[a >= 360] = 0
    return a


def main():
    import_reference()
    from enspara.cards import disorder as rdis
    import enspara.cards as rcards
    from enspara.geometry import rotamer as rrot

    out = {}
    rng = np.random.RandomState(31)
    trajs = [switching(rng, T, 12, 3) for T in RAG_LENGTHS]
    out["rag_X"] = np.concatenate(trajs)
    out["rag_lengths"] = np.array(RAG_LENGTHS)
    tt, mean_ord, mean_dis = rdis.transition_stats(trajs)
    out["rag_mean_ord"], out["rag_mean_dis"] = mean_ord, mean_dis
    out["rag_tt"] = np.concatenate([np.concatenate(row) for row in tt]).astype(np.int32)
    out["rag_tt_counts"] = np.array([[len(c) for c in row] for row in tt])
    out["rag_times"] = np.array([[rdis.traj_ord_disord_times(c) for c in row] for row in tt],
                                dtype=np.float64)
    Ds, two = rdis.assign_order_disorder(trajs)
    assert np.all(two == 2) and two.dtype == np.int16 and Ds[0].dtype == np.int16
    out["rag_D"] = np.concatenate(Ds).astype(np.int8)
    share = out["rag_D"].mean()
    print("disordered share %.3f" % share)
    assert 0.05 < share < 0.95
    lower = (mean_ord < mean_dis) & (out["rag_tt_counts"].max(axis=0) > 1)
    assert lower.any(), "no feature with ord < dis"
    assert (out["rag_tt_counts"].sum(axis=0) == 0).any(), "no feature without transitions"
    mats = rcards.cards_matrices(trajs, np.full(12, 3))
    for k, m in zip(("rag_ss", "rag_dd", "rag_sd", "rag_ds"), mats):
        out[k] = m

    # the restatement against the reference
    assert np.array_equal(nc.mean_times(trajs)[0], mean_ord)
    assert np.array_equal(nc.mean_times(trajs)[1], mean_dis)
    for i, X in enumerate(trajs):
        for j in range(12):
            assert np.array_equal(nc.transition_times(X[:, j]), tt[i][j])
            assert nc.ord_disord_times(tt[i][j]) == tuple(out["rag_times"][i, j])
        assert np.array_equal(nc.disorder_codes(X, mean_ord, mean_dis), Ds[i])
    got, bounds, _, _ = nc.cards_matrices(trajs, np.full(12, 3))
    for k, (g, b, m) in enumerate(zip(got, bounds, mats)):
        if k == 1:      # the reference divides D-D by a float32 log 2 (its int16 state numbers)
            m = nc.dd_in_float64(m)
            b = b + 2 * nc.nm.U * np.abs(m)
        assert np.all(np.abs(g - m) <= b), k
    # a finite lower threshold that the data reaches
    j = np.where(lower)[0][-1]
    spans = np.diff(tt[4][j])
    r = nc.likelihood(mean_ord[j], mean_dis[j], spans.astype(np.int64))
    print("feature %d: ord %.3f < dis %.3f, spans %d .. %d, %d of %d disordered"
          % (j, mean_ord[j], mean_dis[j], spans.min(), spans.max(), (r >= 3).sum(), len(r)))
    assert (r >= 3).any() and (r < 3).any()

    rng = np.random.RandomState(32)
    out["rot_angles"] = np.stack([walk(rng, 1500, 25.0) for _ in KINDS], axis=1)
    series = np.array(nc.ON_GATES, dtype=np.float64)[rng.randint(0, len(nc.ON_GATES), 330)]
    out["rot_gates"] = np.stack([np.mod(series + s, 360) for _, s in KINDS],
                                axis=1).astype(np.float32)
    for key, res in (("rot_angles", "rot_states"), ("rot_gates", "rot_gate_states")):
        A = out[key]
        st = np.zeros((len(KINDS), len(WIDTHS), len(A)), dtype=np.int16)
        for k, (hb, shift) in enumerate(KINDS):
            a = A[:, k]
            if shift:       # as psi_rotamers: float32
                a = a - shift
                a[np.where(a < 0)] += 360
                assert a.dtype == np.float32
            assert a.max() < 360 and a.min() >= 0
            for w, width in enumerate(WIDTHS):
                st[k, w] = rrot._rotamers(a, hb, width)
                assert st[k, w].min() >= 0 and st[k, w].max() < len(hb) - 1
        out[res] = st
        for w, width in enumerate(WIDTHS):
            mine = nc.rotamer_states(A, [0, 1, 2], [k[0] for k in KINDS],
                                     [k[1] for k in KINDS], width)
            assert np.array_equal(mine.T, st[:, w]), (key, width)
    assert np.array_equal(nc.shifted(out["rot_gates"][:, 1], 100), series.astype(np.float32))

    path = os.path.join(HERE, "cards_golden.npz")
    np.savez_compressed(path, **out)
    print("cards_golden.npz", os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
