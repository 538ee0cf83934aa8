"""explicit_r0_calc.map_dye_on_protein on the device (csrc/ek_dye_map.hip)
against tests/_numpy_dye_map.py and the float64 Kabsch model of tests/_numpy_rmsf.py.

No expected value comes from a device call, except where a later stage is checked GIVEN an
earlier stage's returned bits: the touch counts and the r / mu rows are held, exactly, to
the numpy model applied to the aligned coordinates the device returned
(``return_aligned``); the aligned coordinates themselves to ``frame_bound`` of the model.
"""
import functools

import numpy as np
import pytest

import _numpy_dye_map as dm
import _numpy_rmsf as nr

pytestmark = pytest.mark.gpu

PROBE, TOL = 0.04, 6        # TOL: counts == A - TOL and A - TOL - 1 both occur on every case below
# name -> (builder, arguments, g / (Gx + Gy) the model must reach, the bound it must stay below)
CASES = {
    "pep1": (dm.peptide_case, (1, 7), 0.22, 1.4e-5),
    "pep2": (dm.peptide_case, (2, 23), 0.22, 1.4e-5),
    "pep3": (dm.peptide_case, (3, 31), 0.22, 1.4e-5),
    "sel3": (dm.peptide_case, (4, 44, 96, 24, ("N", "CA", "C")), 2e-3, 1e-4),
    "sel4": (dm.peptide_case, (5, 52, 96, 24, ("N", "CA", "C", "O")), 2e-3, 1e-4),
    "sel16": (dm.window_case, (6, 58), 2e-3, 1e-4),
    "D1": (dm.peptide_case, (8, 7, 1), 0.2, 2e-5),
    "D63": (dm.peptide_case, (9, 23, 63), 0.2, 2e-5),
    "D64": (dm.peptide_case, (10, 31, 64), 0.2, 2e-5),
    "D65": (dm.peptide_case, (11, 44, 65), 0.2, 2e-5),
    "P1": (dm.peptide_case, (12, 52, 96, 24, dm.FIT_NAMES, 1), 0.2, 2e-5),
    "blob": (dm.blob_case, (7,), 0.2, 2e-5),
}


# conformations of 6 x 96 the float64 model keeps (computed on the CPU, from the model alone)
MODEL_KEEPS = {"pep1": 452, "pep2": 486, "pep3": 544}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _case(name):
    fn, args, _, _ = CASES[name]
    return _freeze(fn(*args))


@functools.lru_cache(maxsize=None)
def _models(name):
    c = _case(name)
    return [_freeze(dm.model_align(c["dye_xyz"], c["xyz"][p], c["prot_sel"], c["dye_sel"]))
            for p in range(len(c["xyz"]))]


@functools.lru_cache(maxsize=None)
def _device(name):
    from enspara_amd.geometry import explicit_r0_calc as r0c
    return r0c.map_dye_on_protein(probe_radius=PROBE, atom_tol=TOL, return_aligned=True,
                                  **_case(name))


def _bits(m):
    return (m.counts.tobytes(), m.coords_all.tobytes(),
            None if m.aligned is None else m.aligned.tobytes(),
            [k.tobytes() for k in m.kept], [c.tobytes() for c in m.coords])


def _assert_conditioned(name):
    _, _, ratio, cap = CASES[name]
    worst = 0.0
    for m in _models(name):
        assert (m["g"] / m["G"]).min() >= ratio, float((m["g"] / m["G"]).min())
        b = nr.frame_bound(m)
        nr.assert_bound_is_tight(m, b)
        worst = max(worst, float(b.max()))
    assert worst <= cap, worst


# ---- 1. the alignment --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pep1", "pep2", "pep3", "sel3", "sel4", "sel16", "blob"])
def test_alignment_against_the_float64_model(name):
    _assert_conditioned(name)
    c, got = _case(name), _device(name)
    P, (D, A) = len(c["xyz"]), c["dye_xyz"].shape[:2]
    assert got.aligned.dtype == np.float32 and got.aligned.shape == (P, D, A, 3)
    worst = 0.0
    for p, m in enumerate(_models(name)):
        bound = nr.frame_bound(m)
        err = np.abs(got.aligned[p].astype(np.float64) - m["aligned"]).max(axis=(1, 2))
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (p, int((err / bound).argmax()), float((err / bound).max()))
    print("%s: worst error / bound %.3g" % (name, worst))


# ---- 2. counts and r / mu on the returned bits -------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_counts_and_r_mu_are_exact_on_the_returned_bits(name):
    c, got = _case(name), _device(name)
    P, (D, A) = len(c["xyz"]), c["dye_xyz"].shape[:2]
    cutoff = c["radii"] + PROBE
    assert got.counts.dtype == np.int32 and got.counts.shape == (P, D)
    assert got.coords_all.dtype == np.float64 and got.coords_all.shape == (P, D, 9)
    assert len(got.coords) == len(got.kept) == len(got) == P
    from enspara_amd.geometry import explicit_r0_calc as r0c
    for p in range(P):
        want = dm.touch_counts(got.aligned[p], c["xyz"][p], cutoff, c["exclude_atoms"])
        assert np.array_equal(got.counts[p], want), (p, np.flatnonzero(got.counts[p] != want)[:5])
        assert got.kept[p].dtype == np.int64
        assert np.array_equal(got.kept[p], np.flatnonzero(got.counts[p] >= A - TOL))
        rows = r0c.dye_r_mu(got.aligned[p], c["r_atom"], c["mu_atoms"]).astype(np.float64)
        assert np.array_equal(rows, dm.r_mu(got.aligned[p], c["r_atom"], c["mu_atoms"]))
        assert got.coords_all[p].tobytes() == rows.tobytes()
        assert got.coords[p].tobytes() == rows[got.kept[p]].tobytes()


def _host_cull(c):
    """the atoms inside explicit_r0_calc.cull_radius, which tests/test_dye_map_host.py holds
    to 'no atom outside can touch': the device's lists must be exactly these"""
    from enspara_amd.geometry import explicit_r0_calc as r0c
    reach, out = r0c.dye_reach(c["dye_xyz"], c["dye_sel"]), []
    for x in c["xyz"].astype(np.float64):
        c_ref = x[c["prot_sel"]].mean(axis=0)
        inside = np.sqrt(((x - c_ref) ** 2).sum(axis=1)) <= r0c.cull_radius(
            reach, c_ref, c["radii"] + PROBE)
        inside[c["exclude_atoms"]] = False
        out.append(int(inside.sum()))
    return out


def test_the_fixtures_reach_both_sides_of_the_verdict_and_both_cull_regimes():
    atoms = _case("pep1")["xyz"].shape[1]
    for name in ("pep1", "pep2", "pep3"):
        got, A = _device(name), _case(name)["dye_xyz"].shape[1]
        assert (got.counts == A - TOL).any() and (got.counts == A - TOL - 1).any()
        # the peptide is longer than the dye: the cull drops atoms
        assert got.list_len.shape == (6,) and (got.list_len < atoms - 5).all(), got.list_len
        assert (got.list_len > 0).all()
        assert got.list_len.tolist() == _host_cull(_case(name)), name
    blob = _device("blob")
    assert blob.list_len[0] > 1024, blob.list_len       # two LDS batches at least
    # a conformation of 70 atoms spans waves, and 130 x 70 lanes many workgroups
    assert _case("blob")["dye_xyz"].shape[:2] == (130, 70)


# ---- 3. end to end -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pep1", "pep2", "pep3"])
def test_end_to_end_against_the_float64_model(name):
    _assert_conditioned(name)
    c = _case(name)
    P, (D, A) = len(c["xyz"]), c["dye_xyz"].shape[:2]
    cutoff = c["radii"] + PROBE
    ranges = [dm.count_range(m["aligned"], nr.frame_bound(m), c["xyz"][p], cutoff,
                             c["exclude_atoms"]) for p, m in enumerate(_models(name))]
    undecided = sum(int(((lo >= A - TOL) != (hi >= A - TOL)).sum()) for lo, hi, _ in ranges)
    assert undecided <= 0.01 * P * D, undecided
    # the fixture recipe, pinned from the model alone: no verdict is undecided, and it keeps
    # this many of the 576 conformations
    assert undecided == 0
    assert sum(int((model >= A - TOL).sum()) for _, _, model in ranges) == MODEL_KEEPS[name]
    got = _device(name)
    n_kept = 0
    for p, (lo, hi, model) in enumerate(ranges):
        cnt = got.counts[p]
        assert np.all((cnt >= lo) & (cnt <= hi)), (p, np.flatnonzero((cnt < lo) | (cnt > hi))[:5])
        sure = lo == hi
        assert np.array_equal(cnt[sure], model[sure])
        decided = (lo >= A - TOL) == (hi >= A - TOL)
        verdict = np.zeros(D, dtype=bool)
        verdict[got.kept[p]] = True
        assert np.array_equal(verdict[decided], (model >= A - TOL)[decided])
        n_kept += int(verdict.sum())
    print("%s: %d undecided verdicts of %d, %d kept" % (name, undecided, P * D, n_kept))
    assert n_kept == MODEL_KEEPS[name]


# ---- 4. comparison direction -------------------------------------------------------------------
def test_a_distance_equal_to_the_cutoff_touches():
    from enspara_amd.geometry import explicit_r0_calc as r0c
    frame = np.array([[0, 0, 0], [5, 0, 0]], dtype=np.float32)
    radii = np.array([0.25, 0.25])          # + 0.125: 0.375 exactly
    at = np.float32(0.375)
    dye = np.array([[[at, 0, 0]], [[np.nextafter(at, np.float32(1))]  + [0, 0]], [[5, 0, 0]],
                    [[0, -at, 0]], [[0, 0, np.nextafter(at, np.float32(1))]]], dtype=np.float32)
    assert np.float64(at) == 0.375 and radii[0] + 0.125 == 0.375
    kept = r0c.remove_touches_protein_dye_traj(frame, radii, dye, [1], probe_radius=0.125, atom_tol=0)
    assert kept.dtype == np.int64 and kept.tolist() == [1, 2, 4]
    # the atom that only the excluded atom covers is free; without the exclusion it touches
    assert r0c.remove_touches_protein_dye_traj(frame, radii, dye, [], probe_radius=0.125,
                                               atom_tol=0).tolist() == [1, 4]
    # with one touching atom tolerated everything stays
    assert r0c.remove_touches_protein_dye_traj(frame, radii, dye, [], probe_radius=0.125,
                                               atom_tol=1).tolist() == [0, 1, 2, 3, 4]
    # the model says the same
    want = [int(dm.touch_counts(dye, frame, radii + 0.125, [1])[d]) for d in range(5)]
    assert want == [0, 1, 1, 0, 1]


# ---- 5. reach ----------------------------------------------------------------------------------
def test_an_atom_at_the_tip_of_a_straight_tail_is_not_culled():
    from enspara_amd.geometry import explicit_r0_calc as r0c
    rng = np.random.RandomState(5)
    A = 24
    res = np.array([dm.LOCAL[n] for n in ("N", "CA", "C", "O", "CB")]) + 3.0
    tmpl = np.array([dm.LOCAL[n] for n in dm.FIT_NAMES])
    away = tmpl[2] - tmpl.mean(axis=0)
    away /= np.linalg.norm(away)
    straight = np.concatenate([tmpl, tmpl[2] + 0.14 * np.arange(1, A - 4)[:, None] * away])
    dye = (straight @ dm.random_rotation(rng).T + rng.randn(3))[None].astype(np.float32)
    prot_sel, dye_sel = dm.residue_sel(1), np.arange(5, dtype=np.int32)
    frame0 = res.astype(np.float32)
    m = dm.model_align(dye, frame0, prot_sel, dye_sel)
    c_ref = frame0[prot_sel].astype(np.float64).mean(axis=0)
    tip = m["aligned"][0, A - 1]
    out = (tip - c_ref) / np.linalg.norm(tip - c_ref)
    atom = (tip + 0.05 * out).astype(np.float32)            # 0.05 nm beyond the tip
    frame = np.concatenate([frame0, atom[None]])
    radii = np.full(6, 0.17)
    reach = r0c.dye_reach(dye, dye_sel)
    dist = np.linalg.norm(atom.astype(np.float64) - c_ref)
    assert reach < dist < reach + 0.06      # farther from the attachment than any dye atom
    assert abs(np.linalg.norm(tip - c_ref) - reach) < 1e-6      # the tip is what sets the reach
    lo, hi, model = dm.count_range(m["aligned"], nr.frame_bound(m), frame, radii + PROBE,
                                   dm.residue_atoms(1))
    assert lo[0] == hi[0] == model[0] == A - 2      # the tip and the atom before it (0.19 nm)
    got = r0c.map_dye_on_protein(frame[None], radii, dye, prot_sel, dye_sel, dm.residue_atoms(1),
                                 A - 1, (A - 2, A - 3), probe_radius=PROBE, atom_tol=0)
    assert got.list_len.tolist() == [1]
    assert got.counts.tolist() == [[A - 2]] and got.kept[0].size == 0 and got.coords[0].shape == (0, 9)
    assert r0c.find_dyeless_states(got.coords).tolist() == [0]


# ---- 6. chunking -------------------------------------------------------------------------------
def test_chunks_and_repeats_give_identical_bits():
    from enspara_amd.geometry import explicit_r0_calc as r0c
    want = _bits(_device("pep2"))
    for chunk in (1, 4, None):
        got = r0c.map_dye_on_protein(probe_radius=PROBE, atom_tol=TOL, return_aligned=True,
                                     chunk_centres=chunk, **_case("pep2"))
        assert _bits(got) == want, chunk
    plain = r0c.map_dye_on_protein(probe_radius=PROBE, atom_tol=TOL, chunk_centres=4,
                                   **_case("pep2"))
    assert plain.aligned is None and _bits(plain)[:2] == want[:2] and _bits(plain)[3:] == want[3:]


# ---- 7. a fit that is not determined -----------------------------------------------------------
def test_a_collinear_selection_is_refused_by_name():
    from enspara_amd import exception
    from enspara_amd.geometry import explicit_r0_calc as r0c
    c = dict(_case("pep1"))
    dye = c["dye_xyz"].copy()
    dye[5, :5] = dye[5, 0] + 0.1 * np.arange(5, dtype=np.float32)[:, None] * \
        np.array([0.6, 0.0, 0.8], dtype=np.float32)
    c["dye_xyz"] = dye
    m = dm.model_align(dye[5:6], c["xyz"][0], c["prot_sel"], c["dye_sel"])
    assert m["g"][0] / m["G"][0] <= nr.DEGENERATE_RATIO
    with pytest.raises(exception.DataInvalid, match=r"conformation 5 on centre 0 .*6 such"):
        r0c.map_dye_on_protein(**c)


# ---- 8. composition ----------------------------------------------------------------------------
def test_align_full_dye_to_res_is_the_maps_alignment():
    from enspara_amd.geometry import explicit_r0_calc as r0c
    c, got = _case("pep3"), _device("pep3")
    for p in (0, 4):
        al = r0c.align_full_dye_to_res(c["xyz"][p], c["dye_xyz"], c["prot_sel"], c["dye_sel"])
        assert al.dtype == np.float32 and al.tobytes() == got.aligned[p].tobytes()
    # and the touch step alone, on those coordinates, is the map's verdict
    kept = r0c.remove_touches_protein_dye_traj(c["xyz"][4], c["radii"], got.aligned[4],
                                               c["exclude_atoms"], probe_radius=PROBE, atom_tol=TOL)
    assert np.array_equal(kept, got.kept[4])


def test_maps_feed_calc_lifetimes_many():
    from enspara_amd.geometry import dye_lifetimes as dl
    from enspara_amd.geometry import explicit_r0_calc as r0c
    params, lag = (2.5e15, 0.92, 4.1), 0.2
    d_case, a_case = dm.peptide_case(1, 7, D=12, P=3), dm.peptide_case(1, 44, D=12, P=3)
    assert np.array_equal(d_case["xyz"], a_case["xyz"])        # one protein, two residues
    d_map = r0c.map_dye_on_protein(probe_radius=PROBE, atom_tol=TOL, **d_case)
    a_map = r0c.map_dye_on_protein(probe_radius=PROBE, atom_tol=TOL, **a_case)
    assert all(len(k) >= 2 for k in d_map.kept + a_map.kept)
    rng = np.random.RandomState(0)
    d_t, a_t = rng.randint(1, 9, (12, 12)), rng.randint(1, 9, (12, 12))
    centres = dl.centres_from_maps(d_map, d_t, a_map, a_t)
    got = dl.calc_lifetimes_many(centres, params, lag, n_samples=64, random_state=11)
    by_hand = dl.calc_lifetimes_many(
        [(d_map.coords_all[p], d_t, d_map.kept[p], a_map.coords_all[p], a_t, a_map.kept[p])
         for p in range(3)], params, lag, n_samples=64, random_state=11)
    assert len(got) == 3
    for (t1, o1), (t2, o2) in zip(got, by_hand):
        assert len(t1) == 64 and np.array_equal(t1, t2) and list(o1) == list(o2)
    # and the kept rows feed the burst stage's containers
    k2s, rs = r0c.sample_dye_coords(d_map.coords, a_map.coords, [0, 1, 2, 1], random_state=3)
    assert k2s.shape == rs.shape == (4,) and np.all(np.isfinite(k2s)) and np.all(rs > 0)
