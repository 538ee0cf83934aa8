"""Host tests of the dye mapping (no GPU).

1. The numpy model (tests/_numpy_dye_map.py) against the goldens recorded from the
   reference's remove_touches_protein_dye_traj and assemble_dye_r_mu
   (tests/golden/make_dye_map_golden.py): kept indices, counts, r / mu rows.
2. Every input ``map_dye_on_protein`` and its two steps refuse, refused with
   ``DataInvalid`` before any device call (there is no device here: reaching one would
   raise something else).
3. The ragged assembly and ``dye_lifetimes.centres_from_maps`` give what the later stages
   accept; a centre that keeps nothing gives ``([0], [0], [])`` and shows up in
   ``find_dyeless_states``.
4. The cull radius: no atom outside it is within its cutoff of a model-aligned dye atom plus
   the frame bound, and the margin holds, and is no wider than needed, at its own scale.
"""
import os

import numpy as np
import pytest

import _numpy_dye_map as dm
import _numpy_rmsf as nr
from enspara_amd import exception
from enspara_amd.geometry import dye_lifetimes as dl
from enspara_amd.geometry import explicit_r0_calc as r0c


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "dye_map_golden.npz"))


def _exclude(golden):
    return np.flatnonzero(golden["pep_seqs"] == int(golden["resseq"]))


# ---- 1. the model is the reference ---------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_model_counts_and_kept_equal_the_reference(golden, k):
    xyz, aligned, radii = golden["pep_xyz"], golden["aligned"], golden["pep_radii"]
    probe, tol = float(golden["case%d_probe" % k]), int(golden["case%d_tol" % k])
    off = golden["case%d_kept_off" % k]
    A = aligned.shape[2]
    for p in range(len(xyz)):
        counts = dm.touch_counts(aligned[p], xyz[p], radii + probe, _exclude(golden))
        assert np.array_equal(counts, golden["case%d_counts" % k][p])
        assert np.array_equal(dm.kept(counts, A, tol), golden["case%d_kept" % k][off[p]:off[p + 1]])


def test_model_r_mu_equals_the_reference_and_dye_r_mu(golden):
    aligned = golden["aligned"]
    r_atom, mu = int(golden["r_atom"]), tuple(int(v) for v in golden["mu_atoms"])
    # the library lists the dipole's atoms in descending order; select returns them ascending
    names = list(golden["dye_names"])
    assert [names.index(n) for n in golden["mu_names"]] == [mu[1], mu[0]] and mu[0] < mu[1]
    for p in range(len(aligned)):
        want = golden["rmu"][p]
        assert np.array_equal(dm.r_mu(aligned[p], r_atom, mu), want)
        got = r0c.dye_r_mu(aligned[p], r_atom, mu)
        assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)


def test_excluded_atoms_matter_in_the_golden(golden):
    """without the exclusion the residue's own atoms touch: the fixture can tell"""
    xyz, aligned, radii = golden["pep_xyz"], golden["aligned"], golden["pep_radii"]
    with_res = dm.touch_counts(aligned[1], xyz[1], radii + 0.04)
    assert (with_res < golden["case0_counts"][1]).any()


# ---- 2. DataInvalid before any device call -----------------------------------------------------
def _good():
    c = dm.peptide_case(1, 7, D=4, A=8, P=2)
    c["mu_atoms"] = (5, 2)
    return c


def _bad_cases():
    nan_xyz = _good()["xyz"].copy()
    nan_xyz[1, 3, 0] = np.nan
    inf_dye = _good()["dye_xyz"].copy()
    inf_dye[0, 0, 2] = np.inf
    far = _good()["xyz"].copy()
    far[0, 0, 0] = 2.0 ** 21
    atoms = _good()["xyz"].shape[1]
    return [
        ("xyz shape", dict(xyz=_good()["xyz"][0])),
        ("xyz dtype", dict(xyz=_good()["xyz"].astype(np.float64))),
        ("xyz nan", dict(xyz=nan_xyz)),
        ("xyz beyond 2^20", dict(xyz=far)),
        ("dye shape", dict(dye_xyz=_good()["dye_xyz"][:, :, :2])),
        ("dye dtype", dict(dye_xyz=_good()["dye_xyz"].astype(np.float64))),
        ("dye inf", dict(dye_xyz=inf_dye)),
        ("no conformations", dict(dye_xyz=_good()["dye_xyz"][:0])),
        ("radii shape", dict(radii=np.ones(atoms + 1))),
        ("radii nan", dict(radii=np.full(atoms, np.nan))),
        ("radius + probe <= 0", dict(radii=np.zeros(atoms), probe_radius=0.0)),
        ("radius + probe < 0", dict(probe_radius=-1.0)),
        ("probe not a number", dict(probe_radius="wide")),
        ("prot_sel out of range", dict(prot_sel=[0, 1, 2, 3, atoms])),
        ("prot_sel negative", dict(prot_sel=[-1, 1, 2, 3, 4])),
        ("prot_sel repeated", dict(prot_sel=[0, 1, 1, 3, 4])),
        ("dye_sel out of range", dict(dye_sel=[0, 1, 2, 3, 8])),
        ("dye_sel repeated", dict(dye_sel=[0, 1, 2, 2, 4])),
        ("unequal selections", dict(dye_sel=[0, 1, 2, 3])),
        ("two atoms", dict(prot_sel=[0, 1], dye_sel=[0, 1])),
        ("seventeen atoms", dict(prot_sel=list(range(17)), dye_sel=list(range(17)))),
        ("float selection", dict(prot_sel=[0.0, 1.0, 2.0, 3.0, 4.0])),
        ("exclude out of range", dict(exclude_atoms=[atoms])),
        ("exclude repeated", dict(exclude_atoms=[3, 3])),
        ("r_atom out of range", dict(r_atom=8)),
        ("mu_atoms out of range", dict(mu_atoms=(1, 9))),
        ("mu_atoms equal", dict(mu_atoms=(2, 2))),
        ("three mu_atoms", dict(mu_atoms=(1, 2, 3))),
        ("atom_tol negative", dict(atom_tol=-1)),
        ("atom_tol above A", dict(atom_tol=9)),
        ("atom_tol float", dict(atom_tol=2.0)),
        ("atom_tol bool", dict(atom_tol=True)),
        ("chunk_centres zero", dict(chunk_centres=0)),
        ("chunk_centres float", dict(chunk_centres=1.5)),
    ]


@pytest.mark.parametrize("what,change", _bad_cases(), ids=[c[0] for c in _bad_cases()])
def test_invalid_input_raises_before_any_device_call(what, change):
    kw = _good()
    kw.update(change)
    with pytest.raises(exception.DataInvalid):
        r0c.map_dye_on_protein(**kw)


def test_the_two_steps_validate_too():
    c = _good()
    frame = c["xyz"][0]
    with pytest.raises(exception.DataInvalid):
        r0c.align_full_dye_to_res(c["xyz"], c["dye_xyz"], c["prot_sel"], c["dye_sel"])
    with pytest.raises(exception.DataInvalid):
        r0c.align_full_dye_to_res(frame, c["dye_xyz"], c["prot_sel"], c["dye_sel"][:4])
    with pytest.raises(exception.DataInvalid):
        r0c.align_full_dye_to_res(frame.astype(np.float64), c["dye_xyz"], c["prot_sel"], c["dye_sel"])
    with pytest.raises(exception.DataInvalid):
        r0c.remove_touches_protein_dye_traj(frame, c["radii"][:-1], c["dye_xyz"], [])
    with pytest.raises(exception.DataInvalid):
        r0c.remove_touches_protein_dye_traj(frame, c["radii"], c["dye_xyz"], [], atom_tol=9)
    with pytest.raises(exception.DataInvalid):
        r0c.remove_touches_protein_dye_traj(frame, c["radii"], c["dye_xyz"], [len(frame)])
    with pytest.raises(exception.DataInvalid):
        r0c.remove_touches_protein_dye_traj(c["xyz"], c["radii"], c["dye_xyz"], [])


def test_atom_tol_limits_are_valid():
    """0 and A are allowed: they pass validation (and then need the device)"""
    for tol in (0, 8):
        kw = _good()
        out = r0c._map_inputs(kw["xyz"], kw["radii"], kw["dye_xyz"], kw["prot_sel"], kw["dye_sel"],
                              kw["exclude_atoms"], kw["r_atom"], kw["mu_atoms"], 0.04, tol, None)
        assert out[9] == tol and out[6:9] == (7, 5, 2)


# ---- 3. assembly ---------------------------------------------------------------------------------
def _golden_map(golden, k):
    counts = golden["case%d_counts" % k]
    coords_all = golden["rmu"]
    A = golden["aligned"].shape[2]
    coords, kept = r0c._assemble(counts, coords_all, A, int(golden["case%d_tol" % k]))
    return r0c.DyeMap(coords, kept, counts, coords_all, None, None, None)


def test_assembly_gives_what_the_later_stages_accept(golden):
    m = _golden_map(golden, 1)          # centre 0 keeps nothing
    off = golden["case1_kept_off"]
    assert len(m) == 3
    for p in range(3):
        assert m.kept[p].dtype == np.int64
        assert np.array_equal(m.kept[p], golden["case1_kept"][off[p]:off[p + 1]])
        assert m.coords[p].dtype == np.float64 and m.coords[p].shape == (len(m.kept[p]), 9)
        assert np.array_equal(m.coords[p], golden["rmu"][p][m.kept[p]])
    o, flat = r0c._conformations(m.coords, "donor", 3)
    assert np.array_equal(o, off) and flat.shape == (off[-1], 9)
    assert np.array_equal(r0c.find_dyeless_states(m.coords), [0])


def test_centres_from_maps(golden):
    d_map, a_map = _golden_map(golden, 0), _golden_map(golden, 1)
    D = d_map.coords_all.shape[1]
    d_t, a_t = np.ones((D, D)), 2 * np.ones((D, D))
    centres = dl.centres_from_maps(d_map, d_t, a_map, a_t)
    assert len(centres) == 3
    for p, (dc, dt, dk, ac, at, ak) in enumerate(centres):
        assert dc.shape == ac.shape == (D, 9) and dt is d_t and at is a_t
        assert np.array_equal(dk, d_map.kept[p]) and np.array_equal(ak, a_map.kept[p])
        dl._coords(dc, "donor")         # what problem() asks of them
        dl._coords(ac, "acceptor")
    # the centre whose acceptor keeps nothing: make_dye_msm's mark, before any device call
    tprobs, eqs, keep = dl.make_dye_msm(a_t, centres[0][5])
    assert np.array_equal(tprobs, [0]) and np.array_equal(eqs, [0]) and len(keep) == 0
    with pytest.raises(exception.DataInvalid):
        dl.centres_from_maps(d_map, np.ones((D + 1, D + 1)), a_map, a_t)
    with pytest.raises(exception.DataInvalid):
        dl.centres_from_maps(d_map, d_t, [1, 2, 3], a_t)
    short = r0c.DyeMap(a_map.coords[:2], a_map.kept[:2], None, a_map.coords_all[:2], None, None, None)
    with pytest.raises(exception.DataInvalid):
        dl.centres_from_maps(d_map, d_t, short, a_t)


# ---- 4. the cull -------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,resseq,shift", [(1, 7, 0.0), (2, 23, 0.0), (3, 31, 900.0),
                                               (4, 44, 0.0), (5, 52, -300.0)])
def test_no_atom_outside_the_cull_radius_can_touch(seed, resseq, shift):
    """No atom outside the radius is within its cutoff of any model-aligned dye atom plus
    the frame bound of that conformation (_numpy_rmsf.frame_bound, per coordinate: sqrt(3)
    of it in distance).  In addition the dye is turned three other ways about c_ref: the
    device's R is orthogonal whatever S is, so a fit error turns an atom about c_ref."""
    c = dm.peptide_case(seed, resseq, D=24, P=3)
    xyz = (c["xyz"] + np.float32(shift)).astype(np.float32)
    cutoff = c["radii"] + 0.17
    reach = r0c.dye_reach(c["dye_xyz"], c["dye_sel"])
    rng = np.random.RandomState(seed)
    A = c["dye_xyz"].shape[1]
    n_outside = 0
    for p in range(len(xyz)):
        c_ref = xyz[p][c["prot_sel"]].astype(np.float64).mean(axis=0)
        radius = r0c.cull_radius(reach, c_ref, cutoff)
        far = np.sqrt(((xyz[p].astype(np.float64) - c_ref) ** 2).sum(axis=1)) > radius
        n_outside += int(far.sum())
        model = dm.model_align(c["dye_xyz"], xyz[p], c["prot_sel"], c["dye_sel"])
        bound = nr.frame_bound(model)
        nr.assert_bound_is_tight(model, bound)
        e = np.repeat(np.sqrt(3.0) * bound, A)[None, :]
        clouds = [model["aligned"]]
        for _ in range(3):      # any rotation about c_ref
            clouds.append((model["aligned"] - c_ref) @ dm.random_rotation(rng).T + c_ref)
        for cloud in clouds:
            pts = cloud.reshape(-1, 3)
            assert np.sqrt(((pts - c_ref) ** 2).sum(axis=1)).max() <= reach * (1 + 1e-12)
            d = dm.nd.distances(xyz[p][far], pts)
            assert np.all(d > cutoff[far][:, None] + e)
    assert n_outside > 0        # the radius does cull on this fixture


def _toward(p, target):
    """the float32 neighbour of every coordinate of p (float64) on target's side: at most one
    ulp from p, twice what the device's one rounding of an aligned coordinate can do"""
    f = p.astype(np.float32)
    wrong = np.abs(f.astype(np.float64) - target) > np.abs(p - target)
    return np.where(wrong, np.nextafter(f, target.astype(np.float32)), f).astype(np.float64)


@pytest.mark.parametrize("centre", [(0.0, 0.0, 0.0), (3.0, -2.0, 5.0), (900.0, 850.0, -700.0),
                                    (1.0e4, 3.0, -2.0e3)])
def test_the_margin_at_its_own_scale(centre):
    """An atom placed just outside the radius, and a dye atom at ``reach`` from c_ref pointing
    straight at it, moved towards the atom by a whole float32 ulp in every coordinate (the
    device's rounding is half of one): the pair must still be apart by more than the cutoff.
    The radius without its margin fails the same check somewhere off the origin, and the
    margin is no more than twice what this asks: a margin off by 1e-4 nm fails one side."""
    rng = np.random.RandomState(7)
    c_ref = np.array(centre)
    reach, cutoff = 1.7, 0.21
    radius = float(r0c.cull_radius(reach, c_ref, np.array([cutoff]))[0])
    bare = (reach + cutoff) * (1.0 + 2.0 ** -40)       # the form without a fit: no margin
    scale = 2.0 ** -24 * (np.abs(c_ref).max() + reach)
    assert radius - bare >= 2 * np.sqrt(3.0) * scale
    assert radius - bare <= 8 * scale + 2.0 ** -38 * (reach + cutoff)
    dirs = np.concatenate([rng.randn(300, 3), np.eye(3), -np.eye(3),
                           [[1, 1, 1], [-1, 1, -1], [1, -1, -1]]]).astype(np.float64)
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    worst = {"margin": np.inf, "bare": np.inf}
    for u in dirs:
        tip = c_ref + reach * u
        for name, rad in (("margin", radius), ("bare", bare)):
            atom = (c_ref + rad * u).astype(np.float32)
            while np.linalg.norm(atom.astype(np.float64) - c_ref) <= rad:     # just outside
                atom = np.nextafter(atom, (atom + np.sign(u) * np.float32(1e6)).astype(np.float32))
            a64 = atom.astype(np.float64)
            assert np.linalg.norm(a64 - c_ref) - rad <= 4 * np.sqrt(3.0) * scale + 1e-12
            q = _toward(tip, a64)
            d = dm.nd.distances(a64[None], q[None])[0, 0]
            worst[name] = min(worst[name], d - cutoff)
    assert worst["margin"] > 0.0, worst
    if np.abs(c_ref).max() >= 100.0:
        assert worst["bare"] < 0.0, worst       # the check is sharp enough to need the margin
