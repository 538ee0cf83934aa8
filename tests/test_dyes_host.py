"""Dye labelling without a device: the numpy model (tests/_numpy_dyes.py) and the host
helpers of geometry.dyes_from_expt_dist against recorded outputs of the reference
(tests/golden/dyes_golden.npz, made by tests/golden/make_dyes_golden.py), ``load_dye``,
``find_atom_index`` and every ``DataInvalid`` path (none of them loads the library)."""
import os

import numpy as np
import pytest

import _numpy_dyes as nd
from enspara_amd import _lib, ra
from enspara_amd.exception import DataInvalid
from enspara_amd.geometry import dyes_from_expt_dist as dyes

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(HERE, "golden", "dyes_golden.npz"))


def _backbone(G, res):
    return dyes.backbone_indices(G["pep_names"], G["pep_seqs"], int(res))


def _rot_bounds(xyz, bb):
    """DESIGN.md 4l, "how far M may be from the reference's": the float32 error bounds of
    z, x, y from the two angles that condition them, in units of 1"""
    x = xyz.astype(np.float64)
    n, ca, c = x[bb[0]], x[bb[1]], x[bb[2]]
    unit = lambda v: v / np.linalg.norm(v)      # noqa: E731
    C = np.abs(x).max()
    sin1 = np.linalg.norm(np.cross(unit(ca - n), unit(ca - c)))
    normed = unit(np.cross(unit(ca - n), unit(ca - c)))
    cb = ca + np.sin(np.pi / 6) * 0.153 * unit(ca - (n + c) / 2) + np.cos(np.pi / 6) * 0.153 * normed
    z = unit(cb - ca)
    sin2 = np.linalg.norm(np.cross(unit(n - ca), z))
    e_cb = U * (2 * (C + 0.16) + 0.0765 * 8 + 0.1325 * (35 / sin1 + 8))
    e_z = (e_cb + U * 0.153) / 0.153 + 8 * U
    e_x = (2 * (8 * U + e_z + U) + U) / sin2 + 8 * U
    e_y = 2 * (e_z + e_x + U) + U + 8 * U
    return e_cb, max(e_z, e_x, e_y)


def test_geometry_helpers_within_the_derived_bounds(G):
    xyz, dye = G["pep_xyz"], G["geo_dye"]
    bbs = np.array([_backbone(G, r) for r in G["geo_res"]])
    cb = dyes.calc_cb_coords(xyz, bbs)
    assert cb.dtype == np.float32 and cb.shape == (len(bbs), 3)
    # over frames: the same bits, frame by frame
    stack = np.stack([xyz, xyz + np.float32(0.25)])
    assert np.array_equal(dyes.calc_cb_coords(stack, bbs)[0], cb)
    for i, bb in enumerate(bbs):
        e_cb, e_M = _rot_bounds(xyz, bb)
        assert np.abs(cb[i] - G["geo_cb"][i]).max() <= e_cb
        M, t = dyes.determine_rot_mat(xyz, bb)
        Ms, ts = dyes.determine_rot_mat(stack, bb)
        assert M.dtype == t.dtype == np.float32 and np.array_equal(Ms[0], M)
        assert np.array_equal(ts[0], t) and np.array_equal(t, G["geo_t"][i].astype(np.float32))
        print("residue %d: |dM| %.3g of %.3g" % (G["geo_res"][i], np.abs(M - G["geo_M"][i]).max(),
                                                 e_M))
        assert np.abs(M - G["geo_M"][i]).max() <= e_M
        # the model's M is the module's, and both align alike, bit for bit
        mM, mt = nd.rot_mat(xyz, bb)
        assert np.array_equal(mM, M) and np.array_equal(mt, t)
        al = dyes.align_dye_to_res(xyz, dye, bb)
        assert al.dtype == np.float32 and np.array_equal(al, nd.align(dye, M, t))
        l1 = np.abs(dye).sum(axis=1).max()
        bound = l1 * e_M + 6 * U * (l1 + np.abs(t).max())
        assert np.abs(al - G["geo_aligned"][i]).max() <= bound


def test_model_keeps_what_the_reference_keeps(G):
    mask = nd.keep_mask(G["rt_coords"], G["pep_xyz"], G["pep_radii"] + float(G["rt_probe"]))
    assert np.array_equal(np.flatnonzero(mask), G["rt_kept"])
    assert np.array_equal(G["rt_kept"], G["rt_kept_public"])


def test_histogram_helpers(G):
    counts, edges = dyes.bincount_dists(G["bc_dists"], float(G["bc_width"]))
    assert np.array_equal(counts, G["bc_counts"]) and np.array_equal(edges, G["bc_edges"])
    assert np.array_equal(nd.chunk_hist(G["bc_dists"], float(G["bc_width"])), G["bc_counts"])
    probs, edges = nd.pair_distribution(G["pd_a"], G["pd_b"], float(G["pd_width"]))
    assert np.array_equal(probs, G["pd_probs"]) and np.array_equal(edges, G["pd_edges"])
    counts, _ = nd.pair_counts(G["pd_a"], G["pd_b"], float(G["pd_width"]))
    assert np.array_equal(dyes.int_norm_hist(G["pd_edges"], counts), G["pd_probs"])
    # the chunked case: its recorded counts give its recorded distribution
    assert np.array_equal(dyes.int_norm_hist(G["pc_edges"], G["pc_counts"]), G["pc_probs"])
    assert len(G["pc_counts"]) == G["pc_chunk_nbins"].max() > G["pc_chunk_nbins"].min()
    # points on the curve instead of bins: trapezoids
    xs, ys = np.array([0., 1., 3.]), np.array([2., 4., 0.])
    assert np.array_equal(dyes.int_norm_hist(xs, ys), ys / 7.0)
    tot, e = dyes._merge_histograms([np.array([1, 2]), np.array([1, 1, 5])],
                                    [np.arange(3.), np.arange(4.)], weights=[0.5, 0.5])
    assert np.array_equal(tot, [1.0, 1.5, 2.5]) and np.array_equal(e, np.arange(4.))
    tot, e = dyes._merge_histograms([np.array([1, 2, 3]), np.array([4, 5, 6])],
                                    [np.arange(4.), np.arange(4.) * 2])
    assert np.array_equal(tot, [5, 7, 9]) and np.array_equal(e, np.arange(4.))


def test_model_end_to_end(G):
    bbs = [_backbone(G, r) for r in G["e2e_res"]]
    probs, edges, kept, counts = nd.frame_distribution(
        G["pep_xyz"], G["pep_radii"] + 0.2, G["e2e_dye1"], G["e2e_dye2"], bbs, 0.1)
    assert np.array_equal(probs, G["e2e_probs"]) and np.array_equal(edges, G["e2e_edges"])
    for p in range(4):
        assert np.array_equal(kept[p], G["e2e_kept%d" % p])
    assert np.array_equal(counts[0], G["e2e_counts0"])
    assert np.array_equal(counts[1], G["e2e_counts1"])
    # what make_distribution takes
    dd = dyes.make_distribution(ra.RaggedArray([probs]), ra.RaggedArray([edges]))
    assert abs(dd[0][:, 1].sum() - 1) < 1e-12 and dd[0].shape == (len(probs), 2)


def test_find_atom_index_and_backbones():
    names = np.array(["N", "CA", "C", "O", "N", "CA", "CB", "C", "N", "CA", "C"])
    seqs = np.array([5, 5, 5, 5, 9, 9, 9, 9, 9, 9, 9])       # (9 twice: two chains)
    assert dyes.find_atom_index(names, seqs, 5, "CA") == 1
    assert dyes.find_atom_index(names, seqs, 9, "C") == 7
    assert dyes.find_atom_index(names, seqs, 9, "N") == 4
    assert dyes.find_atom_index(names, seqs, 5, "CB") is None
    assert dyes.find_atom_index(names, seqs, 7, "CA") is None
    assert np.array_equal(dyes.backbone_indices(names, seqs, 9), [4, 5, 7])
    with pytest.raises(DataInvalid):
        dyes.backbone_indices(names[:2], seqs[:2], 5)
    with pytest.raises(DataInvalid):
        dyes.find_atom_index(names, seqs[:3], 5, "CA")


def test_load_dye(tmp_path):
    cloud = np.array([[0.1, -0.2, 0.3], [1.5, 2.5, -3.5]])
    np.save(tmp_path / "c.npy", cloud)
    got = dyes.load_dye(str(tmp_path / "c.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, cloud.astype(np.float32))
    pdb = ("REMARK a cloud\n"
           "ATOM      1  C1  DYE A   1      12.340  -5.600   0.125  1.00  0.00           C\n"
           "HETATM    2  C2  DYE A   1    -100.000 200.500  -0.001  1.00  0.00           C\n"
           "TER\n"
           "END\n")
    (tmp_path / "c.pdb").write_text(pdb)
    got = dyes.load_dye(str(tmp_path / "c.pdb"))
    want = np.array([[12.340, -5.600, 0.125], [-100.0, 200.5, -0.001]],
                    dtype=np.float32) / np.float32(10)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    (tmp_path / "e.pdb").write_text("REMARK nothing\nEND\n")
    for bad in ("e.pdb", "missing.pdb"):
        with pytest.raises(DataInvalid):
            dyes.load_dye(str(tmp_path / bad))
    np.save(tmp_path / "bad.npy", np.zeros((3, 2)))
    with pytest.raises(DataInvalid):
        dyes.load_dye(str(tmp_path / "bad.npy"))


@pytest.fixture()
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library was loaded before the input was checked")
    monkeypatch.setattr(_lib, "load", boom)


def _inputs(G):
    xyz = np.stack([G["pep_xyz"]] * 2)
    bbs = np.array([_backbone(G, r) for r in G["e2e_res"]])
    return dict(xyz=xyz, radii=G["pep_radii"], dye1=G["e2e_dye1"], dye2=G["e2e_dye2"],
                backbones=bbs)


def _with(d, **kw):
    d = dict(d)
    d.update(kw)
    return d


def test_invalid_trajectory_input(G, no_library):
    ok = _inputs(G)
    nan_xyz = ok["xyz"].copy()
    nan_xyz[1, 7, 2] = np.nan
    far_dye = ok["dye1"].copy()
    far_dye[0, 0] = np.inf
    flat = ok["xyz"].copy()
    flat[1, ok["backbones"][0]] = flat[1, ok["backbones"][0][0]]     # N = CA = C
    cases = [
        _with(ok, xyz=ok["xyz"][0]),                        # one frame is not a trajectory
        _with(ok, xyz=ok["xyz"].astype(np.float64)),
        _with(ok, xyz=ok["xyz"][:0]),
        _with(ok, xyz=nan_xyz),
        _with(ok, xyz=ok["xyz"] * np.float32(1e7)),         # beyond MAX_COORD
        _with(ok, xyz=flat),                                # no plane: M is not finite
        _with(ok, radii=ok["radii"][:-1]),
        _with(ok, radii=np.full(len(ok["radii"]), np.nan)),
        _with(ok, radii=ok["radii"] - 1.0),                 # cutoff <= 0
        _with(ok, dye1=ok["dye1"][:, :2]),
        _with(ok, dye1=ok["dye1"].astype(np.float64)),
        _with(ok, dye2=far_dye),
        _with(ok, dye2=ok["dye2"][:0]),
        _with(ok, backbones=ok["backbones"][:1]),
        _with(ok, backbones=ok["backbones"].astype(np.float64)),
        _with(ok, backbones=ok["backbones"] + len(ok["radii"])),
        _with(ok, backbones=-ok["backbones"] - 1),
        _with(ok, bin_width=0.0),
        _with(ok, bin_width=-0.1),
        _with(ok, bin_width=np.nan),
        _with(ok, bin_width="wide"),
        _with(ok, bin_width=1e-3),                          # the placements span > 4093 bins
        _with(ok, chunk_frames=0),
        _with(ok, chunk_frames=dyes.MAX_CHUNK_FRAMES + 1),
        _with(ok, chunk_frames=1.5),
        _with(ok, probe_radius="x"),
    ]
    for i, kw in enumerate(cases):
        with pytest.raises(DataInvalid):
            dyes.dye_distance_distribution(**kw)
            pytest.fail("case %d did not raise" % i)
    with pytest.raises(NotImplementedError):
        dyes.dye_distance_distribution(cluster_grid_points=True, **ok)


def test_invalid_stage_input(G, no_library):
    xyz, radii, c = G["pep_xyz"], G["pep_radii"], G["rt_coords"]
    bad_c = c.copy()
    bad_c[3, 1] = np.nan
    for kw in (dict(coords=c.astype(np.float64)), dict(coords=c[:, :2]), dict(coords=c[:0]),
               dict(coords=bad_c), dict(frame_xyz=np.stack([xyz, xyz])),
               dict(frame_xyz=xyz.astype(np.float64)), dict(radii=radii[:5]),
               dict(probe_radius=-1.0)):
        args = dict(coords=c, frame_xyz=xyz, radii=radii)
        args.update(kw)
        with pytest.raises(DataInvalid):
            dyes.remove_touches_protein(**args)
    a, b = G["pd_a"], G["pd_b"]
    for args in ((a.astype(np.float64), b), (a, b[:, :2]), (a, bad_c), (a[:0], b)):
        with pytest.raises(DataInvalid):
            dyes.pairwise_distance_distribution(*args)
    for w in (0.0, -1.0, np.inf, np.nan, 1e-4, 2.0 ** 41):     # (1e-4: > 4093 bins)
        with pytest.raises(DataInvalid):
            dyes.pairwise_distance_distribution(a, b, bin_width=w)
    with pytest.raises(DataInvalid):
        dyes.align_dye_to_res(np.stack([xyz, xyz]), a, [0, 1, 2])
    with pytest.raises(DataInvalid):
        dyes.calc_cb_coords(xyz, [[0, 1, len(xyz)]])
    with pytest.raises(DataInvalid):
        dyes.determine_rot_mat(xyz, [[0, 1, 2], [5, 6, 7]])


def test_the_library_declares_the_entry_points():
    names = {"ek_dyes_open", "ek_dyes_run", "ek_dyes_counts", "ek_dyes_fetch",
             "ek_dyes_last_timing", "ek_dyes_close", "ek_dyes_touches", "ek_dyes_pair_hist"}
    assert names <= set(_lib.SYMBOLS)
    assert dyes.last_labelling_timing().shape == (4,)
