"""geometry.rmsf without a GPU.

mdtraj is not installed where these tests run, so the reference's ``rmsf_calc``
cannot be run and no golden output of it can be recorded: the float64 Kabsch model of
tests/_numpy_rmsf.py is the yardstick.

1. The model against itself: ``rmsf_reference`` against a brute-force loop, its
   invariance under a rigid motion of any frame, the per-residue value against the
   per-atom sums averaged, and a uniform-weight three-frame case worked by hand.
2. csrc/ek_superpose.h compiled with g++ (as tests/test_qcp_host.py builds
   ek_qcp.h), over every family of tests/_structure_cases.py, 24 frames each, frame 0
   the reference.  The fit (float64 centroid, float32 centred coordinates, S as the
   float64 sum of exact products rounded to float32) is numpy's here; lambda and the
   rotation are the header's.  Every frame that is not flagged lies within
   ``frame_bound`` (c = 8) of the Kabsch model, |det R - 1| and
   max |R^T R - I| are at most 1e-13, and the flags obey the two thresholds (flagged
   at g <= 1e-7 (Gx + Gy), not flagged at g >= 1e-4 (Gx + Gy)); every frame of a
   degenerate family is flagged (the header's rule is g <= 2e-5 (Gx + Gy)).  Measured
   here: the worst error is 0.18 of the bound (scale_tiny, A = 3), 0.006 at A = 33.
   Two premises are stated as the model has them: near_collinear reaches g / (Gx + Gy)
   = 4.6e-7 (not 1.2e-8), and the cap "bound <= 1e-3 r_max" is asked of the bound's
   rotation term, since far_offset's float32 grid alone is 1.2e-3 nm
   (_numpy_rmsf.DEGENERATE_RATIO, assert_bound_is_tight).
3. Every DataInvalid / ImproperlyConfigured path of the Python layer, with
   ``_lib.load`` replaced by a function that fails the test.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import _numpy_rmsf as nr
from _structure_cases import family_cases, structure_family

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "enspara_amd", "csrc")
FRAMES = 24
WELL = ("generic", "planar", "mirror", "rotated_copies", "identical", "cube", "scale_tiny",
        "scale_small", "scale_large", "scale_huge", "far_offset")
DEGENERATE = ("collinear_exact", "collinear_rotated", "near_collinear", "two_atom_quantised")

SHIM = r'''
#define __device__
#define __forceinline__ inline
#include <cstdint>
#include "ek_superpose.h"
extern "C" void h_superpose(const float *S, const double *Gx, const double *Gy, int n_atoms,
                            int64_t m, double *R, double *msd, int32_t *flag)
{
    for (int64_t i = 0; i < m; ++i) {
        float s[9];
        double r[9], lam;
        for (int j = 0; j < 9; ++j)
            s[j] = S[9 * i + j];
        msd[i] = ek_msd_lambda_from_S(s, Gx[i], Gy[i], n_atoms, &lam);
        flag[i] = ek_superpose_from_S(s, Gx[i], Gy[i], lam, r);
        for (int j = 0; j < 9; ++j)
            R[9 * i + j] = r[j];
    }
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("superpose_host")
    os.makedirs(d / "hip")
    (d / "hip" / "hip_runtime.h").write_text("")
    (d / "shim.cpp").write_text(SHIM)
    so = str(d / "superpose_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                           "-I", str(d), "-I", CSRC, str(d / "shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.h_superpose.restype = None
    return lib


def header_superpose(host, xyz, ref, sel):
    """the device's arithmetic with numpy's summation order -> aligned float32, R, msd,
    flags"""
    X = xyz.astype(np.float64)
    y = ref.astype(np.float64)
    cx = X[:, sel].sum(axis=1) / len(sel)
    cy = y[sel].sum(axis=0) / len(sel)
    xs = (X[:, sel] - cx[:, None]).astype(np.float32).astype(np.float64)
    ys = (y[sel] - cy).astype(np.float32).astype(np.float64)
    S = np.ascontiguousarray(np.einsum("nai,aj->nij", xs, ys).reshape(-1, 9).astype(np.float32))
    Gx = np.ascontiguousarray((xs * xs).sum(axis=(1, 2)))
    Gy = np.full(len(X), (ys * ys).sum())
    n = len(X)
    R = np.empty((n, 3, 3))
    msd = np.empty(n)
    flag = np.empty(n, dtype=np.int32)
    host.h_superpose(S.ctypes.data_as(C.c_void_p), Gx.ctypes.data_as(C.c_void_p),
                     Gy.ctypes.data_as(C.c_void_p), len(sel), C.c_int64(n),
                     R.ctypes.data_as(C.c_void_p), msd.ctypes.data_as(C.c_void_p),
                     flag.ctypes.data_as(C.c_void_p))
    aligned = (np.einsum("nij,naj->nai", R, X - cx[:, None]) + cy).astype(np.float32)
    return aligned, R, msd, flag


# ---- 1. the model against itself ---------------------------------------------------------

def _blob(rng, n, A):
    base = rng.normal(size=(A, 3))
    return (base[None] + 0.1 * rng.normal(size=(n, A, 3))).astype(np.float32)


def _rigid(rng, x):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, a, b, c = q
    R = np.array([[w * w + a * a - b * b - c * c, 2 * (a * b - w * c), 2 * (a * c + w * b)],
                  [2 * (a * b + w * c), w * w - a * a + b * b - c * c, 2 * (b * c - w * a)],
                  [2 * (a * c - w * b), 2 * (b * c + w * a), w * w - a * a - b * b + c * c]])
    return x @ R.T + rng.normal(size=3)


def test_reference_against_a_brute_force_loop():
    rng = np.random.default_rng(1)
    x = _blob(rng, 7, 11).astype(np.float64)
    w = rng.random(7)
    sel = np.array([9, 0, 4, 5, 2])
    res = np.array([0, 0, 1, 2, 2, 2, 1, 3, 3, 3, 3])
    groups = nr.groups_of(res)
    al = nr.kabsch_superpose(x, x[3], sel)["aligned"]
    per_atom = np.zeros(11)
    for a in range(11):
        for f in range(7):
            if f != 3:
                per_atom[a] += w[f] * sum((al[f, a, k] - x[3, a, k]) ** 2 for k in range(3))
    np.testing.assert_allclose(nr.rmsf_reference(x, w, 3, sel), np.sqrt(per_atom), rtol=1e-12)
    per_res = [np.mean([per_atom[a] for a in g]) for g in groups]
    np.testing.assert_allclose(nr.rmsf_reference(x, w, 3, sel, groups), np.sqrt(per_res),
                               rtol=1e-12)
    # the superposition is one: the selection's centroids coincide, R is a rotation, and
    # no other rotation does better
    m = nr.kabsch_superpose(x, x[3], sel)
    np.testing.assert_allclose(al[:, sel].mean(axis=1), np.tile(x[3, sel].mean(axis=0), (7, 1)),
                               atol=1e-12)
    np.testing.assert_allclose(np.linalg.det(m["R"]), 1.0, atol=1e-12)
    np.testing.assert_allclose(((al[:, sel] - x[3, sel]) ** 2).sum(axis=(1, 2)) / 5, m["msd"],
                               atol=1e-12)


def test_reference_is_invariant_under_rigid_motion():
    rng = np.random.default_rng(2)
    x = _blob(rng, 6, 9).astype(np.float64)
    w = rng.random(6)
    want = nr.rmsf_reference(x, w, 0)
    for f in (1, 4, 5):
        moved = x.copy()
        moved[f] = _rigid(rng, x[f])
        np.testing.assert_allclose(nr.rmsf_reference(moved, w, 0), want, rtol=1e-9)


def test_three_frames_by_hand():
    """an octahedron breathing by +e and -2e about its centre: the optimal rotation is
    the identity, every atom deviates by e and 2e, so with uniform weights the RMSF is
    sqrt((0 + e^2 + 4 e^2) / 3) = e sqrt(5 / 3) for every atom and every residue"""
    rng = np.random.default_rng(3)
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1.0]])
    e = 0.125
    x = np.stack([octa, _rigid(rng, octa * (1 + e)), _rigid(rng, octa * (1 - 2 * e))])
    want = e * np.sqrt(5.0 / 3.0)
    np.testing.assert_allclose(nr.rmsf_reference(x), np.full(6, want), rtol=1e-12)
    groups = nr.groups_of([5, 5, 2, 5, 2, 2])
    assert [g.tolist() for g in groups] == [[0, 1, 3], [2, 4, 5]]
    np.testing.assert_allclose(nr.rmsf_reference(x, groups=groups), [want, want], rtol=1e-12)
    # the summation contract on the same case, float32 in
    al = nr.kabsch_superpose(x, x[0])["aligned"].astype(np.float32)
    sums, gs = nr.accumulate(al, x[0].astype(np.float32), np.full(3, 1 / 3), groups, tile=2)
    np.testing.assert_allclose(np.sqrt(sums), want, rtol=1e-6)
    np.testing.assert_allclose(np.sqrt(gs), want, rtol=1e-6)


# ---- 2. the header ------------------------------------------------------------------------

def _check_family(host, family, A, sel):
    x = structure_family(family, FRAMES, A)
    m = nr.kabsch_superpose(x, x[0], sel)
    ratio = m["g"] / m["G"]
    aligned, R, msd, flag = header_superpose(host, x, x[0], sel)
    well = family in WELL and len(sel) >= 3
    if well:
        assert np.all(ratio >= 2e-3), (family, A, ratio.min())
    else:
        assert family in DEGENERATE or len(sel) == 2
        # (frame 0 against itself has S = x^T x, as degenerate as the structure)
        assert np.all(ratio <= nr.DEGENERATE_RATIO), (family, A, ratio.max())
    # the two thresholds
    assert np.all(flag[ratio <= 1e-7] == 1)
    assert np.all(flag[ratio >= 1e-4] == 0)
    if not well:
        # the header's own rule, g <= 2e-5 (Gx + Gy), is forty times above these
        assert np.all(flag == 1), (family, A, flag)
        return
    bound = nr.frame_bound(m)
    nr.assert_bound_is_tight(m, bound)
    err = np.abs(aligned.astype(np.float64) - m["aligned"]).max(axis=(1, 2))
    print("%s A=%d n_sel=%d: worst error / bound %.3g" % (family, A, len(sel),
                                                          (err / bound).max()))
    assert np.all(err <= bound), (family, A, int((err / bound).argmax()), (err / bound).max())
    det = np.linalg.det(R)
    orth = np.abs(np.einsum("nji,njk->nik", R, R) - np.eye(3)).max(axis=(1, 2))
    assert np.all(np.abs(det - 1.0) <= 1e-13) and np.all(orth <= 1e-13), (det, orth.max())
    scale = m["G"] / len(sel)
    assert np.all(np.abs(msd - m["msd"]) <= 1e-4 * scale)


@pytest.mark.parametrize("family,A", family_cases())
def test_header_against_kabsch_all_atoms(host, family, A):
    _check_family(host, family, A, np.arange(A))


@pytest.mark.parametrize("family,A", [(f, a) for f, a in family_cases() if a >= 7])
def test_header_against_kabsch_subset(host, family, A):
    sel = np.array([31, 2, 17, 8, 5]) if A == 33 else np.array([6, 1, 4, 3][:A - 3])
    _check_family(host, family, A, sel)


# ---- 3. the Python layer's refusals, without a device ---------------------------------------

@pytest.fixture
def no_device(monkeypatch):
    from enspara_amd import _lib

    def fail():
        raise AssertionError("the device library was loaded before validation ended")
    monkeypatch.setattr(_lib, "load", fail)


def test_every_refusal_comes_before_the_device(no_device):
    from enspara_amd import exception
    from enspara_amd.geometry import rmsf
    rng = np.random.default_rng(4)
    x = _blob(rng, 5, 6)
    ref = x[0].copy()
    res = np.array([0, 0, 1, 1, 2, 2])
    bad = exception.DataInvalid
    nan = x.copy()
    nan[2, 1, 0] = np.nan
    inf = x.copy()
    inf[4, 5, 2] = np.inf
    for args, kw in [
            ((x.astype(np.float64), ref), {}),                  # dtype
            ((x[0], ref), {}),                                  # shape
            ((x[:, :, :2], ref), {}),
            ((x[:, :2], ref[:2]), {}),                          # fewer than 3 atoms
            ((x[:0], ref), {}),                                 # no frames
            ((nan, ref), {}), ((inf, ref), {}),                 # not finite
            ((x, ref[:5]), {}), ((x, ref.astype(np.float64)), {}),
            ((x, nan[2]), {}),
            ((x, ref), {"atom_indices": [0, 1]}),               # fewer than 3
            ((x, ref), {"atom_indices": [0, 1, 1]}),            # not unique
            ((x, ref), {"atom_indices": [0, 1, 6]}),            # out of range
            ((x, ref), {"atom_indices": [-1, 1, 2]}),
            ((x, ref), {"atom_indices": [0.0, 1.0, 2.0]}),      # not integers
            ((x, ref), {"atom_indices": [[0, 1, 2]]}),
            ((x, ref), {"chunk_frames": 0}), ((x, ref), {"chunk_frames": 2.5})]:
        with pytest.raises(bad):
            rmsf.superpose(*args, **kw)
    for kw in [{"ref_frame": 5}, {"ref_frame": -1}, {"ref_frame": 1.0},
               {"populations": np.ones(4)}, {"populations": [1, 1, 1, 1, np.nan]},
               {"populations": [1, 1, 1, 1, np.inf]}, {"populations": [1, 1, -0.5, 1, 1]},
               {"populations": ["a"] * 5},
               {"residue_index": res[:5]}, {"residue_index": res.astype(np.float64)},
               {"atom_indices": [0, 1, 1]}, {"atom_indices": [0, 1, 9]}, {"chunk_frames": -3}]:
        kw.setdefault("residue_index", res)
        with pytest.raises(bad):
            rmsf.rmsf_calc(x, **kw)
    for c in (nan, inf, x.astype(np.float64), x[0], x[:, :2]):
        with pytest.raises(bad):
            rmsf.rmsf_calc(c, per_residue=False)
    with pytest.raises(exception.ImproperlyConfigured):
        rmsf.rmsf_calc(x)
    with pytest.raises(exception.ImproperlyConfigured):
        rmsf.rmsf_calc(x, per_residue=True, residue_index=None)


def test_residues_and_bfactors(no_device):
    from enspara_amd import exception
    from enspara_amd.geometry import rmsf
    res = np.array([7, 3, 7, 7, 3, 9, 3, 7, 7])
    off, atoms = rmsf._residues(res, 9)
    assert off.tolist() == [0, 5, 8, 9]
    assert atoms.tolist() == [0, 2, 3, 7, 8, 1, 4, 6, 5]
    assert [g.tolist() for g in nr.groups_of(res)] == [[0, 2, 3, 7, 8], [1, 4, 6], [5]]
    b = rmsf.bfactors_from_rmsfs(res, [0.5, 0.25, 2.0])
    assert b.dtype == np.float64
    assert b.tolist() == [0.5, 0.25, 0.5, 0.5, 0.25, 2.0, 0.25, 0.5, 0.5]
    with pytest.raises(exception.DataInvalid):
        rmsf.bfactors_from_rmsfs(res, [0.5, 0.25])
    assert rmsf.last_timing().shape == (3,)
    assert (rmsf.TILE, rmsf.LDS_ATOMS, rmsf.WAVE_ATOMS) == (nr.TILE, 3072, 512)


def test_library_side_is_declared():
    from enspara_amd import _lib, build
    assert "ek_rmsf.hip" in build.SOURCES
    assert {"ek_rmsf_open", "ek_rmsf_run", "ek_rmsf_fetch", "ek_rmsf_last_timing",
            "ek_rmsf_close"} <= set(_lib.SYMBOLS)
    L = _lib.load()
    h = C.c_void_p()
    sel = np.arange(3, dtype=np.int32)
    ref = np.zeros((3, 3), dtype=np.float32)
    # argument errors come before the device
    assert L.ek_rmsf_open(0, 3, 2, _lib.i32p(sel), _lib.f32p(ref), 0, None, None,
                          C.byref(h)) == _lib.EK_EARG
    sel[2] = 3
    assert L.ek_rmsf_open(0, 3, 3, _lib.i32p(sel), _lib.f32p(ref), 0, None, None,
                          C.byref(h)) == _lib.EK_EARG
    assert L.ek_rmsf_run(None, None, 0, None, -1, 0, None, None, None, None) == _lib.EK_EARG
    assert L.ek_rmsf_fetch(None, None, None) == _lib.EK_EARG
    assert L.ek_rmsf_close(None) == _lib.EK_OK
