"""geometry.rmsf on the device (csrc/ek_rmsf.hip) against tests/_numpy_rmsf.py.

mdtraj is not installed where these tests run, so the reference's ``rmsf_calc``
cannot be run and no golden output of it exists: the float64 Kabsch model is the
yardstick for the superposition, and ``accumulate`` (the summation contract restated
operation for operation) for the sums, bit for bit.

The bound on |aligned_device - aligned_model| is ``frame_bound`` (c = 8),
computed per frame from the model alone.  Before anything is compared the model's
values are asserted to separate: g / (Gx + Gy) >= 2e-3 on every frame of a
well-conditioned family, <= 5e-7 on every frame of a degenerate one, and the
rotation's share of the bound is at most 1e-3 r_max.  No frame of a well-conditioned
family is left out.
"""
import functools

import numpy as np
import pytest

import _numpy_rmsf as nr
from _structure_cases import family_cases, structure_family
from test_rmsf_host import DEGENERATE, FRAMES, WELL
from test_structure_families_host import TOL

pytestmark = pytest.mark.gpu

TILE = nr.TILE
SUBSET_33 = np.array([31, 2, 17, 8, 5])


def _subset(A):
    return SUBSET_33 if A == 33 else np.array([6, 1, 4, 3][:A - 3])


@functools.lru_cache(maxsize=None)
def _model(family, A, subset):
    x = structure_family(family, FRAMES, A)
    sel = _subset(A) if subset else None
    m = nr.kabsch_superpose(x, x[0], sel)
    for v in m.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x, sel, m


def _compare(x, sel, m, aligned, rot, rmsd, cap=True):
    bound = nr.frame_bound(m)
    if cap:
        nr.assert_bound_is_tight(m, bound)
    err = np.abs(aligned.astype(np.float64) - m["aligned"]).max(axis=(1, 2))
    print("worst error / bound %.3g" % (err / bound).max())
    assert np.all(err <= bound), (int((err / bound).argmax()), (err / bound).max())
    det = np.linalg.det(rot)
    orth = np.abs(np.einsum("nji,njk->nik", rot, rot) - np.eye(3)).max(axis=(1, 2))
    assert np.all(np.abs(det - 1.0) <= 1e-13) and np.all(orth <= 1e-13), (det, orth.max())
    d = rmsd.astype(np.float64)
    scale = m["G"] / m["n_sel"]
    assert np.all(np.abs(d * d - m["msd"]) <= TOL * scale), \
        float((np.abs(d * d - m["msd"]) / scale).max())


@pytest.mark.parametrize("family,A,subset", [
    (f, a, s) for f, a in family_cases() if f in WELL and a >= 3
    for s in ((False, True) if a >= 7 else (False,))])
def test_superposition_against_kabsch(family, A, subset):
    from enspara_amd.geometry import rmsf
    x, sel, m = _model(family, A, subset)
    assert np.all(m["g"] / m["G"] >= 2e-3), float((m["g"] / m["G"]).min())
    aligned, rot, rmsd = rmsf.superpose(x, x[0], atom_indices=sel, return_transforms=True)
    assert aligned.dtype == np.float32 and aligned.shape == x.shape
    assert rot.dtype == np.float64 and rot.shape == (FRAMES, 3, 3)
    assert rmsd.dtype == np.float32 and rmsd.shape == (FRAMES,)
    _compare(x, sel, m, aligned, rot, rmsd)
    # the selection's centroid lies on the reference's
    s = np.arange(A) if sel is None else sel
    c = aligned[:, s].astype(np.float64).mean(axis=1)
    want = x[0, s].astype(np.float64).mean(axis=0)
    assert np.all(np.abs(c - want) <= 2.0 ** -22 * np.abs(m["aligned"]).max() + 1e-30)
    # chunked: the same bits
    again = rmsf.superpose(x, x[0], atom_indices=sel, chunk_frames=7)
    assert np.array_equal(again.view(np.uint32), aligned.view(np.uint32))


@pytest.mark.parametrize("family,A", [(f, a) for f, a in family_cases()
                                      if f in DEGENERATE and a >= 3])
def test_degenerate_families_are_refused(family, A):
    from enspara_amd import _lib, exception
    from enspara_amd.geometry import rmsf
    x, _, m = _model(family, A, False)
    assert np.all(m["g"] / m["G"] <= nr.DEGENERATE_RATIO)
    before = _lib.live_resources()
    # frame 0 is the reference frame and is not fitted: frame 1 is the first refused
    with pytest.raises(exception.DataInvalid, match=r"frame 1 .* 23 such"):
        rmsf.rmsf_calc(x, per_residue=False)
    with pytest.raises(exception.DataInvalid, match=r"frame 1 .* 23 such"):
        rmsf.rmsf_calc(x, per_residue=False, chunk_frames=5)
    # superpose has no reference FRAME: a copy of the reference is fitted like any other
    # structure, and a collinear structure against itself is as undetermined as any
    with pytest.raises(exception.DataInvalid, match=r"frame 0 .* 24 such"):
        rmsf.superpose(x, x[0])
    assert _lib.live_resources()[:6] == before[:6]


def _interleaved_residues(A):
    """residues of 1, 2 and 5 atoms, interleaved and not contiguous, values not sorted"""
    sizes, res, k = [5, 1, 2], [], 0
    while len(res) < A:
        res += [100 - k] * sizes[k % 3]
        k += 1
    res = np.array(res[:A])
    return res[np.random.default_rng(A).permutation(A)]


@functools.lru_cache(maxsize=None)
def _frames(n, A):
    rng = np.random.default_rng(1000 * A + n)
    base = rng.normal(scale=1.0 + 0.05 * A ** (1 / 3), size=(A, 3))
    x = (base[None] + 0.1 * rng.normal(size=(n, A, 3))).astype(np.float32)
    x.setflags(write=False)
    return x


def _weights(n, kind):
    if kind is None:
        return None
    w = np.random.default_rng(n).random(n)
    w[::3] = 0.0            # exact zeros
    return w


def _device_sums(x, w, ref_frame, sel, res, chunk):
    from enspara_amd.geometry import rmsf
    groups = rmsf._residues(res, x.shape[1])
    return rmsf._rmsf_sums(x, w, ref_frame, sel, groups, chunk, 0, want_aligned=True)


@pytest.mark.parametrize("n", sorted({1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1}))
@pytest.mark.parametrize("A", [3, 4, 7, 33])
def test_accumulation_bit_for_bit(n, A):
    x = _frames(n, A)
    res = _interleaved_residues(A)
    groups = nr.groups_of(res)
    sel = None if A < 7 else _subset(A)
    for ref_frame in sorted({0, n // 2, n - 1}):
        for kind in ("random", None):
            w = _weights(n, kind)
            first = None
            for chunk in (1, 7, TILE, None):
                sums, gsums, aligned = _device_sums(x, w, ref_frame, sel, res, chunk)
                assert np.array_equal(aligned[ref_frame].view(np.uint32),
                                      x[ref_frame].view(np.uint32))
                if first is None:
                    first = (sums, gsums, aligned)
                    ww = np.full(n, 1.0 / n) if w is None else w
                    want, gwant = nr.accumulate(aligned, x[ref_frame], ww, groups)
                    assert np.array_equal(sums, want), np.abs(sums - want).max()
                    assert np.array_equal(gsums, gwant)
                else:
                    assert np.array_equal(sums, first[0]) and np.array_equal(gsums, first[1])
                    assert np.array_equal(aligned.view(np.uint32), first[2].view(np.uint32))


@pytest.mark.parametrize("A", [513, 3073])
def test_accumulation_where_the_kernel_changes_form(A):
    """one wave per tile up to 512 atoms, four beyond; the frame and the accumulators in
    LDS up to 3072 atoms, in global memory beyond.  At 3073 atoms with all of them selected
    the bound's rotation term (n_sel + 2 = 3075 roundings) exceeds 1e-3 r_max, so that cap
    is not asserted there; the bound itself is, and the five-atom selection's with it."""
    from enspara_amd.geometry import rmsf
    n = 2 * TILE + 1
    x = _frames(n, A)
    res = _interleaved_residues(A)
    groups = nr.groups_of(res)
    w = _weights(n, "random")
    for sel in (None, SUBSET_33):
        first = None
        for chunk in (7, None):
            sums, gsums, aligned = _device_sums(x, w, n // 2, sel, res, chunk)
            if first is None:
                first = (sums, gsums)
                want, gwant = nr.accumulate(aligned, x[n // 2], w, groups)
                assert np.array_equal(sums, want) and np.array_equal(gsums, gwant)
            else:
                assert np.array_equal(sums, first[0]) and np.array_equal(gsums, first[1])
        m = nr.kabsch_superpose(x[:FRAMES], x[n // 2], sel)
        assert np.all(m["g"] / m["G"] >= 2e-3)
        al, rot, rmsd = rmsf.superpose(x[:FRAMES], x[n // 2], atom_indices=sel,
                                       return_transforms=True)
        _compare(x[:FRAMES], sel, m, al, rot, rmsd, cap=(sel is not None or A <= 1024))


@pytest.mark.parametrize("A,per_residue", [(7, True), (33, True), (33, False), (513, True)])
def test_rmsf_end_to_end(A, per_residue):
    """|rmsf - reference| <= sqrt(3) max_f bound_f + 8 2^-53 (frames + atoms in residue)
    rmsf: a weighted RMS of distances moves by at most the largest per-frame
    displacement"""
    from enspara_amd.geometry import rmsf
    n = TILE + 5
    x = _frames(n, A)
    res = _interleaved_residues(A)
    groups = nr.groups_of(res)
    w = np.random.default_rng(A).random(n)
    w /= w.sum()
    sel = None if A < 33 else SUBSET_33
    ref_frame = 3
    m = nr.kabsch_superpose(x, x[ref_frame], sel)
    assert np.all(m["g"] / m["G"] >= 2e-3)
    bound = nr.frame_bound(m)
    nr.assert_bound_is_tight(m, bound)
    want = nr.rmsf_reference(x, w, ref_frame, sel, groups if per_residue else None)
    got = rmsf.rmsf_calc(x, w, ref_frame, per_residue, sel, res if per_residue else None)
    assert got.dtype == np.float64 and got.shape == want.shape
    largest = max(len(g) for g in groups) if per_residue else 1
    tol = np.sqrt(3.0) * bound.max() + 8 * 2.0 ** -53 * (n + largest) * want
    print("worst |rmsf - reference| / tolerance %.3g" % (np.abs(got - want) / tol).max())
    assert np.all(np.abs(got - want) <= tol)
    # the reference frame: its own bits, deviation exactly 0
    sums, _, aligned = rmsf._rmsf_sums(x, np.eye(n)[ref_frame], ref_frame, sel, None, None, 0,
                                       want_aligned=True)
    assert np.array_equal(aligned[ref_frame].view(np.uint32), x[ref_frame].view(np.uint32))
    assert np.all(sums == 0.0)
    assert rmsf.last_timing().shape == (3,) and rmsf.last_timing()[1] > 0


def test_resources_balance():
    from enspara_amd import _lib, exception
    from enspara_amd.geometry import rmsf
    x = _frames(TILE + 1, 33)
    res = _interleaved_residues(33)
    rmsf.rmsf_calc(x, residue_index=res)            # (first use loads the code object)
    before = _lib.live_resources()
    rmsf.rmsf_calc(x, residue_index=res, chunk_frames=7)
    rmsf.superpose(x, x[0], return_transforms=True)
    assert _lib.live_resources()[:6] == before[:6]
    bad = structure_family("collinear_rotated", FRAMES, 7)
    with pytest.raises(exception.DataInvalid, match=r"frame 1 "):
        rmsf.rmsf_calc(bad, residue_index=res[:7])
    assert _lib.live_resources()[:6] == before[:6]
    with pytest.raises(exception.DataInvalid):      # collinear three-atom selection
        rmsf.superpose(np.ascontiguousarray(bad[:, :3]), bad[0, :3])
    assert _lib.live_resources()[:6] == before[:6]
