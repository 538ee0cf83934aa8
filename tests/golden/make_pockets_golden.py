#!/usr/bin/env python3
"""Generate tests/golden/pockets_golden.npz.

    python tests/golden/make_pockets_golden.py

Needs the reference (make_golden.REF) and scipy; runs on the CPU; only data is stored.
The reference's enspara/geometry/pockets.py is loaded with placeholder modules for what
it imports and does not need here (mdtraj, joblib, its own util package), and is fed a
stand-in for a one-frame trajectory: ``.xyz`` [1, atoms, 3] float32, ``.top.n_atoms``,
``.top.atoms[i].element.radius``.  Everything recorded comes out of its functions, called
in the order its get_pocket_cells calls them (whose own result is checked against them).

  cases [24]               names: bp<frame>_<setting> and shell<k>_<setting>, settings
                           a = (spacing 0.1, probe 0.14), b = (0.1, 0.07), c = (0.07, 0.14;
                           beta-peptide only)
  spacing, probe [24]      the setting of each case
  shell<k>_xyz, shell<k>_elements     k = 0 .. 2: the hollow-shell fixtures (below)
  <case>_dims [3]          the grid
  <case>_ax<0..2>          the coordinates of the cells along each axis, float64
  <case>_touches           np.packbits of the bool grid, flat
  <case>_ranks             uint8 grid
  <case>_fc3, <case>_fc5   scipy's fclusterdata labels (t = 1.5 spacings, 'distance') of
                           the cells of rank >= 3 and >= 5, in the order of the grid

The beta-peptide frames 0 .. 5 are bp_xyz[:6] of exposons_golden.npz, radii by bp_elements.
A shell fixture: seeded atoms at a radius drawn uniformly from a range, directions uniform on
the sphere without the two caps |z| > 0.8, then the axes scaled by (1, 1.3, 0.8); elements
drawn from H, C, N, O.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy.cluster.hierarchy

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import REF  # noqa: E402
import _numpy_pockets as npk  # noqa: E402

SETTINGS = {"a": (0.1, 0.14), "b": (0.1, 0.07), "c": (0.07, 0.14)}
SHELLS = [(0.55, 0.75, 120, 11), (0.7, 0.9, 200, 12), (0.4, 0.5, 60, 13)]   # r0, r1, atoms, seed


def shell(r0, r1, atoms, seed):
    rng = np.random.RandomState(seed)
    pts = []
    while len(pts) < atoms:
        v = rng.normal(size=3)
        v /= np.linalg.norm(v)
        if abs(v[2]) <= 0.8:
            pts.append(v * rng.uniform(r0, r1))
    xyz = (np.array(pts) * np.array([1.0, 1.3, 0.8])).astype(np.float32)
    return xyz, np.array(rng.choice(["H", "C", "N", "O"], size=atoms))


def load_reference():
    for name in ("mdtraj", "enspara", "enspara.geometry", "enspara.util",
                 "enspara.util.parallel"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["enspara"].__path__ = []
    sys.modules["enspara.geometry"].__path__ = []
    sys.modules["enspara.util"].__path__ = []
    sys.modules["enspara.util"].parallel = sys.modules["enspara.util.parallel"]
    if "joblib" not in sys.modules:
        try:
            import joblib  # noqa: F401
        except ImportError:
            jl = types.ModuleType("joblib")
            jl.Parallel = jl.delayed = None
            sys.modules["joblib"] = jl
    spec = importlib.util.spec_from_file_location(
        "enspara.geometry.pockets", os.path.join(REF, "enspara", "geometry", "pockets.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["enspara.geometry.pockets"] = mod
    spec.loader.exec_module(mod)
    return mod


class _Element:
    def __init__(self, radius):
        self.radius = radius


class _Atom:
    def __init__(self, radius):
        self.element = _Element(radius)


class _Top:
    def __init__(self, radii):
        self.n_atoms = len(radii)
        self._atoms = [_Atom(float(r)) for r in radii]

    @property
    def atoms(self):
        return iter(self._atoms)


class Frame:
    """what the reference reads of a one-frame mdtraj.Trajectory"""

    def __init__(self, xyz, radii):
        self.xyz = np.ascontiguousarray(xyz[None], dtype=np.float32)
        self.top = _Top(radii)


def reference_case(ref, xyz, elements, spacing, probe):
    struct = Frame(xyz, [npk.RADII[str(e)] for e in elements])
    grid = ref.create_grid(struct, spacing)
    T = ref.determine_touches_protein(struct, grid, probe)
    rank = np.zeros(T.shape)
    ref._check_cartesian_axis(T, rank)
    ref._check_cartesian_axis(T.swapaxes(0, 1), rank.swapaxes(0, 1))
    ref._check_cartesian_axis(T.swapaxes(0, 2), rank.swapaxes(0, 2))
    ref._check_diagonal_axis(T, rank)
    ref._check_diagonal_axis(T[::-1, :, :], rank[::-1, :, :])
    ref._check_diagonal_axis(T[::-1, ::-1, :], rank[::-1, ::-1, :])
    ref._check_diagonal_axis(T[:, ::-1, :], rank[:, ::-1, :])
    out = {"dims": np.array(T.shape, dtype=np.int32),
           "ax0": grid[:, 0, 0, 0].copy(), "ax1": grid[0, :, 0, 1].copy(),
           "ax2": grid[0, 0, :, 2].copy(),
           "touches": np.packbits(T.ravel()), "ranks": rank.astype(np.uint8)}
    assert np.array_equal(out["ranks"], rank)
    for m in (3, 5):
        cells = ref.get_pocket_cells(struct, grid_spacing=spacing, probe_radius=probe, min_rank=m)
        assert np.array_equal(cells, grid[np.where(rank >= m)])
        if len(cells) > 1:
            fc = scipy.cluster.hierarchy.fclusterdata(cells, t=spacing * 1.5,
                                                      criterion="distance")
        else:
            fc = np.ones(len(cells))
        out["fc%d" % m] = fc.astype(np.int32)
    return out


def main():
    ref = load_reference()
    E = np.load(os.path.join(HERE, "exposons_golden.npz"))
    out, names, spacings, probes = {}, [], [], []
    inputs = [("bp%d" % f, E["bp_xyz"][f], E["bp_elements"], "abc") for f in range(6)]
    for k, args in enumerate(SHELLS):
        xyz, elements = shell(*args)
        out["shell%d_xyz" % k], out["shell%d_elements" % k] = xyz, elements
        inputs.append(("shell%d" % k, xyz, elements, "ab"))
    for name, xyz, elements, settings in inputs:
        for s in settings:
            spacing, probe = SETTINGS[s]
            case = "%s_%s" % (name, s)
            res = reference_case(ref, xyz, elements, spacing, probe)
            for key, val in res.items():
                out["%s_%s" % (case, key)] = val
            names.append(case)
            spacings.append(spacing)
            probes.append(probe)
            r = res["ranks"]
            print("%-9s dims %-14s touching %5d  ranks present %s  pocket cells %d / %d, "
                  "pockets %d / %d"
                  % (case, tuple(int(d) for d in res["dims"]), np.unpackbits(res["touches"]).sum(),
                     "".join(str(v) for v in np.unique(r)), len(res["fc3"]), len(res["fc5"]),
                     len(set(res["fc3"])), len(set(res["fc5"]))))
    out["cases"], out["spacing"], out["probe"] = (np.array(names), np.array(spacings),
                                                  np.array(probes))
    path = os.path.join(HERE, "pockets_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
