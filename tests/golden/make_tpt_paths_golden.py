#!/usr/bin/env python3
"""Generate tests/golden/tpt_paths_golden.npz by running the REAL reference's
path searches (bowman-lab/enspara, enspara/tpt/path.py: top_path and paths) on
small graphs.

    python tests/golden/make_tpt_paths_golden.py

The reference's path.py needs nothing but numpy, so it is loaded by file path;
nothing is compiled.  Only inputs and outputs are stored; no reference source is
copied.

`cases` lists the case names.  A case `<c>` stores
  n_<c>                    the number of states
  i_<c>, j_<c>, v_<c>      the matrix as COO triples (row-major order, the entries
                           that are not zero), float64 values
  src_<c>, snk_<c>         sources and sinks as given (int64; unsorted and
                           repeated where the case says so)
  np_<c>, cut_<c>          num_paths (float64, inf = the default) and flux_cutoff
  top_path_<c>, top_flux_<c>
                           top_path(src, snk, F)
  sub_nodes_<c>, sub_off_<c>, sub_flux_<c>
                           paths(..., remove_path='subtract'): the paths one after
                           the other, path p = nodes[off[p]:off[p + 1]], and the
                           fluxes (shape (0,) when there is none)
  bot_nodes_<c>, bot_off_<c>, bot_flux_<c>
                           the same for remove_path='bottleneck'

The cases:
  table6        the 6-state table of the reference's own test_paths, sources [0],
                sinks [4, 5]: [0, 2, 4], [0, 1, 3, 5], [0, 1, 5] with 0.5, 0.3, 0.2
  pair, pair0   n = 2 with the one edge 0 -> 1, and with none (the sink cannot be
                reached: top_path gives ([1], -inf), paths nothing)
  ties40        n = 40, fluxes from {1, 2, 3} at density 0.3 (ties at every pop),
                sources [7, 3, 7], sinks [20, 39, 31] of which 39 has no way in
  ties40_both   the same with sinks [20, 3]: 3 is a source too, so no path
  ties40_np0, ties40_np1, ties40_np3
                ties40 with num_paths 0, 1, 3 (the test follows the append: 1, 1, 3)
  ties40_cut    ties40 with a flux_cutoff that the second path crosses, per mode
                (cut_ holds the subtract run's, cutb_ the bottleneck run's)
  chain300      0 -> 1 -> ... -> 299 with fluxes in [1, 2) and a few shortcuts of
                lower flux: the first path visits every state, later ones take
                the shortcuts
  star63, star64, star65, star257
                a hub 0 with that many leaves, each leading on to the one sink:
                degrees around the wave (64) and the search workgroup (256)
  flux17, flux65
                net fluxes of the chains n17 and n65 of tpt_golden.npz for set A
                (sources [0], sinks [n - 1]): ref_n17_nA, the reference's own
                output, and hp_n65_nA

The generator checks itself: the numpy restatement (tests/_numpy_tpt_paths.py) must
give every stored result bit for bit, and what the docstring promises of a case
(table6's paths, the path counts of the num_paths cases, the full-length first path
of chain300) is asserted before the file is written.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
from make_golden import REF  # noqa: E402
import _numpy_tpt_paths as npp  # noqa: E402


def import_reference_path():
    spec = importlib.util.spec_from_file_location(
        "enspara_ref_tpt_path", os.path.join(REF, "enspara", "tpt", "path.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def star(leaves, seed):
    rng = np.random.RandomState(seed)
    n = leaves + 2
    F = np.zeros((n, n))
    F[0, 1:leaves + 1] = rng.randint(1, 4, size=leaves)
    F[1:leaves + 1, n - 1] = rng.randint(1, 4, size=leaves)
    return F


def chain300():
    n = 300
    rng = np.random.RandomState(300)
    F = np.zeros((n, n))
    F[np.arange(n - 1), np.arange(1, n)] = 1.0 + rng.randint(1, 8, size=n - 1) / 8.0
    for a, b, f in ((150, 151, 1.0),    # the chain's one bottleneck; 100 -> 200 goes round it
(0, 299, 0.125), (10, 50, 0.25), (100, 200, 0.5), (40, 45, 0.75),
                    (250, 299, 0.375)):
        F[a, b] = f
    return F


def ties40():
    F = npp.random_fluxes(40, 0.3, 'int', 40)
    F[:, 39] = 0.0
    return F


def build_cases():
    tg = np.load(os.path.join(HERE, "tpt_golden.npz"))
    table6 = np.zeros((6, 6))
    for a, b, f in ((0, 1, 0.5), (0, 2, 0.5), (1, 3, 0.3), (1, 5, 0.2), (2, 4, 0.5),
                    (3, 5, 0.3)):
        table6[a, b] = f
    T = ties40()
    src, snk = [7, 3, 7], [20, 39, 31]
    cases = [
        ("table6", table6, [0], [4, 5], {}),
        ("pair", np.array([[0.0, 0.7], [0.0, 0.0]]), [0], [1], {}),
        ("pair0", np.zeros((2, 2)), [0], [1], {}),
        ("ties40", T, src, snk, {}),
        ("ties40_both", T, src, [20, 3], {}),
        ("ties40_np0", T, src, snk, {"num_paths": 0}),
        ("ties40_np1", T, src, snk, {"num_paths": 1}),
        ("ties40_np3", T, src, snk, {"num_paths": 3}),
        ("ties40_cut", T, src, snk, {"flux_cutoff": "second"}),
        ("chain300", chain300(), [0], [299], {}),
    ]
    for leaves in (63, 64, 65, 257):
        cases.append(("star%d" % leaves, star(leaves, leaves), [0], [leaves + 1], {}))
    cases.append(("flux17", tg["ref_n17_nA"], [0], [16], {}))
    cases.append(("flux65", tg["hp_n65_nA"], [0], [64], {}))
    return cases


def pack(found):
    off = np.zeros(len(found) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in found])
    nodes = np.concatenate(found).astype(np.int64) if found else np.zeros(0, dtype=np.int64)
    return nodes, off


def same(a, b):
    (pa, fa), (pb, fb) = a, b
    fa, fb = np.asarray(fa, dtype=np.float64), np.asarray(fb, dtype=np.float64)
    return (len(pa) == len(pb) and all(np.array_equal(x, y) for x, y in zip(pa, pb)) and
            fa.tobytes() == fb.tobytes())


def main():
    ref = import_reference_path()
    out, names = {}, []
    for name, F, src, snk, kw in build_cases():
        F = np.ascontiguousarray(F, dtype=np.float64)
        assert np.all(np.isfinite(F))
        n = F.shape[0]
        i, j = np.nonzero(F)
        out["n_" + name] = np.array(n)
        out["i_" + name], out["j_" + name] = i.astype(np.int32), j.astype(np.int32)
        out["v_" + name] = F[i, j]
        out["src_" + name] = np.array(src, dtype=np.int64)
        out["snk_" + name] = np.array(snk, dtype=np.int64)
        path, flux = ref.top_path(src, snk, F.copy())
        out["top_path_" + name] = np.asarray(path, dtype=np.int64)
        out["top_flux_" + name] = np.array(float(flux))
        assert same(([path], [flux]), ([npp.top_path(src, snk, F)[0]],
                                       [npp.top_path(src, snk, F)[1]])), name
        num_paths = float(kw.get("num_paths", np.inf))
        out["np_" + name] = np.array(num_paths)
        counts = []
        for tag, how in (("sub", "subtract"), ("bot", "bottleneck")):
            cut = kw.get("flux_cutoff", 1 - 1E-10)
            if cut == "second":
                # between what one path and what two paths explain
                _, f = ref.paths(src, snk, F.copy(), remove_path=how)
                total = F[src, :].sum()
                e1 = 0.0 + f[0] / total
                e2 = e1 + f[1] / total
                cut = (e1 + e2) / 2
                assert e1 < cut < e2 and len(f) > 2
            out[("cut_" if tag == "sub" else "cutb_") + name] = np.array(cut)
            res = ref.paths(src, snk, F.copy(), remove_path=how, num_paths=num_paths,
                            flux_cutoff=cut)
            mine = npp.paths(src, snk, F, remove_path=how, num_paths=num_paths,
                             flux_cutoff=cut)
            assert same(res, mine), (name, how)
            nodes, off = pack(res[0])
            out["%s_nodes_%s" % (tag, name)] = nodes
            out["%s_off_%s" % (tag, name)] = off
            out["%s_flux_%s" % (tag, name)] = np.asarray(res[1], dtype=np.float64).reshape(-1)
            counts.append(len(res[0]))
            if name == "table6":
                assert [list(p) for p in res[0]] == [[0, 2, 4], [0, 1, 3, 5], [0, 1, 5]]
                assert np.allclose(res[1], [0.5, 0.3, 0.2], rtol=1e-15, atol=0)
            if name == "chain300" and how == "subtract":
                assert list(res[0][0]) == list(range(300)) and len(res[0]) >= 2
            if name == "ties40_cut":
                assert len(res[0]) == 2
        if name in ("pair0", "ties40_both"):
            assert counts == [0, 0]
        if name.startswith("ties40_np"):
            assert counts == [max(int(num_paths), 1)] * 2
        if name == "pair0":
            assert list(path) == [1] and flux == -np.inf
        if name.startswith("star"):
            assert counts == [n - 2] * 2
        print("%-12s n %4d  entries %5d  paths %s  top %s" % (
            name, n, len(i), counts, float(flux)), flush=True)
        names.append(name)
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "tpt_paths_golden.npz")
    np.savez_compressed(path, **out)
    print("tpt_paths_golden.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
