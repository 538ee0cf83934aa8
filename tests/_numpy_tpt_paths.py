"""A plain numpy restatement of enspara_amd.tpt.path (the reference's
enspara/tpt/path.py), written from the rule csrc/ek_tpt_path.hip states and not
from the reference's text; tests/test_tpt_paths_host.py pins it to the goldens
made with the real reference, bit for bit, and the GPU tests then use it as an
oracle on graphs made on the fly.

The rule.  A search keeps, per state, min_flux (-inf; +inf for the sources), the
edge it was last improved through, and the moment of its FIRST insertion into
the set of candidates: the sources first, in the order given (a repeat counts
where it first stands), then, for the node popped at step t, its improved
neighbours in ascending state index.  Each step pops the candidate with the
largest min_flux, the earliest insertion on ties, and marks it visited; the
search ends once every sink is visited or no candidate is left.  Popping u
offers every unvisited v with F[u, v] > 0 the value w = min(F[u, v],
min_flux[u]), taken iff w > min_flux[v].  The path ends at the first sink (in
the order given) with the largest min_flux and goes back along the improving
edges.

Works on a CSR of the matrix so that a graph of several thousand states takes
well under a second per path.
"""
import heapq

import numpy as np
import scipy.sparse

INF = np.inf


def as_csr(net_flux):
    """(n, indptr, cols, vals) with ascending columns; vals is a copy.  Entries that
    are not > 0 may be present: a search does not follow them."""
    F = scipy.sparse.csr_matrix(net_flux, dtype=np.float64, copy=True)
    F.sum_duplicates()
    F.sort_indices()
    assert F.shape[0] == F.shape[1]
    return F.shape[0], F.indptr.astype(np.int64), F.indices.astype(np.int64), F.data.copy()


def total_flux(net_flux, sources):
    """numpy's sum over the sources' rows of the (dense equivalent of the) matrix"""
    sources = np.array(sources, dtype=int).reshape(-1)
    if scipy.sparse.issparse(net_flux):
        rows = scipy.sparse.csr_matrix(net_flux, dtype=np.float64)[sources, :].toarray()
    else:
        rows = np.asarray(net_flux, dtype=np.float64)[sources, :]
    return rows.sum()


def search(sources, sinks, n, indptr, cols, vals):
    """-> (path int64, flux, the CSR slots of the path's edges from the source on,
    pops)"""
    sources = np.array(sources, dtype=int).reshape(-1)
    sinks = np.array(sinks, dtype=int).reshape(-1)
    min_flux = np.full(n, -INF)
    slot = np.full(n, -1, dtype=np.int64)
    before = np.full(n, -1, dtype=np.int64)
    visited = np.zeros(n, dtype=bool)
    queued = np.zeros(n, dtype=bool)
    order = np.zeros(n, dtype=np.int64)
    # the candidates as a heap of (-min_flux, first insertion, state); an entry whose
    # state was visited or improved since is stale and skipped when it surfaces
    candidates = []
    for rank, s in enumerate(sources):
        if not queued[s]:
            queued[s] = True
            order[s] = rank
            min_flux[s] = INF
            heapq.heappush(candidates, (-INF, rank, int(s)))
    is_sink = np.zeros(n, dtype=bool)
    is_sink[sinks] = True
    sinks_left = int(is_sink.sum())
    step = 0
    while candidates:
        neg, _, u = heapq.heappop(candidates)
        if visited[u] or -neg != min_flux[u]:
            continue
        step += 1
        assert step <= n
        visited[u] = True
        if is_sink[u]:
            sinks_left -= 1
        if sinks_left == 0:
            break
        lo, hi = indptr[u], indptr[u + 1]
        v, f = cols[lo:hi], vals[lo:hi]
        w = np.where(f > min_flux[u], min_flux[u], f)
        take = np.flatnonzero((f > 0) & ~visited[v] & (w > min_flux[v]))
        for k in take:                  # ascending state index
            x = int(v[k])
            min_flux[x] = w[k]
            slot[x] = lo + k
            before[x] = u
            if not queued[x]:
                queued[x] = True
                order[x] = step * n + x
            heapq.heappush(candidates, (-float(w[k]), int(order[x]), x))
    end = int(sinks[np.argmax(min_flux[sinks])])
    path, slots = [end], []
    while before[path[-1]] != -1:
        assert len(path) <= n
        slots.append(int(slot[path[-1]]))
        path.append(int(before[path[-1]]))
    return (np.array(path[::-1], dtype=np.int64), float(min_flux[end]),
            np.array(slots[::-1], dtype=np.int64), step)


def top_path(sources, sinks, net_flux):
    n, indptr, cols, vals = as_csr(net_flux)
    path, flux, _, _ = search(sources, sinks, n, indptr, cols, vals)
    return path, flux


def remove(vals, slots, how):
    """take a path (its edges' slots, from the source on) out of the CSR values"""
    if how == 'subtract':
        vals[slots] = vals[slots] - vals[slots].min()
    else:
        assert how == 'bottleneck'
    vals[slots[np.argmin(vals[slots])]] = 0.0


def paths(sources, sinks, net_flux, remove_path='subtract', num_paths=np.inf,
          flux_cutoff=(1 - 1E-10), return_pops=False):
    if remove_path not in ('subtract', 'bottleneck'):
        raise ValueError(remove_path)
    n, indptr, cols, vals = as_csr(net_flux)
    total = np.float64(total_flux(net_flux, sources))
    found, fluxes, pops = [], [], []
    explained = np.float64(0.0)
    with np.errstate(all="ignore"):
        while True:
            path, flux, slots, steps = search(sources, sinks, n, indptr, cols, vals)
            pops.append(steps)
            if np.isinf(flux):
                break
            found.append(path)
            fluxes.append(flux)
            explained = explained + np.float64(flux) / total
            if len(found) >= num_paths or explained >= flux_cutoff:
                break
            remove(vals, slots, remove_path)
    out = (found, np.array(fluxes, dtype=np.float64))
    return out + (pops,) if return_pops else out


# ---- tests/golden/tpt_paths_golden.npz (make_tpt_paths_golden.py says what is in it) ------
MODES = (("sub", "subtract"), ("bot", "bottleneck"))


def golden_case(g, name):
    """-> dict: F (dense), src, snk, num_paths, cut {mode: flux_cutoff}, top (path, flux),
    want {mode: (paths, fluxes)}"""
    n = int(g["n_" + name])
    F = np.zeros((n, n))
    F[g["i_" + name], g["j_" + name]] = g["v_" + name]
    want = {}
    for tag, how in MODES:
        nodes, off = g["%s_nodes_%s" % (tag, name)], g["%s_off_%s" % (tag, name)]
        want[how] = ([nodes[off[p]:off[p + 1]] for p in range(len(off) - 1)],
                     g["%s_flux_%s" % (tag, name)])
    return {"F": F, "src": g["src_" + name], "snk": g["snk_" + name],
            "num_paths": float(g["np_" + name]),
            "cut": {"subtract": float(g["cut_" + name]),
                    "bottleneck": float(g["cutb_" + name])},
            "top": (g["top_path_" + name], float(g["top_flux_" + name])), "want": want}


def assert_same_paths(got, want, what=""):
    """paths equal as arrays (int64), fluxes bit for bit (float64)"""
    (gp, gf), (wp, wf) = got, want
    assert isinstance(gp, list) and len(gp) == len(wp), (what, len(gp), len(wp))
    for k, (a, b) in enumerate(zip(gp, wp)):
        assert a.dtype == np.int64 and np.array_equal(a, b), (what, k, a, b)
    gf = np.asarray(gf)
    assert gf.dtype == np.float64 and gf.shape == (len(wp),), (what, gf.dtype, gf.shape)
    assert gf.tobytes() == np.asarray(wf, dtype=np.float64).tobytes(), (what, gf, wf)


# ---- graphs the tests and the golden generator make -------------------------------------
def random_fluxes(n, density, kind, seed):
    """a seeded n x n matrix with about density * n^2 entries > 0 and a zero diagonal:
    kind 'int' draws them from {1, 2, 3} (ties at every pop), 'tenths' from {0.1, 0.2},
    'uniform' from (0, 1)"""
    rng = np.random.RandomState(seed)
    mask = rng.rand(n, n) < density
    np.fill_diagonal(mask, False)
    if kind == 'int':
        vals = rng.randint(1, 4, size=(n, n)).astype(np.float64)
    elif kind == 'tenths':
        vals = rng.randint(1, 3, size=(n, n)) / 10.0
    else:
        assert kind == 'uniform'
        vals = rng.rand(n, n)
    return np.where(mask, vals, 0.0)


def sparse_fluxes(n, per_row, seed):
    """a seeded CSR matrix of n states with per_row entries from (0, 1) in every row, a
    chain 0 -> 1 -> .. among them so that the last state can be reached from the first"""
    rng = np.random.RandomState(seed)
    i = np.repeat(np.arange(n), per_row)
    j = rng.randint(0, n, size=n * per_row)
    j[::per_row] = (np.arange(n) + 1) % n
    v = rng.rand(n * per_row) + 0.01
    keep = i != j
    # (a pair drawn twice is summed: still > 0)
    return scipy.sparse.csr_matrix((v[keep], (i[keep], j[keep])), shape=(n, n))
