"""Want side of the sharded feature-space PAM tests (TEST CODE).

A host restatement of the reference's MPI sweep (kmedoids.py:575-699 with the
cost of :478-479 in its MPI form: every rank's np.sum(d ** 2), added in rank
order, over the global sample count) on the CONCATENATED samples with the
oracle's metrics (oracle/features.py).  Line by line oracle/cluster.py's
``pam_update_numpy``; the one difference is ``_cost``.  Pinned to it in
tests/test_feature_pam_gloo.py (one shard: the two are the same function)."""
import numpy as np

from oracle import features as of

METRICS = {0: of.euclidean, 1: of.manhattan, 2: of.hamming}


def _cost(d, bounds):
    s = 0.0
    for r in range(len(bounds) - 1):                 # rank order
        s += float(np.sum(d[bounds[r]:bounds[r + 1]] ** 2))
    return s / len(d)


def pam_update_mpi(X, mid, medoid_inds, assignments, distances, bounds,
                   proposals=None, random_state=None):
    """-> (medoid_inds, distances float64, assignments int64)"""
    metric = METRICS[mid]
    if not isinstance(random_state, np.random.RandomState):
        random_state = np.random.RandomState(random_state)
    medoid_inds = [int(i) for i in medoid_inds]
    medoid_rows = [X[i] for i in medoid_inds]
    distances = np.asarray(distances, dtype=np.float64)
    assignments = np.asarray(assignments, dtype=np.int64)
    for cid in range(len(medoid_inds)):
        members = np.flatnonzero(assignments == cid)         # :611
        if proposals is None:
            prop = int(random_state.choice(members))         # :514
        else:
            prop = int(proposals[cid])
        nd = metric(X, X[prop])                              # :637
        new_dist = np.zeros_like(distances) - 1
        new_assig = np.zeros_like(assignments) - 1
        down = distances > nd                                # :644
        new_assig[down] = cid
        new_dist[down] = nd[down]
        up_other = (distances <= nd) & (assignments != cid)  # :651
        new_assig[up_other] = assignments[up_other]
        new_dist[up_other] = distances[up_other]
        up_this = (distances <= nd) & (assignments == cid)   # :658
        trial = list(medoid_rows)
        trial[cid] = X[prop]
        sub = np.flatnonzero(up_this)
        if len(sub):
            sa, sd = of.assign_to_nearest_center(X[sub], np.array(trial),
                                                 metric)     # :666
            new_assig[sub] = sa
            new_dist[sub] = sd
        if _cost(new_dist, bounds) < _cost(distances, bounds):   # :680-683
            distances, assignments = new_dist, new_assig
            medoid_rows = trial
            medoid_inds[cid] = prop
    return medoid_inds, distances, assignments


def start_kcenters(X, mid, K, init_centers=None):
    """k-centers by the reference-shaped host loop around the oracle's metric
    -> (center indices, assignments int64, distances float64)"""
    from enspara_amd.cluster.kcenters import kcenters
    f = METRICS[mid]
    r = kcenters(X, lambda A, y: f(np.asarray(A), np.asarray(y)), n_clusters=K,
                 init_centers=init_centers)
    return ([int(i) for i in r.center_indices],
            np.asarray(r.assignments, dtype=np.int64),
            np.asarray(r.distances, dtype=np.float64))


def start_nearest(X, mid, med):
    a, d = of.assign_to_nearest_center(X, X[np.asarray(med)], METRICS[mid])
    return a, d


def khybrid_want(X, mid, K, n_iters, seed, bounds, init_centers=None):
    med, a, d = start_kcenters(X, mid, K, init_centers)
    rs = np.random.RandomState(seed)
    for _ in range(n_iters):
        med, d, a = pam_update_mpi(X, mid, med, a, d, bounds, random_state=rs)
    return med, d, a


def cold_medoids(n, K, seed):
    """the single-process cold start (kmedoids.py:345-352)"""
    rng = np.random.default_rng(seed=seed)
    med = np.array([])
    while len(np.unique(med)) < K:
        med = rng.integers(0, n, K)
    return [int(g) for g in med]
