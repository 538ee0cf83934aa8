"""Prinz's reversible maximum-likelihood iteration in plain numpy: the reference
of tests/test_msm_mle_host.py and tests/test_gpu_msm_mle.py.

Written from Prinz et al., J. Chem. Phys. 134, 174105 (2011), in the operation
order the library documents for its kernel (enspara_amd/csrc/ek_msm_mle.hip): per
sweep, for every state

    den = C_rs[i] - C[i,i];  if den > 0: X[i,i] = C[i,i] * (X_rs[i] - X[i,i]) / den
    X_rs[i] += (new X[i,i] - old X[i,i])
    logl    += C[i,i] * log(X[i,i] / X_rs[i])                      if X[i,i] > 0

then for every pair i < j in lexicographic order, with x = X[i,j] = X[j,i],

    a = (C_rs[i] - C[i,j]) + (C_rs[j] - C[j,i])
    b = C_rs[i] (X_rs[j] - x) + C_rs[j] (X_rs[i] - x)
        - (C[i,j] + C[j,i]) (X_rs[i] + X_rs[j] - 2 x)
    c = -(C[i,j] + C[j,i]) (X_rs[i] - x) (X_rs[j] - x)
    v = x if a == 0 else (-b + sqrt(b b - 4 a c)) / (2 a)
    X_rs[i] += v - x;  X_rs[j] += v - x;  X[i,j] = X[j,i] = v
    logl += C[i,j] log(v) / X_rs[i] + C[j,i] log(v) / X_rs[j]      if v > 0

and another sweep follows while |logl - logl of the sweep before| > tol.

Two forms: `sequential` does exactly that, one pair after the other, over ALL
pairs; `levelled` takes the pairs with C[i,j] + C[j,i] > 0 level by level
(`levels_of`), a level's pairs at once as numpy arrays, for sizes the Python loop
is too slow for.  Every operation of X and X_rs is a single IEEE operation in
both, so the two agree bit for bit where the level argument holds
(tests/test_msm_mle_host.py checks that they do); logl is summed in each form's
own order and returned with the number of its terms and the sum of their
magnitudes, which bound what a reordering can change.
"""
import numpy as np


def _start(C):
    C = np.array(C, dtype=np.float64)
    X = C + C.T
    return C, X, X.sum(axis=1), C.sum(axis=1)


def _result(X, X_rs, logls, mags, terms, n_iter):
    return {"X": X, "X_rs": X_rs, "logl": np.array(logls), "abs": np.array(mags),
            "P": np.array(terms), "n_iter": n_iter}


def sequential(C, max_iter, tol=-1.0):
    """-> dict: X, X_rs after the sweeps; per sweep logl, sum |term| (`abs`) and the
    number of terms (`P`); n_iter = sweeps that ran"""
    C, X, X_rs, C_rs = _start(C)
    n = len(C)
    logls, mags, terms = [], [], []
    oldlogl = 0.0
    n_iter = 0
    for _ in range(max_iter):
        logl, mag, P = 0.0, 0.0, 0
        for i in range(n):
            old = X[i, i]
            den = C_rs[i] - C[i, i]
            if den > 0:
                X[i, i] = C[i, i] * (X_rs[i] - X[i, i]) / den
            X_rs[i] = X_rs[i] + (X[i, i] - old)
            if X[i, i] > 0:
                t = C[i, i] * np.log(X[i, i] / X_rs[i])
                logl += t
                mag += abs(t)
                P += 1
        for i in range(n - 1):
            for j in range(i + 1, n):
                x = X[i, j]
                s = C[i, j] + C[j, i]
                a = (C_rs[i] - C[i, j]) + (C_rs[j] - C[j, i])
                b = (C_rs[i] * (X_rs[j] - x) + C_rs[j] * (X_rs[i] - x)
                     - s * (X_rs[i] + X_rs[j] - 2 * x))
                c = -s * (X_rs[i] - x) * (X_rs[j] - x)
                if a == 0:
                    v = x
                else:
                    v = (-b + np.sqrt(b * b - 4 * a * c)) / (2 * a)
                X_rs[i] = X_rs[i] + (v - x)
                X_rs[j] = X_rs[j] + (v - x)
                X[i, j] = v
                X[j, i] = v
                if v > 0:
                    t1 = C[i, j] * np.log(v) / X_rs[i]
                    t2 = C[j, i] * np.log(v) / X_rs[j]
                    logl += t1 + t2
                    mag += abs(t1) + abs(t2)
                    P += 2
        logls.append(logl)
        mags.append(mag)
        terms.append(P)
        n_iter += 1
        if abs(logl - oldlogl) > tol:
            oldlogl = logl
        else:
            break
    return _result(X, X_rs, logls, mags, terms, n_iter)


def levels_of(C):
    """(i, j, level) of the pairs i < j with C[i,j] + C[j,i] > 0, in lexicographic
    order: level = 1 + max(last[i], last[j]), last[s] = level of the latest earlier
    pair with state s, -1 if there is none.  (A full pattern gives i + j - 1, which
    is what is returned for one without walking the n^2 / 2 pairs in Python.)"""
    C = np.asarray(C, dtype=np.float64)
    n = len(C)
    S = C + C.T
    I, J = np.nonzero(np.triu(S > 0, 1))
    if len(I) == n * (n - 1) // 2:
        return I, J, I + J - 1
    last = [-1] * n
    level = np.empty(len(I), dtype=np.int64)
    for p, (i, j) in enumerate(zip(I.tolist(), J.tolist())):
        lv = 1 + max(last[i], last[j])
        level[p] = last[i] = last[j] = lv
    return I, J, level


def levelled(C, max_iter, tol=-1.0):
    """the same sweeps, the pairs that are not zero level by level"""
    C, X, X_rs, C_rs = _start(C)
    n = len(C)
    I, J, level = levels_of(C)
    order = np.argsort(level, kind="stable")
    I, J, level = I[order], J[order], level[order]
    n_levels = int(level[-1]) + 1 if len(level) else 0
    ptr = np.searchsorted(level, np.arange(n_levels + 1))
    cij, cji, xp = C[I, J], C[J, I], X[I, J]
    cd, xd = np.diagonal(C).copy(), np.diagonal(X).copy()
    logls, mags, terms = [], [], []
    oldlogl = 0.0
    n_iter = 0
    for _ in range(max_iter):
        den = C_rs - cd
        with np.errstate(all="ignore"):
            nx = np.where(den > 0, cd * (X_rs - xd) / den, xd)
        X_rs = X_rs + (nx - xd)
        xd = nx
        pos = xd > 0
        t = cd[pos] * np.log(xd[pos] / X_rs[pos])
        logl, mag, P = float(t.sum()), float(np.abs(t).sum()), int(pos.sum())
        for lv in range(n_levels):
            q = slice(ptr[lv], ptr[lv + 1])
            i, j = I[q], J[q]
            x, cq, cp = xp[q], cij[q], cji[q]
            cri, crj, xri, xrj = C_rs[i], C_rs[j], X_rs[i], X_rs[j]
            s = cq + cp
            a = (cri - cq) + (crj - cp)
            b = cri * (xrj - x) + crj * (xri - x) - s * (xri + xrj - 2 * x)
            c = -s * (xri - x) * (xrj - x)
            with np.errstate(all="ignore"):
                v = (-b + np.sqrt(b * b - 4 * a * c)) / (2 * a)
            v = np.where(a == 0, x, v)
            xri = xri + (v - x)
            xrj = xrj + (v - x)
            X_rs[i] = xri
            X_rs[j] = xrj
            xp[q] = v
            pos = v > 0
            lg = np.log(v[pos])
            t1 = cq[pos] * lg / xri[pos]
            t2 = cp[pos] * lg / xrj[pos]
            logl += float((t1 + t2).sum())
            mag += float(np.abs(t1).sum() + np.abs(t2).sum())
            P += 2 * int(pos.sum())
        logls.append(logl)
        mags.append(mag)
        terms.append(P)
        n_iter += 1
        if abs(logl - oldlogl) > tol:
            oldlogl = logl
        else:
            break
    X = np.zeros((n, n))
    X[I, J] = xp
    X[J, I] = xp
    X[np.arange(n), np.arange(n)] = xd
    return _result(X, X_rs, logls, mags, terms, n_iter)


def finish(X, X_rs):
    """transition probabilities and populations of an iterate"""
    return X / X.sum(axis=-1).reshape(len(X), 1), X_rs / X_rs.sum()


# ---- the inputs both test files use ---------------------------------------------
def dense_counts(n, seed):
    """integer counts, every cell positive"""
    return np.random.RandomState(seed).randint(1, 50, size=(n, n)).astype(np.float64)


def sparse_counts(n, fill, seed):
    """about `fill` of the cells counted, plus a ring i -> i + 1 so that every row
    of C has counts; the diagonal partly empty"""
    rng = np.random.RandomState(seed)
    C = rng.randint(1, 30, size=(n, n)) * (rng.rand(n, n) < fill)
    C[np.arange(n), (np.arange(n) + 1) % n] += 1 + rng.randint(0, 5, size=n)
    return C.astype(np.float64)
