"""ctypes front of ek_pam_pairs_probe (include/enspara_hip.h) and the oracle's
statement of what it must return.  Shared by tests/test_gpu_pam_pairs.py and
tests/_lifetime_cases.py.  Inputs are centred float32 structures and float64 traces,
as oracle.qcp.center_and_trace gives them."""
import ctypes as C

import numpy as np

from enspara_amd import _lib

GROUP = 8                       # EK_PAM_GROUP: columns per dmin row
FILL = np.uint32(0x7FC0BEEF)    # a NaN no kernel computes: "never written"


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _filled(*shape):
    return np.full(shape, FILL, dtype=np.uint32).view(np.float32)


def _f32(a, width=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.reshape(len(a), width if width is not None else a[0].size)


def tables(form, rows, rows_G, cols, cols_G, held, old_lo, n_old, dprop=None, device=0):
    """rows [K + 1][A][3] (row K: the held medoid), cols [n_col][A][3] -> T [n_col][K],
    O [n_old][K], dmin [ceil(n_col / 8)][K], each FILL where nothing was written"""
    rows = _f32(rows)
    cols = _f32(cols, rows.shape[1])
    K, n_col, A = len(rows) - 1, len(cols), rows.shape[1] // 3
    rows_G = np.ascontiguousarray(rows_G, dtype=np.float64)
    cols_G = np.ascontiguousarray(cols_G, dtype=np.float64)
    if dprop is not None:
        dprop = np.ascontiguousarray(dprop, dtype=np.float32)
        assert len(dprop) == n_col
    T, O = _filled(n_col, K), _filled(n_old, K)
    dmin = _filled((n_col + GROUP - 1) // GROUP, K)
    _lib.check(_lib.load().ek_pam_pairs_probe(
        device, form, A, _p(rows), _p(rows_G), len(rows), _p(cols), _p(cols_G), n_col,
        K, held, old_lo, n_old, _p(dprop), _p(T), _p(O), _p(dmin), None, 0, 0, None))
    return T, O, dmin


def listed(form, rows, rows_G, cols, cols_G, lst, n_pad, device=0):
    """vecs [n_col][n_pad]: rmsd(row lst[i], column j) at [j][lst[i]], FILL elsewhere"""
    rows = _f32(rows)
    cols = _f32(cols, rows.shape[1])
    A = rows.shape[1] // 3
    rows_G = np.ascontiguousarray(rows_G, dtype=np.float64)
    cols_G = np.ascontiguousarray(cols_G, dtype=np.float64)
    lst = np.ascontiguousarray(lst, dtype=np.uint32)
    vecs = _filled(len(cols), n_pad)
    _lib.check(_lib.load().ek_pam_pairs_probe(
        device, form, A, _p(rows), _p(rows_G), len(rows), _p(cols), _p(cols_G), len(cols),
        0, -1, 0, 0, None, None, None, None, _p(lst), len(lst), n_pad, _p(vecs)))
    return vecs


# ---- what the oracle says --------------------------------------------------------------------
def _group_min(T):
    n_col, K = T.shape
    out = np.empty(((n_col + GROUP - 1) // GROUP, K), dtype=np.float32)
    for g in range(len(out)):
        out[g] = T[GROUP * g:GROUP * (g + 1)].min(axis=0)
    return out


def want_tables(rows, rows_G, cols, cols_G, held, old_lo, n_old, dprop=None):
    """oracle.qcp.rmsd_centered of the same arrays: the medoid table (row `held` replaced by
    row K) against every column / against its own rows old_lo ..; dmin the float32
    minimum over each group of 8 live columns; with dprop, T and dmin from O"""
    from oracle import qcp
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    K, A = len(rows) - 1, rows.shape[1]
    med, med_G = rows[:K].copy(), np.array(rows_G[:K], dtype=np.float64)
    if held >= 0:
        med[held], med_G[held] = rows[K], rows_G[K]
    O = np.empty((n_old, K), dtype=np.float32)
    for i in range(n_old):
        O[i] = qcp.rmsd_centered(med, med_G, med[old_lo + i], med_G[old_lo + i])
    if dprop is not None:
        dprop = np.asarray(dprop, dtype=np.float32)
        T = np.maximum(O - dprop[:, None], np.float32(0))
        assert T.dtype == np.float32
    else:
        T = np.empty((len(cols), K), dtype=np.float32)
        for j in range(len(cols)):
            T[j] = qcp.rmsd_centered(med, med_G, cols[j].reshape(A, 3), cols_G[j])
    return T, O, _group_min(T)


def want_listed(rows, rows_G, cols, cols_G, lst, n_pad):
    from oracle import qcp
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    A = rows.shape[1]
    lst = np.asarray(lst, dtype=np.int64)
    sub, sub_G = np.ascontiguousarray(rows[lst]), np.ascontiguousarray(rows_G[lst])
    vecs = _filled(len(cols), n_pad)
    for j in range(len(cols)):
        vecs[j, lst] = qcp.rmsd_centered(sub, sub_G, cols[j].reshape(A, 3), cols_G[j])
    return vecs


def same_bits(got, want, what):
    got, want = got.view(np.uint32), want.view(np.uint32)
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d of %d entries differ, first at %s: got %r want %r" % (
        what, len(bad), want.size, tuple(bad[0]),
        got[tuple(bad[0])].view(np.float32), want[tuple(bad[0])].view(np.float32))
