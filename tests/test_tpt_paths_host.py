"""enspara_amd.tpt.path without a device: the numpy restatement the GPU tests lean on
(tests/_numpy_tpt_paths.py) against the goldens made with the real reference
(tests/golden/make_tpt_paths_golden.py), bit for bit; the argument checks, which run
before any device call; the C ABI's own; and the module's surface."""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.sparse

import _numpy_tpt_paths as npp
from enspara_amd import _lib
from enspara_amd.exception import DataInvalid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "tpt_paths_golden.npz")
CASES = ["table6", "pair", "pair0", "ties40", "ties40_both", "ties40_np0", "ties40_np1",
         "ties40_np3", "ties40_cut", "chain300", "star63", "star64", "star65", "star257",
         "flux17", "flux65"]
F3 = np.array([[0., 2., 1.], [0., 0., 2.], [0., 0., 0.]])


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_module_surface():
    import enspara_amd.tpt as tpt
    from enspara_amd.tpt import path
    assert path.__all__ == ['paths', 'top_path']
    assert callable(path.paths) and callable(path.top_path)
    assert not hasattr(tpt, "paths") and "paths" not in tpt.__all__
    assert "enspara_amd.tpt.path" in tpt.__doc__


# ---- the restatement against the goldens ---------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_reference(golden, name):
    c = npp.golden_case(golden, name)
    path, flux = npp.top_path(c["src"], c["snk"], c["F"])
    npp.assert_same_paths(([path], np.array([flux])), ([c["top"][0]], [c["top"][1]]), "top")
    for _, how in npp.MODES:
        got = npp.paths(c["src"], c["snk"], c["F"], remove_path=how,
                        num_paths=c["num_paths"], flux_cutoff=c["cut"][how])
        npp.assert_same_paths(got, c["want"][how], how)
        # a sparse matrix is its dense equivalent
        got = npp.paths(c["src"], c["snk"], scipy.sparse.lil_matrix(c["F"]), remove_path=how,
                        num_paths=c["num_paths"], flux_cutoff=c["cut"][how])
        npp.assert_same_paths(got, c["want"][how], how + " sparse")


def test_golden_is_what_its_docstring_says(golden):
    g = golden
    assert list(g["cases"]) == CASES
    assert os.path.getsize(GOLDEN) < 600 * 1024
    c = npp.golden_case(g, "table6")
    for _, how in npp.MODES:
        found, fluxes = c["want"][how]
        assert [list(p) for p in found] == [[0, 2, 4], [0, 1, 3, 5], [0, 1, 5]]
        np.testing.assert_allclose(fluxes, [0.5, 0.3, 0.2], rtol=1e-15, atol=0)
    assert list(c["src"]) == [0] and list(c["snk"]) == [4, 5]
    c = npp.golden_case(g, "pair0")
    assert list(c["top"][0]) == [1] and c["top"][1] == -np.inf
    assert all(len(c["want"][how][0]) == 0 and c["want"][how][1].shape == (0,)
               for _, how in npp.MODES)
    assert [len(npp.golden_case(g, "pair")["want"][how][0]) for _, how in npp.MODES] == [1, 1]
    c = npp.golden_case(g, "ties40")
    assert list(c["src"]) == [7, 3, 7] and list(c["snk"]) == [20, 39, 31]
    assert set(np.unique(c["F"])) == {0., 1., 2., 3.} and not c["F"][:, 39].any()
    assert c["num_paths"] == np.inf and c["cut"]["subtract"] == 1 - 1E-10
    assert 39 not in [p[-1] for how in c["want"] for p in c["want"][how][0]]
    both = npp.golden_case(g, "ties40_both")
    assert list(both["snk"]) == [20, 3] and both["top"][1] == np.inf
    assert all(len(both["want"][how][0]) == 0 for how in both["want"])
    for k, count in ((0, 1), (1, 1), (3, 3)):
        cc = npp.golden_case(g, "ties40_np%d" % k)
        assert cc["num_paths"] == k and np.array_equal(cc["F"], c["F"])
        assert all(len(cc["want"][how][0]) == count for how in cc["want"])
    cut = npp.golden_case(g, "ties40_cut")
    for how in cut["want"]:
        assert len(cut["want"][how][0]) == 2 < len(c["want"][how][0])
        f = c["want"][how][1]
        total = c["F"][c["src"], :].sum()
        assert f[0] / total < cut["cut"][how] <= f[0] / total + f[1] / total
    c = npp.golden_case(g, "chain300")
    assert list(c["want"]["subtract"][0][0]) == list(range(300))
    from enspara_amd.tpt import path
    for leaves in (63, 64, 65, path.SEARCH_WG + 1):
        c = npp.golden_case(g, "star%d" % leaves)
        assert int((c["F"][0] > 0).sum()) == leaves and c["F"].shape[0] == leaves + 2
        assert all(len(c["want"][how][0]) == leaves for how in c["want"])
    tg = np.load(os.path.join(os.path.dirname(GOLDEN), "tpt_golden.npz"))
    assert np.array_equal(npp.golden_case(g, "flux17")["F"], tg["ref_n17_nA"])
    assert np.array_equal(npp.golden_case(g, "flux65")["F"], tg["hp_n65_nA"])
    # more paths than one batch holds by default
    assert len(npp.golden_case(g, "flux65")["want"]["subtract"][0]) > 64


def test_restatement_orders_ties_by_first_insertion():
    # 0 -> {1, 2} -> 3, all fluxes equal: 1 was inserted before 2, so 3 is reached through 1
    F = np.zeros((4, 4))
    F[0, 1] = F[0, 2] = F[1, 3] = F[2, 3] = 1.0
    path, flux = npp.top_path([0], [3], F)
    assert list(path) == [0, 1, 3] and flux == 1.0
    # sources in the order given: from 2 first
    F = np.zeros((4, 4))
    F[2, 3] = F[1, 3] = 1.0
    assert list(npp.top_path([2, 1], [3], F)[0]) == [2, 3]
    assert list(npp.top_path([1, 2, 1], [3], F)[0]) == [1, 3]


# ---- arguments -----------------------------------------------------------------------------
@pytest.mark.parametrize("call", [
    lambda p: p.top_path(0, 2, np.zeros((3, 4))),
    lambda p: p.top_path(0, 2, np.zeros(3)),
    lambda p: p.top_path(0, 2, np.zeros((0, 0))),
    lambda p: p.top_path(0, 2, np.full((3, 3), np.nan)),
    lambda p: p.top_path(0, 2, np.array([[0, np.inf, 0], [0, 0, 1], [0, 0, 0]])),
    lambda p: p.top_path([], 2, F3),
    lambda p: p.top_path(0, [], F3),
    lambda p: p.top_path(0, 3, F3),
    lambda p: p.top_path(-1, 2, F3),
    lambda p: p.paths(0, 3, F3),
    lambda p: p.paths([0, 7], 2, F3, remove_path='bottleneck'),
    lambda p: p.paths(0, 2, np.zeros((2, 3))),
    lambda p: p.paths(0, 2, np.where(F3 > 0, -np.inf, 0.)),
    lambda p: p.paths(0, 2, scipy.sparse.csr_matrix(np.zeros((3, 4)))),
    lambda p: p.paths(0, 5, scipy.sparse.lil_matrix(F3)),
    lambda p: p.paths(0, 2, scipy.sparse.coo_matrix(np.nan * F3)),
    lambda p: p.paths(0, 2, np.zeros((3, 4)), remove_path=lambda F, path: F),
])
def test_argument_errors_raise_before_any_device_call(call):
    from enspara_amd.tpt import path
    before = _lib.live_resources().dev_allocs_total
    with pytest.raises(DataInvalid):
        call(path)
    assert _lib.live_resources().dev_allocs_total == before


def test_remove_path_must_be_known():
    from enspara_amd.tpt import path
    for bad in ("subtrac", "", None, 3):
        with pytest.raises(ValueError, match="subtract"):
            path.paths(0, 2, F3, remove_path=bad)
    # (before the matrix is looked at, as in the reference)
    with pytest.raises(ValueError):
        path.paths(0, 2, np.zeros((2, 3)), remove_path="no")


def test_c_abi_argument_errors():
    L = _lib.load()
    F = np.ascontiguousarray(F3)
    s, k = np.array([0], dtype=np.int32), np.array([2], dtype=np.int32)
    far = np.array([3], dtype=np.int32)
    indptr = np.array([0, 2, 3, 3], dtype=np.int64)
    cols = np.array([1, 2, 2], dtype=np.int32)
    vals = np.array([2., 1., 2.])
    h = ctypes.c_void_p()
    i32p, i64p, f64p = _lib.i32p, _lib.i64p, _lib.f64p
    before = tuple(_lib.live_resources())[:6]

    def open_(n=3, dense=f64p(F), csr=(None, None, None), src=s, snk=k, mode=1, caps=(0, 0),
              out=ctypes.byref(h)):
        return L.ek_tpt_paths_open(0, n, dense, csr[0], csr[1], csr[2], i32p(src), len(src),
                                   i32p(snk), len(snk), mode, 5, 1.0, 0.9, caps[0], caps[1],
                                   None, out)

    def err():
        return L.ek_last_error()

    assert open_(out=None) == _lib.EK_EARG
    assert open_(n=0) == _lib.EK_EARG and b"1 <= n <= 65535" in err()
    assert open_(n=65536) == _lib.EK_EARG
    assert open_(dense=None) == _lib.EK_EARG and b"either a dense matrix or CSR" in err()
    assert open_(csr=(i64p(indptr), i32p(cols), f64p(vals))) == _lib.EK_EARG
    assert b"either" in err()
    assert open_(src=far) == _lib.EK_EARG and b"sources" in err()
    assert open_(snk=far) == _lib.EK_EARG and b"sinks" in err()
    assert open_(src=s[:0]) == _lib.EK_EARG and b"sources" in err()
    assert open_(mode=3) == _lib.EK_EARG and b"mode 3" in err()
    assert open_(caps=(-1, 0)) == _lib.EK_EARG and b"batch" in err()
    assert open_(caps=(4097, 0)) == _lib.EK_EARG
    assert open_(caps=(0, -1)) == _lib.EK_EARG
    for bad_ptr in ([1, 2, 3, 3], [0, 2, 1, 3], [0, 2, 3, 2]):
        bp = np.array(bad_ptr, dtype=np.int64)
        assert open_(dense=None, csr=(i64p(bp), i32p(cols), f64p(vals))) == _lib.EK_EARG
        assert b"indptr" in err()
    for bad_cols in ([2, 1, 2], [1, 1, 2], [1, 3, 2], [-1, 2, 2]):
        bc = np.array(bad_cols, dtype=np.int32)
        assert open_(dense=None, csr=(i64p(indptr), i32p(bc), f64p(vals))) == _lib.EK_EARG
        assert b"not sorted inside [0, 3)" in err()
    assert open_(dense=None, csr=(i64p(indptr), None, f64p(vals))) == _lib.EK_EARG
    assert not h.value
    out = np.zeros(4, dtype=np.int32)
    fl = np.zeros(1)
    assert L.ek_tpt_paths_next(None, i32p(out), i32p(out), f64p(fl), i32p(out), i32p(out),
                               i32p(out)) == _lib.EK_EARG
    assert b"null handle" in err()
    assert L.ek_tpt_paths_stats(None, None, None) == _lib.EK_EARG
    assert L.ek_tpt_paths_close(None) == _lib.EK_OK
    assert tuple(_lib.live_resources())[:6] == before


def test_constants_are_those_of_the_kernels():
    from enspara_amd.tpt import path
    src = open(os.path.join(os.path.dirname(os.path.abspath(path.__file__)), os.pardir, "csrc",
                            "ek_tpt_path.hip")).read()
    for name, value in (("TPT_PATH_LDS_STATES", path.LDS_STATES),
                        ("TPT_PATH_STATE_BYTES", path.STATE_BYTES),
                        ("TPT_PATH_WG", path.SEARCH_WG), ("TPT_PATH_MAX_N", path.MAX_STATES)):
        assert re.findall(r"^#define %s (\d+)\b" % name, src, flags=re.M) == [str(value)], name
    # min_flux, key, previous, frontier, flags
    assert path.STATE_BYTES == 8 + 4 + 4 + 4 + 1
    # a workgroup may have 160 KiB; the reductions' scratch and control words need < 1 KiB,
    # and one more tile of 256 states would not fit
    lds = 160 * 1024
    assert path.LDS_STATES * path.STATE_BYTES + 1024 <= lds
    assert (path.LDS_STATES + 256) * path.STATE_BYTES > lds
    # the insertion key  step * n + state  fits 32 bits for step <= n
    assert path.MAX_STATES * path.MAX_STATES + path.MAX_STATES < 2 ** 32
