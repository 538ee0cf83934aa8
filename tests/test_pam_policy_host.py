"""enspara_amd/csrc/ek_pam_policy.h -- what the PAM window path decides between two
launches -- compiled for the host with g++ and driven through a small extern "C" shim.
The header includes nothing of HIP; the expected values below are literals worked out
from the constants the header documents (16384 frames, a quarter of them, pauses of 15
and 32 windows for the prefetch; waits of 8..256 windows, counted down before they are
read, for the one-workgroup window; 65536 listed frames, 1024 chunks of 64 leaves; windows
of 32).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "enspara_amd", "csrc")

SHIM = r'''
#include <new>
#include "ek_pam_policy.h"
extern "C" {
void limits(int *out)
{
    out[0] = EK_PAM_WIN; out[1] = EK_PAM_GROUP; out[2] = EK_PW_FULL_LEAVES;
    out[3] = EK_SP_CAP; out[4] = EK_SP_MAX_PAIRS; out[5] = EK_SP_MAX_CHUNKS;
    out[6] = (int)EK_PF_MIN_FRAMES;
}
int prune_ok(int prune, int exact, int A) { return ek_pam_prune_ok(prune, exact, A); }
int pf_short(long long n_act, long long n) { return ek_pf_short(n_act, n); }

int form_size() { return (int)sizeof(EkPrefetchForm); }
void form_init(void *m) { new (m) EkPrefetchForm(); }
int form_try(void *m, int prune, int exact, int A, int win_count, long long n)
{
    return ((EkPrefetchForm *)m)->try_restricted(prune, exact, A, win_count, n);
}
int form_use_bounds(void *m, int possible)
{
    return ((EkPrefetchForm *)m)->use_bounds(possible != 0);
}
int form_retry_exact(void *m, int bounds, long long n_act, long long n)
{
    return ((EkPrefetchForm *)m)->retry_exact(bounds != 0, n_act, n);
}
void form_too_many(void *m) { ((EkPrefetchForm *)m)->too_many(); }
void form_begin(void *m) { ((EkPrefetchForm *)m)->begin(); }
// out: windows of the pause to go, windows to go with exact tables
void form_get(void *m, int *out)
{
    EkPrefetchForm *p = (EkPrefetchForm *)m;
    out[0] = p->pause.left; out[1] = p->exact_left;
}

int vecs_size() { return (int)sizeof(EkVecs); }
void vecs_init(void *m) { new (m) EkVecs(); }
void vecs_whole(void *m) { ((EkVecs *)m)->whole(); }
void vecs_listed(void *m, long long n_act, int count, int after_sparse_reset)
{
    ((EkVecs *)m)->listed(n_act, count, after_sparse_reset != 0);
}
int vecs_finished(void *m, int reset_there, int stop, int count)
{
    return ((EkVecs *)m)->finished(reset_there != 0, stop, count);
}
int vecs_sparse_reset(void *m, int count) { return ((EkVecs *)m)->sparse_reset(count); }
int vecs_reset_there(void *m, int finish_later, long long n_act, int count)
{
    return ((EkVecs *)m)->reset_there(finish_later != 0, n_act, count);
}
void vecs_get(void *m, long long *out)
{
    out[0] = ((EkVecs *)m)->rows; out[1] = ((EkVecs *)m)->cols;
}

int spw_size() { return (int)sizeof(EkSpWait); }
void spw_init(void *m) { new (m) EkSpWait(); }
int spw_over(void *m, long long max_pairs) { return ((EkSpWait *)m)->over(max_pairs); }
void spw_handed_back(void *m) { ((EkSpWait *)m)->handed_back(); }
void spw_clean(void *m) { ((EkSpWait *)m)->clean(); }
void spw_begin(void *m) { ((EkSpWait *)m)->begin(); }
void spw_get(void *m, int *out)
{
    out[0] = ((EkSpWait *)m)->wait.left; out[1] = ((EkSpWait *)m)->wait.next;
}

int sp_list_ok(int slots, long long n_act) { return ek_sp_list_ok(slots != 0, n_act); }
int tables_cover(int lo, int n, int cid0, int count)
{
    return ek_pam_tables_cover(lo, n, cid0, count);
}
int sp_eligible(int option, int list_ready, int tables, int prune, int frame_major,
                int chunks, int leaves, int wait_over, int columns)
{
    return ek_sp_eligible(option != 0, list_ready != 0, tables != 0, prune != 0,
                          frame_major != 0, chunks, leaves, wait_over != 0, columns != 0);
}

// out: hi, cnt, the counts that ride along
void sweep_win(int cid, int K, int width, int n_slots, int *out)
{
    const EkSweepWin w(cid, K, width);
    out[0] = w.hi; out[1] = w.cnt; out[2] = w.ride_along(n_slots, K, width);
}
int counts_stand(int ncnt, int n_done, int n_slots)
{
    return ek_sweep_counts_stand(ncnt, n_done, n_slots);
}
int draw_at(const uint32_t *raw, long long n_raw, long long *pos, long long m, long long *out)
{
    int64_t p = *pos, o = *out;
    const int r = ek_draw_at(raw, n_raw, &p, m, &o);
    *pos = p; *out = o;
    return r;
}
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("pam_policy_host")
    (d / "shim.cpp").write_text(SHIM)
    # the header alone, as a translation unit of its own: nothing of HIP behind it
    (d / "alone.cpp").write_text('#include "ek_pam_policy.h"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC,
                           str(d / "alone.cpp")])
    so = str(d / "pam_policy_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC,
                           str(d / "shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    ll = C.c_longlong
    lib.pf_short.argtypes = [ll, ll]
    lib.form_try.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, ll]
    lib.form_retry_exact.argtypes = [C.c_void_p, C.c_int, ll, ll]
    lib.vecs_listed.argtypes = [C.c_void_p, ll, C.c_int, C.c_int]
    lib.vecs_reset_there.argtypes = [C.c_void_p, C.c_int, ll, C.c_int]
    lib.spw_over.argtypes = [C.c_void_p, ll]
    lib.sp_list_ok.argtypes = [C.c_int, ll]
    lib.draw_at.argtypes = [C.c_void_p, ll, C.POINTER(ll), ll, C.POINTER(ll)]
    return lib


def _new(lib, what):
    mem = C.create_string_buffer(getattr(lib, what + "_size")())
    getattr(lib, what + "_init")(mem)
    return mem


def _ints(fn, mem, n):
    out = (C.c_int * n)()
    fn(mem, out)
    return list(out)


def test_limits(lib):
    out = (C.c_int * 7)()
    lib.limits(out)
    assert list(out) == [32, 8, 64, 65536, 16384, 1024, 16384]


# ---- the prefetch form ------------------------------------------------------------------
def _try(lib, m, prune=1, exact=1, A=3, win_count=1, n=16384):
    return lib.form_try(m, prune, exact, A, win_count, n)


def test_restricted_gate_on_both_sides_of_each_clause(lib):
    m = _new(lib, "form")
    assert _try(lib, m) == 1
    assert _try(lib, m, n=16383) == 0
    assert _try(lib, m, A=2) == 0
    assert _try(lib, m, win_count=0) == 0
    assert _try(lib, m, prune=0) == 0
    assert _try(lib, m, exact=0) == 0
    assert _try(lib, m, A=1000, win_count=32, n=10 ** 7) == 1
    assert _ints(lib.form_get, m, 2) == [0, 0]     # (no gate moves a pause)
    assert lib.prune_ok(1, 1, 3) == 1
    assert (lib.prune_ok(0, 1, 3), lib.prune_ok(1, 0, 3), lib.prune_ok(1, 1, 2)) == (0, 0, 0)


def test_short_list_is_a_quarter_of_the_frames(lib):
    assert lib.pf_short(4096, 16384) == 1
    assert lib.pf_short(4097, 16384) == 0
    assert lib.pf_short(0, 16384) == 1
    # the retry with exact tables: the same boundary, and only for a list made from bounds
    m = _new(lib, "form")
    assert lib.form_retry_exact(m, 1, 4096, 16384) == 0
    assert lib.form_retry_exact(m, 0, 4097, 16384) == 0
    assert _ints(lib.form_get, m, 2) == [0, 0]
    assert lib.form_retry_exact(m, 1, 4097, 16384) == 1
    assert _ints(lib.form_get, m, 2) == [0, 32]


def test_pause_after_too_many_within_reach(lib):
    """15 windows skip the restricted form -- whatever their gate would say --, the 16th
    tries it."""
    m = _new(lib, "form")
    assert _try(lib, m) == 1
    lib.form_too_many(m)
    assert _ints(lib.form_get, m, 2) == [15, 0]
    assert [_try(lib, m) for _ in range(15)] == [0] * 15
    assert _ints(lib.form_get, m, 2) == [0, 0]
    assert _try(lib, m) == 1
    # the pause does not grow: 15 again
    for _ in range(3):
        lib.form_too_many(m)
        assert [_try(lib, m) for _ in range(16)] == [0] * 15 + [1]
    # a window the gate would refuse counts down too
    lib.form_too_many(m)
    assert [_try(lib, m, n=100) for _ in range(15)] == [0] * 15
    assert _try(lib, m) == 1
    # a sweep that begins ends the pause
    lib.form_too_many(m)
    assert _try(lib, m) == 0
    lib.form_begin(m)
    assert _try(lib, m) == 1


def test_exact_tables_after_loose_bounds(lib):
    """The next 32 windows that take the restricted form use exact tables; windows that
    do not reach it count nothing down."""
    m = _new(lib, "form")
    assert lib.form_use_bounds(m, 1) == 1
    assert lib.form_use_bounds(m, 0) == 0
    assert lib.form_retry_exact(m, 1, 5000, 16384) == 1
    # windows kept from the restricted form (the gate, the pause): exact_left stands
    lib.form_too_many(m)
    for _ in range(15):
        assert _try(lib, m) == 0
    assert _try(lib, m, n=100) == 0
    assert _ints(lib.form_get, m, 2) == [0, 32]
    got = []
    for _ in range(33):
        assert _try(lib, m) == 1
        got.append(lib.form_use_bounds(m, 1))
    assert got == [0] * 32 + [1]
    # read before it counts down; a window where bounds are not possible counts too
    assert lib.form_retry_exact(m, 1, 5000, 16384) == 1
    assert [lib.form_use_bounds(m, 0) for _ in range(31)] == [0] * 31
    assert _ints(lib.form_get, m, 2) == [0, 1]
    assert lib.form_use_bounds(m, 1) == 0
    assert lib.form_use_bounds(m, 1) == 1
    # a sweep that begins leaves it
    assert lib.form_retry_exact(m, 1, 5000, 16384) == 1
    lib.form_begin(m)
    assert _ints(lib.form_get, m, 2) == [0, 32]


# ---- the one-workgroup window's wait ------------------------------------------------------
def test_wait_after_a_hand_back_is_seven_windows(lib):
    m = _new(lib, "spw")
    assert [lib.spw_over(m, 16384) for _ in range(3)] == [1, 1, 1]
    lib.spw_handed_back(m)
    assert _ints(lib.spw_get, m, 2) == [8, 16]
    assert [lib.spw_over(m, 16384) for _ in range(8)] == [0] * 7 + [1]
    assert [lib.spw_over(m, 16384) for _ in range(3)] == [1, 1, 1]


def test_waits_double_up_to_256_and_a_clean_window_starts_over(lib):
    m = _new(lib, "spw")
    waits = []
    for _ in range(8):
        lib.spw_handed_back(m)
        waits.append(_ints(lib.spw_get, m, 2)[0])
        while not lib.spw_over(m, 16384):
            pass
    assert waits == [8, 16, 32, 64, 128, 256, 256, 256]
    # exactly: a wait of 16 keeps 15 windows out
    m = _new(lib, "spw")
    lib.spw_handed_back(m)
    assert [lib.spw_over(m, 1) for _ in range(8)] == [0] * 7 + [1]
    lib.spw_handed_back(m)
    assert [lib.spw_over(m, 1) for _ in range(16)] == [0] * 15 + [1]
    lib.spw_clean(m)                       # a clean window in between: 8 again
    assert _ints(lib.spw_get, m, 2) == [0, 8]
    lib.spw_handed_back(m)
    assert _ints(lib.spw_get, m, 2) == [8, 16]
    lib.spw_begin(m)                       # a sweep begins: at rest
    assert _ints(lib.spw_get, m, 2) == [0, 8]
    assert lib.spw_over(m, 16384) == 1


def test_max_pairs_zero_ignores_the_wait(lib):
    m = _new(lib, "spw")
    lib.spw_handed_back(m)
    assert [lib.spw_over(m, 0) for _ in range(10)] == [1] * 10
    # ... which goes by all the same: the eighth window was the first eligible one
    assert _ints(lib.spw_get, m, 2) == [0, 16]
    lib.spw_handed_back(m)
    assert [lib.spw_over(m, 0) for _ in range(5)] == [1] * 5
    assert [lib.spw_over(m, 16384) for _ in range(11)] == [0] * 10 + [1]


# ---- eligibility of the one-workgroup window ----------------------------------------------
def test_each_clause_alone_refuses_the_one_workgroup_window(lib):
    ok = dict(option=1, list_ready=1, tables=1, prune=1, frame_major=1, chunks=1024,
              leaves=65536, wait_over=1, columns=1)
    order = list(ok)
    assert lib.sp_eligible(*[ok[k] for k in order]) == 1
    for k, bad in (("option", 0), ("list_ready", 0), ("tables", 0), ("prune", 0),
                   ("frame_major", 0), ("chunks", 1025), ("leaves", 65537),
                   ("wait_over", 0), ("columns", 0)):
        assert lib.sp_eligible(*[bad if q == k else ok[q] for q in order]) == 0, k
    # the clauses' own boundaries
    assert (lib.sp_list_ok(1, 65536), lib.sp_list_ok(1, 65537), lib.sp_list_ok(0, 10)) == \
        (1, 0, 0)
    assert lib.tables_cover(64, 32, 64, 32) == 1
    assert lib.tables_cover(64, 32, 64, 8) == 1        # at least `count` slots
    assert lib.tables_cover(64, 8, 64, 9) == 0
    assert lib.tables_cover(64, 32, 65, 8) == 0        # made for another window
    assert lib.tables_cover(64, 0, 64, 1) == 0         # forgotten


# ---- the vectors' bookkeeping ---------------------------------------------------------------
def _vecs(lib, m):
    out = (C.c_longlong * 2)()
    lib.vecs_get(m, out)
    return list(out)


def test_vectors_bookkeeping(lib):
    m = _new(lib, "vecs")
    assert _vecs(lib, m) == [-1, 0]
    assert lib.vecs_sparse_reset(m, 1) == 0            # whole vectors: a fill
    assert lib.vecs_reset_there(m, 1, 0, 0) == 0
    # written at list[0 .. 300) of 32 columns, after a fill
    lib.vecs_listed(m, 300, 32, 0)
    assert _vecs(lib, m) == [300, 32]
    assert (lib.vecs_sparse_reset(m, 32), lib.vecs_sparse_reset(m, 8)) == (1, 1)
    assert lib.vecs_reset_there(m, 1, 300, 32) == 1
    assert lib.vecs_reset_there(m, 0, 300, 32) == 0    # no finish kernel behind the window
    assert lib.vecs_reset_there(m, 1, 299, 32) == 0    # another list
    assert lib.vecs_reset_there(m, 1, 300, 8) == 0     # columns that are no slots
    # a window of 8 after the sparse reset of all 32 columns: 32 columns stand
    lib.vecs_whole(m)
    assert lib.vecs_sparse_reset(m, 8) == 0
    lib.vecs_listed(m, 120, 8, 1)
    assert _vecs(lib, m) == [120, 32]
    assert lib.vecs_reset_there(m, 1, 120, 8) == 0
    assert lib.vecs_sparse_reset(m, 32) == 1
    # cols < count: 8 columns listed, 32 wanted -- a fill
    lib.vecs_whole(m)
    lib.vecs_listed(m, 120, 8, 0)
    assert _vecs(lib, m) == [120, 8]
    assert (lib.vecs_sparse_reset(m, 8), lib.vecs_sparse_reset(m, 9)) == (1, 0)
    # the finish kernel did the reset but the window stopped early: as before
    assert lib.vecs_finished(m, 1, 5, 8) == 0
    assert _vecs(lib, m) == [120, 8]
    assert lib.vecs_finished(m, 0, 8, 8) == 0          # it was not asked to
    assert _vecs(lib, m) == [120, 8]
    # ... and ran to its end: nothing written is left, any prefetch resets for free
    assert lib.vecs_finished(m, 1, 8, 8) == 1
    assert _vecs(lib, m) == [0, 8]
    assert (lib.vecs_sparse_reset(m, 8), lib.vecs_sparse_reset(m, 9)) == (1, 0)
    assert lib.vecs_reset_there(m, 1, 0, 8) == 1
    lib.vecs_whole(m)                                  # a pass over all frames
    assert _vecs(lib, m) == [-1, 8]
    assert lib.vecs_sparse_reset(m, 1) == 0


# ---- the sweep's arithmetic -----------------------------------------------------------------
def _win(lib, cid, K, width, n_slots):
    out = (C.c_int * 3)()
    lib.sweep_win(cid, K, width, n_slots, out)
    return list(out)       # hi, cnt, ride-along counts


def test_sweep_windows_and_ride_along_counts(lib):
    assert _win(lib, 0, 70, 32, 32) == [32, 32, 32]
    assert _win(lib, 32, 70, 32, 32) == [64, 32, 6]
    assert _win(lib, 64, 70, 32, 6) == [70, 6, 0]
    # a window opened where another stopped
    assert _win(lib, 5, 70, 32, 32) == [37, 32, 32]
    assert _win(lib, 39, 70, 32, 31) == [70, 31, 0]
    # the draws ended at an empty cluster: none ride along
    assert _win(lib, 0, 70, 32, 31) == [32, 32, 0]
    assert _win(lib, 0, 70, 32, 0) == [32, 32, 0]
    # they stand if there are any and the window ran to its end
    assert lib.counts_stand(32, 32, 32) == 1
    assert lib.counts_stand(32, 31, 32) == 0
    assert lib.counts_stand(0, 6, 6) == 0


@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("m", [1, 2, 3, 255, 256, 257, 2 ** 32])
def test_draws_are_numpys(lib, seed, m):
    n = 64
    raw = np.random.RandomState(seed).randint(0, 2 ** 32, size=4 * n + 64, dtype=np.uint32)
    ref = np.random.RandomState(seed)
    want = [int(ref.choice(m)) for _ in range(n)]

    def draws(n_raw):
        pos, out, got = C.c_longlong(0), C.c_longlong(-1), []
        while len(got) < n and \
                lib.draw_at(raw.ctypes.data, n_raw, C.byref(pos), m, C.byref(out)) == 0:
            got.append(out.value)
        return got, pos.value

    got, used = draws(len(raw))
    assert got == want
    # the RandomState is where `used` raw outputs would have left it
    check = np.random.RandomState(seed)
    if used:
        check.randint(0, 2 ** 32, size=used, dtype=np.uint32)
    assert int(check.randint(0, 10 ** 9)) == int(ref.randint(0, 10 ** 9))
    assert (used == 0) == (m == 1) and used >= (n if m > 1 else 0)
    if m in (2, 256, 2 ** 32):
        assert used == n            # a mask that rejects nothing
    if m > 1:
        # the outputs run out under the last draw: it is not made, nothing of it consumed
        got, pos = draws(used - 1)
        assert got == want[:n - 1]
        out, p = C.c_longlong(-7), C.c_longlong(pos)
        assert lib.draw_at(raw.ctypes.data, used - 1, C.byref(p), m, C.byref(out)) == 1
        assert (p.value, out.value) == (pos, -7)
        assert lib.draw_at(raw.ctypes.data, 0, C.byref(C.c_longlong(0)), m, C.byref(out)) == 1
