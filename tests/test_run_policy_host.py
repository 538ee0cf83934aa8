"""enspara_amd/csrc/ek_run_policy.h -- what the k-centers run loops decide between two
batches -- compiled for the host with g++ and driven through a small extern "C" shim.
The header includes nothing of HIP; the expected values below are literals worked out
from the constants the header documents (0.65 / +0.1 / 2..64 for the pick cap, 6.5 / 8.5 /
14 / 22 for the group's ladder, 0.8 T / 1.8 / 1.35 T' and 8..1024 for the single shard's,
2 % and 2..64 for the triangle masks, the active view's theta and 1..8, the batch caps).
"""
import ctypes as C
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "enspara_amd", "csrc")

SHIM = r'''
#include <new>
#include "ek_run_policy.h"
extern "C" {
int cap_size() { return (int)sizeof(EkPickCap); }
void cap_init(void *m, int option) { new (m) EkPickCap(option); }
// out: cap, probing, batches left to wait, the next wait
void cap_update(void *m, int T, int got, int ran, int room, int *out)
{
    EkPickCap *p = (EkPickCap *)m;
    p->update(T, got, ran, room);
    out[0] = p->cap; out[1] = p->probing; out[2] = p->wait.left; out[3] = p->wait.next;
}

int grp_size() { return (int)sizeof(EkGroupLadder); }
void grp_init(void *m, int on, int Tmax, int small_shards)
{
    new (m) EkGroupLadder(on != 0, Tmax, small_shards != 0);
}
// out: the form wanted, wait16, its next, wait32, its next, the first form
void grp_update(void *m, int T, double per_round, int ran, int *out)
{
    EkGroupLadder *p = (EkGroupLadder *)m;
    out[0] = p->update(T, per_round, ran);
    out[1] = p->wait16.left; out[2] = p->wait16.next;
    out[3] = p->wait32.left; out[4] = p->wait32.next;
    out[5] = p->first();
}

int lad_size() { return (int)sizeof(EkFormLadder); }
void lad_init(void *m, int adaptive, int tri, int Tmax)
{
    new (m) EkFormLadder(adaptive != 0, tri != 0, Tmax);
}
// another ladder, at home on entry `home` (no run builds one with both neighbours eligible)
void lad_set(void *m, int l0, int l1, int l2, int home)
{
    EkFormLadder *p = (EkFormLadder *)m;
    p->ladder[0] = l0; p->ladder[1] = l1; p->ladder[2] = l2;
    p->n = 3; p->home = home; p->form = p->ladder[home];
}
// out: entries, form, home's form, probing, gap, since, up_ok, down_ok, due(1000)
void lad_get(void *m, double per_round, int *out)
{
    EkFormLadder *p = (EkFormLadder *)m;
    out[0] = p->n; out[1] = p->form; out[2] = p->ladder[p->home]; out[3] = p->probing;
    out[4] = p->gap; out[5] = p->since; out[6] = p->up_ok(per_round);
    out[7] = p->down_ok(per_round); out[8] = p->due(1000);
}
void lad_update(void *m, int got, double ms, double per_round)
{
    ((EkFormLadder *)m)->update(got, ms, per_round);
}
double lad_rate_home(void *m) { return ((EkFormLadder *)m)->rate_home; }

int tri_size() { return (int)sizeof(EkTriPause); }
void tri_init(void *m) { new (m) EkTriPause(); }
// out: paused, batches left, the next pause
void tri_look(void *m, unsigned long long looked, unsigned long long left_out, int *out)
{
    EkTriPause *p = (EkTriPause *)m;
    const unsigned long long now[2] = {looked, left_out};
    p->look(now);
    out[0] = p->paused(); out[1] = p->wait.left; out[2] = p->wait.next;
}
void tri_skipped(void *m, int *out)
{
    EkTriPause *p = (EkTriPause *)m;
    p->skipped();
    out[0] = p->paused(); out[1] = p->wait.left; out[2] = p->wait.next;
}

int view_size() { return (int)sizeof(EkViewPolicy); }
void view_init(void *m) { new (m) EkViewPolicy(); }
// iout: est, build, pause left, next pause; dout: theta, guard
void view_decide(void *m, float last_max, double rho, double shrink, unsigned c0,
                 unsigned c1, long long view_n, long long n, int left, double per_round,
                 int forced, long long *iout, double *dout)
{
    EkViewPolicy *p = (EkViewPolicy *)m;
    const uint32_t cnt[2] = {c0, c1};
    const EkViewPlan v = p->decide(last_max, rho, shrink, cnt, view_n, n, left, per_round,
                                   forced != 0);
    iout[0] = v.est; iout[1] = v.build; iout[2] = p->pause.left; iout[3] = p->pause.next;
    dout[0] = (double)v.theta; dout[1] = v.guard;
}
void view_consts(double *out)
{
    out[0] = EK_VIEW_IDLE; out[1] = EK_VIEW_PAUSE_MAX; out[2] = EK_VIEW_PAUSED_BATCH;
    out[3] = EK_VIEW_REL; out[4] = EK_VIEW_ABS; out[5] = EK_VIEW_BATCH;
    out[6] = EK_VIEW_MIN_ROUNDS; out[7] = EK_MS_BATCH8;
}

int batch_single(int form, int left, int due, double per_round, int probing, int forced,
                 int view)
{
    return ek_batch_single(form, left, due, per_round, probing != 0, forced != 0, view);
}
int batch_group(int T, int left, double per_round, int ladder)
{
    return ek_batch_group(T, left, per_round, ladder != 0);
}
double per_round_guess(int T) { return ek_per_round_guess(T); }
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("run_policy_host")
    (d / "shim.cpp").write_text(SHIM)
    # the header alone, as a translation unit of its own: nothing of HIP behind it
    (d / "alone.cpp").write_text('#include "ek_run_policy.h"\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", CSRC,
                           str(d / "alone.cpp")])
    so = str(d / "run_policy_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC,
                           str(d / "shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.lad_rate_home.restype = C.c_double
    lib.per_round_guess.restype = C.c_double
    lib.lad_update.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double]
    lib.lad_get.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
    lib.grp_update.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p]
    lib.tri_look.argtypes = [C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_void_p]
    lib.view_decide.argtypes = [C.c_void_p, C.c_float, C.c_double, C.c_double, C.c_uint,
                                C.c_uint, C.c_longlong, C.c_longlong, C.c_int, C.c_double,
                                C.c_int, C.c_void_p, C.c_void_p]
    lib.batch_single.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int,
                                 C.c_int]
    lib.batch_group.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int]
    return lib


def _new(lib, what, *args):
    mem = C.create_string_buffer(getattr(lib, what + "_size")())
    getattr(lib, what + "_init")(mem, *args)
    return mem


# ---- pick cap ------------------------------------------------------------------------
def _cap(lib, mem, T, got, ran, room):
    out = (C.c_int * 4)()
    lib.cap_update(mem, T, got, ran, room, out)
    return list(out)       # cap, probing, wait, next wait


def test_pick_cap_probe_kept_or_lost(lib):
    m = _new(lib, "cap", 0)
    # yield 80 / (10 x 16) = 0.50 at form 16, 1000 centers to go: the other value, on trial
    assert _cap(lib, m, 16, 80, 10, 1000) == [16, 1, 0, 2]
    # 976 / 1600 = 0.61 > 0.50 + 0.1: it stays
    assert _cap(lib, m, 16, 976, 100, 1000) == [16, 0, 0, 2]

    m = _new(lib, "cap", 0)
    assert _cap(lib, m, 16, 80, 10, 1000) == [16, 1, 0, 2]
    # 944 / 1600 = 0.59: back to 4, two batches of waiting, then four
    assert _cap(lib, m, 16, 944, 100, 1000) == [4, 0, 2, 4]
    assert _cap(lib, m, 16, 80, 10, 1000) == [4, 0, 1, 4]      # (waiting: no probe)
    assert _cap(lib, m, 16, 80, 10, 1000) == [4, 0, 0, 4]
    assert _cap(lib, m, 16, 80, 10, 1000) == [16, 1, 0, 4]
    assert _cap(lib, m, 16, 80, 10, 1000) == [4, 0, 4, 8]      # the second loss waits 4


def test_pick_cap_wait_never_exceeds_64(lib):
    m = _new(lib, "cap", 0)
    waits = []
    for _ in range(9):
        while True:
            cap, probing, wait, nxt = _cap(lib, m, 8, 40, 10, 1000)    # yield 0.50
            if probing:
                break
        cap, probing, wait, nxt = _cap(lib, m, 8, 40, 10, 1000)        # no better: lost
        assert (cap, probing) == (4, 0)
        waits.append(wait)
    assert waits == [2, 4, 8, 16, 32, 64, 64, 64, 64]


def test_pick_cap_needs_room_a_low_yield_and_rounds_that_ran(lib):
    m = _new(lib, "cap", 0)
    assert _cap(lib, m, 16, 80, 10, 64) == [4, 0, 0, 2]        # room = 4 x form: no probe
    assert _cap(lib, m, 16, 104, 10, 1000) == [4, 0, 0, 2]     # yield 0.65: no probe
    assert _cap(lib, m, 16, 0, 0, 1000) == [4, 0, 0, 2]        # nothing ran
    assert _cap(lib, m, 16, 80, 10, 65) == [16, 1, 0, 2]
    # the form changed under the probe: not comparable, back
    assert _cap(lib, m, 8, 80, 10, 1000) == [4, 0, 2, 4]


@pytest.mark.parametrize("pinned", [4, 8, 16])
def test_pick_cap_set_by_option_never_moves(lib, pinned):
    m = _new(lib, "cap", pinned)
    for got in (80, 16, 160, 80):
        assert _cap(lib, m, 16, got, 10, 1000) == [pinned, 0, 0, 2]


# ---- the group's ladder ----------------------------------------------------------------
def _grp(lib, mem, T, per_round, ran=5):
    out = (C.c_int * 6)()
    lib.grp_update(mem, T, per_round, ran, out)
    return list(out)       # want, wait16, its next, wait32, its next, first form


def test_group_ladder_8_to_16(lib):
    m = _new(lib, "grp", 1, 16, 0)
    assert _grp(lib, m, 8, 6.4) == [8, 0, 1, 0, 1, 8]
    assert _grp(lib, m, 8, 6.5)[0] == 16
    m = _new(lib, "grp", 1, 16, 1)         # small shards
    assert _grp(lib, m, 8, 4.4)[0] == 8
    assert _grp(lib, m, 8, 4.5)[0] == 16
    assert _grp(lib, m, 16, 5.4)[0] == 8
    assert _grp(lib, m, 16, 5.5)[0] == 16


def test_group_ladder_16_back_to_8_waits_longer_each_time(lib):
    m = _new(lib, "grp", 1, 16, 0)
    assert _grp(lib, m, 16, 8.4) == [8, 1, 2, 0, 1, 8]
    assert _grp(lib, m, 8, 7.0) == [8, 0, 2, 0, 1, 8]          # the wait: one batch
    assert _grp(lib, m, 8, 7.0)[0] == 16
    assert _grp(lib, m, 16, 8.4) == [8, 2, 4, 0, 1, 8]
    # a batch of 16 that holds resets the next wait
    m = _new(lib, "grp", 1, 16, 0)
    assert _grp(lib, m, 16, 8.4)[:3] == [8, 1, 2]
    assert _grp(lib, m, 8, 7.0)[0] == 8
    assert _grp(lib, m, 8, 7.0)[0] == 16
    assert _grp(lib, m, 16, 8.5)[:3] == [16, 0, 1]
    # ... and the waits stop doubling at 64
    m = _new(lib, "grp", 1, 16, 0)
    assert [_grp(lib, m, 16, 1.0)[1] for _ in range(9)] == [1, 2, 4, 8, 16, 32, 64, 64, 64]


def test_group_ladder_32(lib):
    m = _new(lib, "grp", 1, 32, 0)
    assert _grp(lib, m, 16, 13.9)[0] == 16
    assert _grp(lib, m, 16, 14.0)[0] == 32
    assert _grp(lib, m, 32, 22.0) == [32, 0, 1, 0, 1, 8]
    assert _grp(lib, m, 32, 21.9) == [16, 0, 1, 1, 2, 8]
    assert _grp(lib, m, 16, 15.0) == [16, 0, 1, 0, 2, 8]       # wait32: one batch
    assert _grp(lib, m, 16, 15.0)[0] == 32
    assert _grp(lib, m, 32, 21.9) == [16, 0, 1, 2, 4, 8]
    m = _new(lib, "grp", 1, 16, 0)         # no rounds of 32 in this group
    assert _grp(lib, m, 16, 14.0)[0] == 16


def test_group_ladder_batch_without_rounds_changes_nothing(lib):
    m = _new(lib, "grp", 1, 32, 0)
    _grp(lib, m, 16, 8.4)
    _grp(lib, m, 32, 21.9)
    before = _grp(lib, m, 16, 1.0, ran=0)
    assert before == [16, 1, 2, 1, 2, 8]
    assert _grp(lib, m, 8, 20.0, ran=0) == [8] + before[1:]
    assert _grp(lib, m, 32, 1.0, ran=0) == [32] + before[1:]
    # a group whose form is pinned stays where it is
    m = _new(lib, "grp", 0, 16, 0)
    assert _grp(lib, m, 16, 1.0) == [16, 0, 1, 0, 1, 16]


# ---- the single shard's ladder -----------------------------------------------------------
def _lad(lib, mem, per_round=0.0):
    out = (C.c_int * 9)()
    lib.lad_get(mem, per_round, out)
    return dict(zip(("n", "form", "home", "probing", "gap", "since", "up_ok", "down_ok",
                     "due"), out))


def test_ladder_probe_loses_then_wins(lib):
    m = _new(lib, "lad", 1, 0, 16)
    s = _lad(lib, m)
    assert (s["n"], s["form"], s["home"], s["gap"], s["due"]) == (3, 1, 1, 8, 8)
    lib.lad_update(m, 8, 1.0, 1.0)         # 8 centers per ms at home; 8 since: look up
    s = _lad(lib, m)
    assert (s["form"], s["home"], s["probing"]) == (8, 1, 1)
    lib.lad_update(m, 3, 1.0, 3.0)         # the probe: 3 per ms -- back, the gap doubles
    s = _lad(lib, m)
    assert (s["form"], s["home"], s["probing"], s["gap"], s["since"]) == (1, 1, 0, 16, 0)
    lib.lad_update(m, 8, 1.0, 1.0)
    s = _lad(lib, m)
    assert (s["probing"], s["since"], s["due"]) == (0, 8, 8)  # 8 of 16: not yet
    lib.lad_update(m, 8, 0.5, 1.0)
    assert _lad(lib, m)["probing"] == 1 and lib.lad_rate_home(m) == 16.0
    lib.lad_update(m, 24, 1.0, 8.0)        # 24 per ms against 16: rounds of 8 are home
    s = _lad(lib, m)
    assert (s["form"], s["home"], s["probing"], s["gap"], s["since"]) == (8, 8, 0, 8, 0)
    assert lib.lad_rate_home(m) == 24.0


def test_ladder_gap_doubles_up_to_1024(lib):
    m = _new(lib, "lad", 1, 0, 16)
    gaps = []
    for _ in range(9):
        lib.lad_update(m, _lad(lib, m)["gap"], 1.0, 1.0)
        assert _lad(lib, m)["probing"] == 1
        lib.lad_update(m, 0, 1.0, 1.0)
        gaps.append(_lad(lib, m)["gap"])
    assert gaps == [16, 32, 64, 128, 256, 512, 1024, 1024, 1024]


def test_ladder_neighbours(lib):
    m = _new(lib, "lad", 1, 0, 16)
    assert _lad(lib, m, 0.1)["up_ok"] == 1         # from one-center steps: always up
    assert _lad(lib, m, 0.1)["down_ok"] == 0
    lib.lad_set(m, 1, 8, 16, 1)
    assert _lad(lib, m, 0.79 * 8)["up_ok"] == 0
    assert _lad(lib, m, 6.4)["up_ok"] == 1
    assert _lad(lib, m, 1.8)["down_ok"] == 0
    assert _lad(lib, m, 1.79)["down_ok"] == 1
    lib.lad_set(m, 1, 8, 16, 2)
    assert _lad(lib, m, 16.0)["up_ok"] == 0        # nothing wider
    assert _lad(lib, m, 10.7)["down_ok"] == 1      # under 1.35 x 8
    assert _lad(lib, m, 10.8)["down_ok"] == 0
    # neither neighbour worth a look: the count starts again
    lib.lad_set(m, 1, 8, 16, 1)
    lib.lad_update(m, 8, 1.0, 4.0)
    s = _lad(lib, m)
    assert (s["form"], s["probing"], s["since"]) == (8, 0, 0)


def test_ladder_direction_alternates(lib):
    """On 1 / 8 / 16 no form has both neighbours eligible (up from 8 needs 6.4 per round,
    down to 1 under 1.8), so the rule is driven on a ladder 6 / 8 / 16: at 7 per round
    both are (7 >= 0.8 x 8, 7 < 1.35 x 6)."""
    m = _new(lib, "lad", 1, 0, 16)
    lib.lad_set(m, 6, 8, 16, 1)
    s = _lad(lib, m, 7.0)
    assert (s["up_ok"], s["down_ok"]) == (1, 1)
    seen = []
    for _ in range(4):
        lib.lad_update(m, _lad(lib, m)["gap"], 1.0, 7.0)
        s = _lad(lib, m)
        assert s["probing"] == 1
        seen.append(s["form"])
        lib.lad_update(m, 0, 1.0, 7.0)
        assert _lad(lib, m)["form"] == 8
    assert seen == [16, 6, 16, 6]


def test_ladder_of_a_pinned_form(lib):
    m = _new(lib, "lad", 0, 0, 16)
    for _ in range(5):
        lib.lad_update(m, 100, 1.0, 16.0)
        s = _lad(lib, m, 16.0)
        assert (s["n"], s["form"], s["probing"], s["due"]) == (1, 16, 0, 1000)
    m = _new(lib, "lad", 0, 1, 1)          # triangle inequality, one center per pass
    s = _lad(lib, m)
    assert (s["n"], s["form"]) == (1, 1)
    m = _new(lib, "lad", 1, 0, 8)          # the ladder of a narrow context: 1 / 8
    assert (_lad(lib, m)["n"], _lad(lib, m)["form"]) == (2, 1)


# ---- pause of the triangle masks -----------------------------------------------------------
def test_triangle_pause(lib):
    out = (C.c_int * 3)()
    m = _new(lib, "tri")
    lib.tri_look(m, 1000, 19, out)         # 1.9 % left out
    assert list(out) == [1, 2, 4]
    lib.tri_skipped(m, out)
    lib.tri_skipped(m, out)
    assert list(out) == [0, 0, 4]
    lib.tri_look(m, 2000, 38, out)         # (the counters run on: 1000 and 19 again)
    assert list(out) == [1, 4, 8]
    for _ in range(4):
        lib.tri_skipped(m, out)
    lib.tri_look(m, 3000, 58, out)         # 20 of 1000: the masks stay, the next pause is 2
    assert list(out) == [0, 0, 2]
    m = _new(lib, "tri")
    lib.tri_look(m, 1000, 20, out)
    assert list(out) == [0, 0, 2]
    lib.tri_look(m, 1000, 20, out)         # nothing looked at: no pause either
    assert list(out) == [0, 0, 2]
    m = _new(lib, "tri")
    pauses = []
    for k in range(1, 9):
        lib.tri_look(m, 1000 * k, 0, out)
        pauses.append(out[1])
    assert pauses == [2, 4, 8, 16, 32, 64, 64, 64]


# ---- the active view -----------------------------------------------------------------------
def _view(lib, m, last_max, cnt, view_n, n, left, per_round, forced=0, rho=0.75,
          shrink=0.8):
    io = (C.c_longlong * 4)()
    do = (C.c_double * 2)()
    lib.view_decide(m, last_max, rho, shrink, cnt[0], cnt[1], view_n, n, left, per_round,
                    forced, io, do)
    return dict(est=io[0], build=io[1], pause=io[2], next=io[3], theta=do[0], guard=do[1])


def test_view_constants(lib):
    out = (C.c_double * 8)()
    lib.view_consts(out)
    assert list(out) == [0.95, 8, 64, 1e-3, 1e-3, 16, 24, 12]


def test_view_theta_and_guard(lib):
    m = _new(lib, "view")
    # (0.75 x 2 - 0.001) / 2.002 = 0.74875124875...: the float below it
    v = _view(lib, m, 2.0, (500, 0), 0, 1000, 1000, 10.0)
    assert v["theta"] == float.fromhex("0x1.7f5c52p-1") == 0.7487512230873108
    assert v["guard"] == pytest.approx(1.499999948620796, rel=1e-14)
    # (0.75 x 0.5 - 0.001) / 2.002 = 0.186813186813...: the nearest float lies above it
    # (0x1.7e97eap-3 = 0.18681319057...), the answer is the one before
    v = _view(lib, m, 0.5, (500, 0), 0, 1000, 1000, 10.0)
    assert v["theta"] == float.fromhex("0x1.7e97e8p-3") == 0.18681317567825317
    assert v["guard"] == pytest.approx(0.3749999777078628, rel=1e-14)
    assert v["guard"] <= 0.75 * 0.5
    # a maximum so small that nothing is settled: no decision, the pauses untouched
    v = _view(lib, m, 0.001, (1000, 0), 0, 1000, 1000, 10.0)
    assert (v["theta"] <= 0.0, v["est"], v["build"], v["pause"], v["next"]) == \
        (True, 0, 0, 0, 1)


def test_view_estimate_and_build(lib):
    m = _new(lib, "view")
    assert _view(lib, m, 2.0, (500, 900), 0, 1000, 1000, 10.0)["est"] == 500
    assert _view(lib, m, 2.0, (500, 900), 600, 1000, 1000, 10.0)["est"] == 800
    assert _view(lib, m, 2.0, (500, 400), 600, 1000, 1000, 10.0)["est"] == 500
    # at most 0.8 x the frames streamed, and 24 rounds' worth of centers left
    assert _view(lib, m, 2.0, (800, 0), 0, 1000, 240, 10.0)["build"] == 1
    assert _view(lib, m, 2.0, (801, 0), 0, 1000, 240, 10.0)["build"] == 0
    assert _view(lib, m, 2.0, (800, 0), 0, 1000, 239, 10.0)["build"] == 0
    assert _view(lib, m, 2.0, (800, 0), 0, 1000, 24, 0.5)["build"] == 1    # (>= 1 per round)
    assert _view(lib, m, 2.0, (800, 0), 0, 1000, 23, 0.5)["build"] == 0
    # under a view: against the view's frames
    assert _view(lib, m, 2.0, (480, 0), 600, 1000, 1000, 10.0)["build"] == 1
    assert _view(lib, m, 2.0, (481, 0), 600, 1000, 1000, 10.0)["build"] == 0
    # forced: whenever a frame can be left out
    assert _view(lib, m, 2.0, (999, 0), 0, 1000, 1, 10.0, forced=1)["build"] == 1
    assert _view(lib, m, 2.0, (1000, 0), 0, 1000, 1000, 10.0, forced=1)["build"] == 0


def test_view_pauses(lib):
    m = _new(lib, "view")
    idle = [_view(lib, m, 2.0, (951, 0), 0, 1000, 1000, 10.0) for _ in range(5)]
    assert [v["pause"] for v in idle] == [1, 2, 4, 8, 8]
    assert [v["build"] for v in idle] == [0] * 5
    v = _view(lib, m, 2.0, (900, 0), 0, 1000, 1000, 10.0)  # between the two shares: as it was
    assert (v["pause"], v["next"]) == (8, 8)
    v = _view(lib, m, 2.0, (500, 0), 0, 1000, 1000, 10.0)  # a build
    assert (v["build"], v["next"]) == (1, 1)
    assert _view(lib, m, 2.0, (951, 0), 0, 1000, 1000, 10.0)["pause"] == 1
    assert _view(lib, m, 2.0, (950, 0), 0, 1000, 1000, 10.0)["next"] == 2  # 0.95: not above
    # forced views never pause
    m = _new(lib, "view")
    v = _view(lib, m, 2.0, (1000, 0), 0, 1000, 1000, 10.0, forced=1)
    assert (v["pause"], v["next"]) == (0, 1)


# ---- batch lengths -------------------------------------------------------------------------
def test_batch_single(lib):
    b = lib.batch_single     # form, left, due, per_round, probing, forced, view
    # one-center steps: never past the goal
    assert b(1, 3, 100, 0.6, 0, 0, 0) == 3
    assert b(1, 1000, 1000, 0.6, 0, 0, 0) == 256
    assert b(1, 1000, 50, 0.6, 0, 0, 1) == 50      # (the view's cap is for rounds)
    assert b(1, 10, 8, 0.6, 1, 0, 0) == 4
    assert b(1, 2, 8, 0.6, 1, 0, 0) == 2
    assert b(1, 100, 100, 0.6, 0, 1, 0) == 2
    assert b(1, 1, 100, 0.6, 0, 1, 0) == 1
    # rounds
    assert b(16, 1000, 1000, 10.0, 0, 0, 0) == 101
    assert b(16, 1000, 1000, 10.0, 0, 0, 1) == 16
    assert b(16, 1000, 1000, 10.0, 0, 0, 2) == 64
    assert b(16, 1000, 1000, 10.0, 1, 0, 1) == 3
    assert b(16, 1000, 1000, 10.0, 0, 1, 1) == 2
    assert b(16, 5000, 5000, 1.0, 0, 0, 0) == 256
    assert b(16, 5, 5, 16.0, 0, 0, 0) == 2
    assert b(8, 1000, 8, 4.0, 0, 0, 0) == 3        # back when another form is due
    assert b(8, 30, 30, 4.0, 0, 0, 2) == 8


def test_batch_group(lib):
    b = lib.batch_group      # T, left, per_round, ladder
    assert b(16, 1000, 5.0, 0) == 202
    assert b(8, 1000, 5.0, 1) == 12
    assert b(16, 1000, 5.0, 1) == 64
    assert b(32, 1000, 5.0, 1) == 48
    assert b(8, 20, 4.0, 1) == 7
    assert b(16, 10000, 1.0, 0) == 256
    assert b(16, 3, 8.0, 1) == 2
    assert lib.per_round_guess(16) == pytest.approx(9.6, rel=1e-15)
    assert lib.per_round_guess(1) == pytest.approx(0.6, rel=1e-15)
