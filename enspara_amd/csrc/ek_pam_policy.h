// ek_pam_policy.h -- what the PAM window path decides between two launches, in plain
// C++17: no HIP, nothing of the context.  The steps of ek_api_pam.hip (the proposal
// prefetch, ek_pam_window_run, ek_pam_sweep) enqueue kernels, wait, and hand what came
// back to the structs below; every threshold lives here once.  The header builds for the
// host alone (tests/test_pam_policy_host.py drives it from a shim).
#pragma once
#include "ek_pam_limits.h"
#include "ek_run_policy.h"

// only when dist[f] is known to be the distance to medoid assign[f] (a state
// this library produced; not one uploaded by the caller) may the search skip
// medoids out of the members' reach
// (and not for 1- or 2-atom "structures": collinear points make the largest
// root of the QCP quartic a double root, the computed distances are then too
// erratic to be treated as a metric)
inline bool ek_pam_prune_ok(bool prune, bool state_exact, int A)
{
    return prune && state_exact && A >= 3;
}

// ---- the prefetch form ------------------------------------------------------------------
// The distance vectors of a window's proposals: exact only at the frames a proposal can
// touch (a list, ek_pam_active_kernel; +inf elsewhere), or a pass over all frames.
static constexpr int64_t EK_PF_MIN_FRAMES = 16384;  // below it the passes cost less than the list
// a short list: straight from the frame-major copy (a quarter of the frames costs
// about what the passes over all of them do)
inline bool ek_pf_short(int64_t n_act, int64_t n) { return n_act * 4 <= n; }

struct EkPrefetchForm {
    // too many frames within reach (large clusters): the test cost a table, a scan and
    // a read-back for nothing -- left out for a while.  A waiting window counts down and
    // is skipped, the one that brings the count to 0 included.
    EkWait pause{15, 15};
    // windows to go with exact tables: where the bounds are too loose -- few atoms,
    // clusters as wide as they are apart: more than a quarter of the frames "within
    // reach" -- the window's tables are made again exactly, and the next windows'
    // right away.  Read before it counts down, and only by windows that take the
    // restricted form.
    int exact_left = 0;

    // is the restricted form tried for this window?
    bool try_restricted(bool prune, bool state_exact, int A, int32_t win_count, int64_t n)
    {
        if (pause.tick())
            return false;
        return ek_pam_prune_ok(prune, state_exact, A) && win_count > 0 && n >= EK_PF_MIN_FRAMES;
    }
    // (in the restricted form) the proposal-to-medoid table only as the lower bounds the
    // old medoids' table gives?  `possible`: the window's slots and proposals coincide,
    // the proposals are members of their clusters, the option is on
    bool use_bounds(bool possible)
    {
        const bool bounds = possible && exact_left == 0;
        if (exact_left > 0)
            --exact_left;
        return bounds;
    }
    // the list made from bounds holds n_act frames: again with exact tables?
    bool retry_exact(bool bounds, int64_t n_act, int64_t n)
    {
        if (!bounds || ek_pf_short(n_act, n))
            return false;
        exact_left = 32;
        return true;
    }
    void too_many() { pause.lose(); }
    void begin() { pause.left = 0; }    // a sweep begins (exact_left stands)
};

// ---- the distance vectors' bookkeeping --------------------------------------------------
// rows >= 0: the vectors are +inf except at list[0 .. rows) of their first `cols`
// columns; rows = -1: whole vectors were written.
struct EkVecs {
    int64_t rows = -1;
    int32_t cols = 0;
    // a prefetch of `count` columns: can the vectors go back to +inf by the entries the
    // window before wrote (instead of filling them whole)?
    bool sparse_reset(int count) const { return rows >= 0 && cols >= count; }
    void whole() { rows = -1; }         // whole vectors are (about to be) written
    // written at list[0 .. n_act) only: of `count` columns after a fill, of the columns
    // there were after a sparse reset
    void listed(int64_t n_act, int count, bool after_sparse_reset)
    {
        rows = n_act;
        cols = after_sparse_reset ? cols : count;
    }
    // the one-workgroup window over that list: does the reset ride in its finish kernel?
    // (where every column written is one of the window's slots)
    bool reset_there(bool finish_later, int64_t n_act, int count) const
    {
        return finish_later && rows == n_act && cols == count;
    }
    // the window is through: the finish kernel has put the vectors back to +inf if it was
    // asked to and the window ran to its end -> nothing of them is a prefetched vector
    bool finished(bool reset_there, int32_t stop, int32_t count)
    {
        if (!reset_there || stop != count)
            return false;
        rows = 0;
        return true;
    }
};

// ---- the one-workgroup window (ek_pam_sparse.hip) -----------------------------------------
// the list of a restricted prefetch serves a window right away if the window's slots and
// the proposals coincide and one workgroup can hold it
inline bool ek_sp_list_ok(bool slots, int64_t n_act) { return slots && n_act <= EK_SP_CAP; }

// (a window that had to hand a proposal back -- more ambiguous members x
// medoids within reach than one workgroup should search -- cost a window's
// set-up for one slot: the next few go the three-launch way, twice as many
// each time it happens again)
// The count goes down FIRST and the window is eligible if it is 0 then: after a wait of
// 8 seven windows go the three-launch way, the eighth may be one workgroup's again.
struct EkSpWait {
    EkWait wait{8, 256};
    // a window is about to run: does the wait let it be one workgroup's?
    // max_pairs == 0 (every search handed back, on purpose) ignores the wait
    bool over(int64_t max_pairs)
    {
        if (wait.left > 0)
            --wait.left;
        return wait.left == 0 || max_pairs == 0;
    }
    void handed_back() { wait.lose(); }
    void clean() { wait.reset(); }
    void begin()
    {
        wait.left = 0;
        wait.reset();
    }
};

// May the window [cid0, +count) be worked through by one workgroup?  A clause each.
inline bool ek_sp_eligible(bool option,             // EK_OPT_PAM_ONE_WORKGROUP
                           bool list_ready,         // ek_sp_list_ok, and still in place
                           bool tables,             // made for cid0, at least `count` slots
                           bool prune,              // ek_pam_prune_ok
                           bool frame_major,        // the frame-major copy is there
                           int chunks, int leaves,  // of the cost sums: what LDS holds
                           bool wait_over,          // EkSpWait::over
                           bool columns)            // slot i's vector is column i
{
    return option && list_ready && tables && prune && frame_major &&
           chunks <= EK_SP_MAX_CHUNKS && leaves <= EK_SP_MAX_CHUNKS * EK_PW_FULL_LEAVES &&
           wait_over && columns;
}
inline bool ek_pam_tables_cover(int32_t tab_lo, int32_t tab_n, int32_t cid0, int32_t count)
{
    return tab_lo == cid0 && count <= tab_n;
}

// ---- the sweep's arithmetic ---------------------------------------------------------------
// the window at `cid`: clusters [cid, hi), cnt of them
struct EkSweepWin {
    int32_t hi, cnt;
    EkSweepWin(int32_t cid, int32_t K, int32_t width) : hi(std::min(K, cid + width)), cnt(hi - cid) {}
    // (the counts the next window starts with ride along when this one covers its
    // clusters -- n_slots == cnt: no empty cluster in the way --: how many)
    int32_t ride_along(int32_t n_slots, int32_t K, int32_t width) const
    {
        return n_slots == cnt ? std::min(K, hi + width) - hi : 0;
    }
};
// ... and they stand if the window ran to its end
inline bool ek_sweep_counts_stand(int32_t ncnt, int32_t n_done, int32_t n_slots)
{
    return ncnt > 0 && n_done == n_slots;
}

// numpy's legacy RandomState.choice(m) / randint(0, m): 32-bit outputs of the
// Mersenne Twister masked to the bits of m - 1, values above it rejected; m == 1
// consumes nothing.  `raw` are such outputs, *pos the next unused one.
// -> 0: drawn, 1: the outputs ran out (nothing consumed)
inline int ek_draw_at(const uint32_t *raw, int64_t n_raw, int64_t *pos, int64_t m, int64_t *out)
{
    const uint64_t rng = (uint64_t)(m - 1);
    if (rng == 0) {
        *out = 0;
        return 0;
    }
    uint64_t mask = rng;
    mask |= mask >> 1;
    mask |= mask >> 2;
    mask |= mask >> 4;
    mask |= mask >> 8;
    mask |= mask >> 16;
    int64_t p = *pos;
    for (;;) {
        if (p >= n_raw)
            return 1;
        const uint64_t v = raw[p++] & mask;
        if (v <= rng) {
            *out = (int64_t)v;
            *pos = p;
            return 0;
        }
    }
}
