// ek_run_policy.h -- what the k-centers run loops decide between two batches, in plain
// C++17: no HIP, nothing of the context.  ek_run_rounds (ek_api_run.hip, one shard) and
// ek_ms_run (ek_api_ms.hip, a group of shards) enqueue a batch, wait once, and hand the
// counters that came back to the structs below; every threshold lives here once.  The
// header builds for the host alone (tests/test_run_policy_host.py drives it from a shim).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

// A wait that doubles while what it waits for keeps losing: `left` batches to go, `next`
// the length of the wait after this one, from `first` up to `most`.
struct EkWait {
    int left = 0, next, first, most;
    constexpr EkWait(int first_, int most_) : next(first_), first(first_), most(most_) {}
    void lose()
    {
        left = next;
        next = std::min(2 * next, most);
    }
    void reset() { next = first; }
    bool tick()                 // a batch went by: was it one of a wait?
    {
        if (left <= 0)
            return false;
        --left;
        return true;
    }
};

// ---- pick cap ------------------------------------------------------------------------
// How many far frames per label the candidate pick keeps (ek_top_dev.h): 4 suits
// frames in clouds around templates, 16 a continuous landscape (round 5: the
// walk 1.3e10 -> 2.5e10 pairs/s).  By the yield the rounds show: a batch that
// accepts under 65 % of its guesses lets the next batch of the same form try the
// other value; it stays if it accepts a tenth more, a look that loses waits twice
// as long (80 % and a twentieth cost the ladder on template data 9 % at 125 000
// frames: the early rounds of 8 sit just under 80 % there).
// A cap set by option (pick_cap > 0) never moves.  Across shards the numbers are ones
// every shard sees alike.
struct EkPickCap {
    int cap;
    bool adaptive;
    bool probing = false;
    EkWait wait{2, 64};
    int form = 0;               // the form the home yield was taken at
    double yield_home = 0.0;
    explicit EkPickCap(int option) : cap(option > 0 ? option : 4), adaptive(option <= 0) {}
    // a batch of `ran` rounds of `T` candidates accepted `got` centers; `room`: centers
    // still to find, as the caller counts them
    void update(int T, int32_t got, int32_t ran, int32_t room)
    {
        if (!adaptive || ran <= 0)
            return;
        const double yield = (double)got / ((double)ran * T);
        if (probing) {
            probing = false;
            if (T == form && yield > yield_home + 0.1) {
                wait.reset();               // the other value is home now
            } else {
                cap = cap == 4 ? 16 : 4;    // back
                wait.lose();
            }
        } else if (!wait.tick() && yield < 0.65 && room > 4 * T) {
            yield_home = yield;
            form = T;
            cap = cap == 4 ? 16 : 4;
            probing = true;
        }
    }
};

// the first guess of the centers a round of T candidates accepts
inline double ek_per_round_guess(int T) { return 0.6 * T; }

// ---- single shard: the form ladder -----------------------------------------------------
// A round with T candidates costs more than a one-center step (more FMAs per
// byte, the small kernels that decide the chain) and accepts between 1 and T
// centers.  At the very start of a fit the guesses rarely hit -- every new
// center reshapes the distances of most frames -- and one-center steps are the
// faster way forward; soon after, nearly every guess is accepted.  Both forms
// produce the same centers, labels and distances, so the choice is free: every
// batch is timed on the device (centers per millisecond) and the other form is
// tried for a short batch at intervals that double while it keeps losing.
struct EkFormLadder {
    // the forms the run moves between, by candidates per pass
    int ladder[4], n = 0;
    bool adaptive;
    int home = 0;               // ladder index of the form being run
    int form;                   // ... its candidates per pass (the probe's while probing)
    bool probing = false;
    int probe_up = 1;           // direction of the next probe (they alternate)
    double rate_home = 0.0;     // centers per ms of the home form
    int32_t gap = 8;            // centers until another form is tried again
    int32_t since = 0;          // centers since one last was
    // adaptive: no form is pinned (candidates = -1, adaptation on); tri: the triangle
    // inequality applies to this run; Tmax: the widest form
    EkFormLadder(bool adaptive_, bool tri, int Tmax) : adaptive(adaptive_)
    {
        // (triangle inequality, round 5: the rounds of 4 .. 32 candidates leave out
        // the tiles none of their candidates can change -- ek_round_ti_* --, the
        // one-center steps the tiles the new center cannot.
        // Round 4 ran one center per pass with the option on, 3.7 x slower than
        // without it on data where nothing can be left out.)
        if (adaptive || (tri && Tmax <= 1))
            ladder[n++] = 1;
        if (Tmax > 1) {
            // (the ladder is 1 / 8 / 16: rounds of 32 run only where the option pins them,
            // and a pinned form has no ladder -- `adaptive` needs candidates = -1)
            if (adaptive && Tmax >= 16)
                ladder[n++] = 8;
            ladder[n++] = Tmax;
        }
        form = ladder[0];
    }
    // centers until the ladder wants the host back
    int32_t due(int32_t left) const { return adaptive ? std::max(gap - since, 1) : left; }
    // which form next: the batch accepted `got` centers in `ms` milliseconds
    void update(int32_t got, double ms, double per_round)
    {
        if (!adaptive)
            return;
        const double rate = got / std::max(ms, 1e-6);
        if (probing) {
            probing = false;
            since = 0;
            if (rate > rate_home) {     // the probed form wins: it is home now
                for (int q = 0; q < n; ++q)
                    if (ladder[q] == form)
                        home = q;
                rate_home = rate;
                gap = 8;
            } else {                    // back, and wait twice as long
                form = ladder[home];
                gap = std::min(gap * 2, 1024);
            }
            return;
        }
        rate_home = rate;
        since += got;
        if (since < gap)
            return;
        // Which neighbour on the ladder is worth a look?  One-center steps
        // can only win while rounds accept fewer than ~1.4 centers (the cost
        // ratio of the two forms); a narrower round only while the wider one
        // accepts fewer than the narrower could at its lower cost (8 / 16:
        // cost ratio <= 1.35); a wider round only if the chain of the
        // current one is usually accepted whole -- it breaks where the
        // farthest point is not a stored candidate, and more candidates
        // behind that point change nothing.
        const bool up = up_ok(per_round), down = down_ok(per_round);
        int target = -1;
        if (up && down)
            target = probe_up ? home + 1 : home - 1;
        else if (up)
            target = home + 1;
        else if (down)
            target = home - 1;
        if (target >= 0) {
            probe_up = target > home ? 0 : 1;
            form = ladder[target];
            probing = true;
        } else {
            since = 0;
        }
    }
    bool up_ok(double per_round) const
    {
        const int T = ladder[home];
        return home + 1 < n && (T == 1 || per_round >= 0.8 * T);
    }
    bool down_ok(double per_round) const
    {
        if (home <= 0)
            return false;
        if (ladder[home - 1] == 1)
            return per_round < 1.8;
        return per_round < 1.35 * ladder[home - 1];
    }
};

// ---- a group of shards: the ladder of ek_ms_run -----------------------------------------
// Rounds of 8 or of 16 candidates: early in a fit every new center reshapes
// most frames' distances and a round accepts one to three of its guesses --
// eight of them then cost less than sixteen.  ek_run_rounds moves between
// the forms by measured centers per ms; here every shard has to take the
// SAME decision at the same round, so it is taken from what they all see
// alike: the centers the rounds of a batch accepted.  Rounds of 8 while they
// accept fewer than 6.5; a batch of 16 that accepts fewer than 8.5 per round
// goes back to 8 and the next try waits twice as many batches.  On SMALL shards
// (option key 18 = 1, set by sharded.kcenters_sharded for every rank alike when
// the largest shard has under 300 000 frames) 4.5 and 5.5: with the exchange's
// tails a round of 16 costs only 1.3 x a round of 8 on a 125 000-frame shard and
// the ladder lost 7 % there to staying narrow too long -- while at 10^6 frames
// per shard the lower thresholds cost 8 % (a third of the early rounds of 16
// break and are offered again, 0.2 ms each).  A change of
// form costs one exchange without a pass (the state's farthest frames are
// offered again).  Results do not depend on the form.
// Round 5: rounds of 32 -- two passes of 16 behind ONE plan, chain and
// exchange -- once rounds of 16 are usually accepted whole (>= 14 per round);
// back to 16 when a batch of them accepts fewer than 22 per round (what 16
// would accept at most, with half the passes), the next try twice as far off.
struct EkGroupLadder {
    bool on;                    // the group moves between forms (else: Tmax throughout)
    int Tmax;
    double up16, down16;
    EkWait wait16{1, 64}, wait32{1, 64};
    EkGroupLadder(bool on_, int Tmax_, bool small_shards)
        : on(on_), Tmax(Tmax_), up16(small_shards ? 4.5 : 6.5),
          down16(small_shards ? 5.5 : 8.5)
    {
    }
    int first() const { return on ? 8 : Tmax; }
    // the form after a batch of `ran` rounds of T that accepted `per_round` centers each
    int update(int T, double per_round, int32_t ran)
    {
        if (!on || ran <= 0)
            return T;
        int want = T;
        if (T == 8) {
            if (!wait16.tick() && per_round >= up16)
                want = 16;
        } else if (T == 16) {
            if (per_round < down16) {
                want = 8;
                wait16.lose();
            } else {
                wait16.reset();
                if (!wait32.tick() && Tmax == 32 && per_round >= 14.0)
                    want = 32;
            }
        } else if (per_round < 22.0) {
            want = 16;
            wait32.lose();
        } else {
            wait32.reset();
        }
        return want;
    }
};

// ---- pause of the triangle masks -----------------------------------------------------------
// (the masks cost two small launches per round; where they leave nothing
// out -- frames in no order: the bench's data -- they pause, for twice as
// many batches each time a look finds nothing again)
struct EkTriPause {
    EkWait wait{2, 64};         // batches without masks / the next pause
    unsigned long long seen[2] = {0, 0};    // the counters at the last look
    bool paused() const { return wait.left > 0; }
    // a batch ran with masks: the device's counters (pairs looked at, left out) now
    void look(const unsigned long long now[2])
    {
        const unsigned long long looked = now[0] - seen[0], left_out = now[1] - seen[1];
        seen[0] = now[0];
        seen[1] = now[1];
        if (looked > 0 && left_out * 50 < looked)   // under 2 % left out
            wait.lose();
        else
            wait.reset();
    }
    // a batch of rounds ran without them
    void skipped() { (void)wait.tick(); }
};

// ---- the active view (ek_view.hip; DESIGN.md 4a "Active view") ---------------------
// The policy's two numbers are options (EK_OPT_VIEW_RHO, EK_OPT_VIEW_RATIO, per mille):
// a view's guard sits at rho x the maximum it was built at (frames at up to about half
// of that are settled), and a view is built when it would stream at most ratio x the
// frames streamed now.
static constexpr int EK_VIEW_MIN_ROUNDS = 24;   // rounds left that make a rebuild worth it
static constexpr int EK_VIEW_BATCH = 16;        // rounds between two looks at the policy
// The look (ek_view_look_kernel) rides behind the last round of a batch and comes back
// with the control word.  Looks that find nothing settled pause, as the triangle masks
// do: 1, 2, 4, 8 batches after an estimate above EK_VIEW_IDLE x the frames streamed;
// a paused batch may be EK_VIEW_PAUSED_BATCH rounds long.
static constexpr double EK_VIEW_IDLE = 0.95;
static constexpr int EK_VIEW_PAUSE_MAX = 8;
static constexpr int EK_VIEW_PAUSED_BATCH = 4 * EK_VIEW_BATCH;
static constexpr double EK_VIEW_REL = 1e-3, EK_VIEW_ABS = 1e-3;     // ek_round_ti_*'s margin

struct EkViewPlan {
    float theta = 0.f;          // frames at up to theta are settled; <= 0: no decision
    double guard = 0.0;         // no center is accepted at or below it under the view
    int64_t est = 0;            // frames a view built now would hold
    bool build = false;
};

struct EkViewPolicy {
    EkWait pause{1, EK_VIEW_PAUSE_MAX};     // batches without a look / the next pause
    // The answer to a look: last_max the maximum it was taken at, cnt what it counted,
    // view_n the frames of the live view (0: none), n the shard's frames, left the
    // centers still to find.
    EkViewPlan decide(float last_max, double rho, double shrink, const uint32_t cnt[2],
                      int64_t view_n, int64_t n, int32_t left, double per_round, bool forced)
    {
        EkViewPlan p;
        // frames at up to theta are settled while centers are accepted above
        // guard = 2 theta (1 + rel) + abs = rho x the maximum now
        const double th = (rho * (double)last_max - EK_VIEW_ABS) / (2.0 * (1.0 + EK_VIEW_REL));
        p.theta = (float)th;
        if ((double)p.theta > th)
            p.theta = std::nextafterf(p.theta, 0.f);
        if (!(p.theta > 0.f))
            return p;
        p.guard = 2.0 * (double)p.theta * (1.0 + EK_VIEW_REL) + EK_VIEW_ABS;
        // how many frames a view built now would hold (cnt, counted on the
        // device at the theta of the same maximum): those of this store
        // above theta (what is pending not applied: a few too many) and, under
        // a view, the shard's frames outside it that a lower theta lets in
        // again (the shard's own copy of the view's frames is as old as the
        // view: every one of them counts there)
        p.est = (int64_t)cnt[0] +
                (view_n > 0 ? std::max<int64_t>(0, (int64_t)cnt[1] - view_n) : 0);
        const int64_t store_n = view_n > 0 ? view_n : n;    // the frames streamed now
        p.build = forced ? p.est < n
                         : ((double)p.est <= shrink * (double)store_n &&
                            (double)left >= EK_VIEW_MIN_ROUNDS * std::max(per_round, 1.0));
        if (!forced) {
            if ((double)p.est > EK_VIEW_IDLE * (double)store_n)
                pause.lose();
            else if (p.build || (double)p.est <= shrink * (double)store_n)
                pause.reset();
        }
        return p;
    }
};

// ---- batch lengths: rounds (or steps) between two looks at the control word ------------
// long enough to amortise the host's look at the control word, short
// enough to come back when another form is due
// view: 0 no view policy, 1 looks every batch, 2 the looks pause
inline int32_t ek_batch_single(int form, int32_t left, int32_t due, double per_round,
                               bool probing, bool forced, int view)
{
    const bool one = form == 1;
    int32_t batch;
    if (one)    // (never past the goal: a step has no limit check of its own)
        batch = std::min(left, probing ? 4 : std::min(due, 256));
    else if (probing)
        batch = 3;
    else
        batch = std::max(2, std::min(256, (int32_t)(std::min(left, due) / per_round) + 1));
    // (the policy of the active view looks at the state between batches; forced
    // views -- tests -- are rebuilt every other round)
    if (forced)
        batch = std::min(batch, 2);
    else if (view && !one)
        batch = std::min(batch, view == 2 ? EK_VIEW_PAUSED_BATCH : EK_VIEW_BATCH);
    return batch;
}

// Rounds of 8 between two looks at the group's ladder.  Rounds 3-5: 24 exchanges, of which the
// early ones were a third exchanges without a pass -- 17 to 19 passes.  With the headers
// first (round 6) an exchange is a pass, and 24 of them kept the million-frame fit in
// rounds of 8 for 74 passes instead of 56 (0.338 s against 0.321); 12: 47 passes, 0.318 s
// (16: 0.340; the 125 000-frame shard does not care: 12.85 / 13.0 / 12.9 us per center).
// -DEK_MS_BATCH8=.. builds the others.
#ifndef EK_MS_BATCH8
#define EK_MS_BATCH8 12
#endif
inline int32_t ek_batch_group(int T, int32_t left, double per_round, bool ladder)
{
    int32_t batch = std::max(2, std::min(256, (int32_t)(left / per_round) + 2));
    if (ladder)
        batch = std::min(batch, T == 8 ? EK_MS_BATCH8 : (T == 16 ? 64 : 48));
    return batch;
}
