// ek_api_run.hip -- the C ABI of include/enspara_hip.h: the k-centers fit of one shard.
// ek_kcenters_run and the loop behind it (ek_run_rounds: batches of steps or rounds, one
// host wait each), and the host side of the active view (ek_view.hip).  What the loop
// decides between two batches is in ek_run_policy.h, which builds without HIP.
#include "ek_ctx.h"
#include "ek_run_policy.h"
#include "ek_view.h"
#include <cmath>

// ---- the active view's buffers (kernels: ek_view.hip; when to build one: EkViewPolicy) -------
void ek_view_free(ek_ctx *c)
{
    (void)ek_dev_free(c->v_tiles);
    (void)ek_dev_free(c->v_qtiles);
    (void)ek_dev_free(c->v_G);
    (void)ek_dev_free(c->v_dist);
    (void)ek_dev_free(c->v_assign);
    (void)ek_dev_free(c->v_act);
    (void)ek_dev_free(c->v_blockcnt);
    (void)ek_dev_free(c->v_blockoff);
    (void)ek_dev_free(c->v_count);
    (void)ek_dev_free(c->v_selcnt);
    c->v_tiles = c->v_qtiles = nullptr;
    c->v_G = nullptr;
    c->v_dist = nullptr;
    c->v_assign = nullptr;
    c->v_act = c->v_blockcnt = c->v_blockoff = c->v_count = c->v_selcnt = nullptr;
    c->view_cap = 0;
}

// room for a view of `frames` frames (whole tiles); EK_ENOMEM: there is none, and the
// context remembers
static int ek_view_alloc(ek_ctx *c, int64_t frames)
{
    const int64_t cap = (frames + EK_TILE - 1) / EK_TILE * EK_TILE;
    if (c->view_cap >= cap)
        return EK_OK;
    EK_HIP(ek_wait(c));
    ek_view_free(c);
    const size_t nt = (size_t)(cap / EK_TILE), A3 = (size_t)3 * c->A;
    const size_t nblk = ek_view_sel_blocks(std::max<int64_t>(c->n, 1));
    hipError_t e = hipSuccess;
#define EK_VALLOC(ptr, bytes)                                                  \
    if (e == hipSuccess)                                                       \
        e = ek_malloc_named(c, (void **)&(ptr), (bytes), #ptr);
    EK_VALLOC(c->v_tiles, nt * A3 * EK_TILE * sizeof(float));
    EK_VALLOC(c->v_qtiles, ek_quad_tiles_bytes((int64_t)nt, c->A));
    EK_VALLOC(c->v_G, (size_t)cap * sizeof(double));
    EK_VALLOC(c->v_dist, (size_t)cap * sizeof(float));
    EK_VALLOC(c->v_assign, (size_t)cap * sizeof(int32_t));
    EK_VALLOC(c->v_act, (size_t)cap * sizeof(uint32_t));
    EK_VALLOC(c->v_blockcnt, nblk * sizeof(uint32_t));
    EK_VALLOC(c->v_blockoff, nblk * sizeof(uint32_t));
    // (the looks' words are zeroed by the looks themselves, ek_view_look_kernel: a
    // selection, which may come between two looks, counts into a word of its own)
    EK_VALLOC(c->v_count, 4 * sizeof(uint32_t));
    EK_VALLOC(c->v_selcnt, sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemsetAsync(c->v_count, 0, 4 * sizeof(uint32_t), c->stream);
#undef EK_VALLOC
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ek_view_free(c);
        if (e == hipErrorOutOfMemory) {
            c->view_nomem = true;
            return EK_ENOMEM;
        }
        EK_HIP(e);
    }
    c->view_cap = cap;
    c->v_parity = 0;
    return EK_OK;
}

// a run's view, for the one who has to put it back
struct EkViewRun {
    bool on = false;
    int64_t n = 0;              // frames in it
    int32_t label_lo = 0;       // centers from this label on carry positions of the view
    double guard = 0.0;         // no center is accepted at or below it
    bool tiles_valid = false;   // v_tiles holds this view (built on demand from v_qtiles)
};

// 0xFF bytes all over the view's buffers (active view 3, ek_view_layout_check)
static hipError_t ek_view_poison(ek_ctx *c)
{
    const size_t cap = (size_t)c->view_cap, nt = cap / EK_TILE, A3 = (size_t)3 * c->A;
    hipError_t e =
        hipMemsetAsync(c->v_tiles, 0xFF, nt * A3 * EK_TILE * sizeof(float), c->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(c->v_qtiles, 0xFF, ek_quad_tiles_bytes((int64_t)nt, c->A),
                           c->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(c->v_G, 0xFF, cap * sizeof(double), c->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(c->v_dist, 0xFF, cap * sizeof(float), c->stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(c->v_assign, 0xFF, cap * sizeof(int32_t), c->stream);
    return e;
}

// the view's store from the selection c->v_act[0 .. n_v): traces, distances, labels and
// the quad copy; without a quad copy in the context (rounds of 8 at most) the frame-minor
// tiles instead.  No frame-major copy: the rounds read the shard's through v_act
// (ek_run_use_store).  -> whether v_tiles holds the view
static bool ek_view_build(ek_ctx *c, int64_t n_v)
{
    ek_launch_view_build(c->v_act, n_v, c->A, c->qt_valid, c->aos, c->G, c->dist, c->assign,
                         c->qt_valid ? c->v_qtiles : c->v_tiles, c->v_G, c->v_dist, c->v_assign,
                         c->stream);
    return !c->qt_valid;
}

static void ek_view_scatter_back(ek_ctx *c, EkViewRun &v)
{
    ek_launch_view_scatter(c->v_act, v.n, c->v_dist, c->v_assign, c->dist, c->assign,
                           c->hist, v.label_lo, c->hist_cap, c->ctl, c->goff, c->stream);
    v.on = false;
}

// ---- one descriptor of a round, for both loops ----------------------------------------------
// over the shard's own store; ek_run_rounds points it at a view as well (ek_run_use_store)
void ek_round_of(ek_ctx *c, int T, double cutoff, EkRound &R)
{
    R.dist = c->dist;
    R.assign = c->assign;
    R.vecs = c->vecs;
    R.n = c->n;
    R.n_pad = c->n_pad;
    R.goff = c->goff;
    R.A = c->A;
    R.T = T;
    R.tiles = c->tiles;
    R.qtiles = c->qtiles;
    R.aos = c->aos;
    R.act = nullptr;
    R.G = c->G;
    R.recs = c->recsT;
    R.plan = c->plan;
    R.pend = c->pend;
    R.ord = c->ord;
    R.blockmax = c->blockmax;
    R.pm = c->pm;
    R.fm = c->fine_pick ? c->fm : nullptr;
    // (the per-prefix maxima in the pass: where they pay -- shards of up to ~half a
    // million frames: 10 % of a fit at 125 000; at 10^6 the pass's extra instructions
    // cost what the chain kernel's sweep did, profiles/r06/sweep_ab_*.log)
    R.sweep = (c->pass_sweep == 2 ||
               (c->pass_sweep == 1 && ek_sweep_pays(c->n))) ? 1 : 0;
    R.top = c->top;
    R.ctile = c->ctile;
    R.ctrace = c->ctrace;
    R.hist = c->hist;
    R.ctl = c->ctl;
    R.tick = c->tick;
    R.rows = c->rows;
    R.vmask = c->vmask;
    R.cutoff = cutoff;
    R.pick_cap = c->pick_cap > 0 ? c->pick_cap : 4;
}

// ---- which form the run takes (ek_last_run_form) ------------------------------------------
// Over the shard's whole store, for the widest form of the run (Tmax candidates; 1: steps
// of one center alone): a view has frame counts of its own, and the ladder's narrower
// forms read shorter or equal lists.
static void ek_note_run_form(ek_ctx *c, int fpl, int nt, bool fused, int Tmax, int sweep,
                             bool fine_buf)
{
    const int nb = (int)((c->n + EK_BLOCK - 1) / EK_BLOCK);
    const bool fine = fused && Tmax > 1 && fine_buf && ek_fine_fits(nb);
    c->last_form[0] = fpl;
    c->last_form[1] = nt ? 1 : 0;
    c->last_form[2] = sweep ? 1 : 0;
    c->last_form[3] = fine ? 1 : 0;
    c->last_form[4] = nb;
    c->last_form[5] = Tmax > 1 ? (fine ? 4 * (int64_t)nb : nb) : ek_step_blocks(fpl, c->n);
}

// ---- k-centers rounds on one shard, in the form that pays (ek_run_policy.h) -----------------
#define EK_RC(call)                                                            \
    do {                                                                       \
        const int rc_ = (call);                                                \
        if (rc_)                                                               \
            return rc_;                                                        \
    } while (0)

// what the steps of one run share
struct EkRun {
    ek_ctx *c;
    EkViewRun &view;
    int32_t first_label, goal;
    double dist_cutoff;
    bool tri;                   // the triangle inequality applies to this run
    bool fused;                 // three launches per round (ek_round.hip)
    int fpl, nt;
    int view_mode;              // c->active_view where a view may be used, else 0
    bool forced;
    double rho, shrink;
    EkRound R;                  // the round over the store the rounds see: the shard's
    int nb = 0;                 //   own, or its active view; its blocks of EK_BLOCK
    EkFormLadder lad;
    EkPickCap cap;
    EkTriPause ti;
    EkViewPolicy vp;
    int held = -1;              // form the candidate record(s) were picked for
    bool pending = false;       // a fused round may have left a chain to apply
    bool masks_fresh = false;   // ti_tmask describes the plan the next pass will run
    bool looked = false;        // the last batch carried a look: look_cnt is its answer
    uint32_t look_cnt[2] = {0, 0};
    EkCtl cr;                   // the control word as the last batch left it
    double per_round;           // centers per round of the current wide form
    int32_t rounds_before = 0;
    EkRun(ek_ctx *c_, EkViewRun &view_, bool adaptive, bool tri_, int Tmax)
        : c(c_), view(view_), tri(tri_), lad(adaptive, tri_, Tmax), cap(c_->pick_cap),
          per_round(ek_per_round_guess(lad.form))
    {
        memset(&cr, 0, sizeof(cr));
    }
};

// ---- reserve the triangle buffers -----------------------------------------------------------
static int ek_run_reserve_tri(ek_ctx *c, int32_t goal)
{
    if (goal > c->ti_cap) {
        EK_HIP(ek_wait(c));
        (void)ek_dev_free(c->ti_D);
        c->ti_D = nullptr;
        c->ti_cap = 0;
        EK_HIP(ek_dev_malloc((void **)&c->ti_D, (size_t)(goal + 1) * sizeof(float)));
        c->ti_cap = goal + 1;
    }
    if (!c->ti_skip)        // (each only if it is missing)
        EK_HIP(ek_dev_malloc((void **)&c->ti_skip,
                             (size_t)std::max<int64_t>(c->n_tiles, 1)));
    if (!c->ti_stats)
        EK_HIP(ek_dev_malloc((void **)&c->ti_stats, 2 * sizeof(unsigned long long)));
    EK_HIP(hipMemsetAsync(c->ti_stats, 0, 2 * sizeof(unsigned long long),
                          c->stream));
    if (goal > c->ti_rtab_cap) {
        EK_HIP(ek_wait(c));
        (void)ek_dev_free(c->ti_rtab);
        c->ti_rtab = nullptr;
        c->ti_rtab_cap = 0;
        EK_HIP(ek_dev_malloc((void **)&c->ti_rtab,
                         (size_t)(goal + 1) * EK_MAX_CANDS * sizeof(float)));
        c->ti_rtab_cap = goal + 1;
    }
    if (!c->ti_tmask)
        EK_HIP(ek_dev_malloc((void **)&c->ti_tmask,
                         (size_t)std::max<int64_t>(c->n_tiles, 1) * sizeof(uint32_t)));
    return EK_OK;
}

// ---- the store the rounds see: the shard's own, or its active view ---------------------------
static void ek_run_use_store(EkRun &run, bool the_view)
{
    ek_ctx *c = run.c;
    EkRound &R = run.R;
    if (the_view) {
        R.dist = c->v_dist;
        R.assign = c->v_assign;
        R.tiles = c->v_tiles;
        R.qtiles = c->v_qtiles;
        R.aos = c->aos;         // (frame-major rows stay the shard's: ek_round_row)
        R.act = c->v_act;
        R.G = c->v_G;
        R.n = run.view.n;
        R.n_pad = (run.view.n + EK_TILE - 1) / EK_TILE * EK_TILE;
    } else {
        R.dist = c->dist;
        R.assign = c->assign;
        R.tiles = c->tiles;
        R.qtiles = c->qtiles;
        R.aos = c->aos;
        R.act = nullptr;
        R.G = c->G;
        R.n = c->n;
        R.n_pad = c->n_pad;
    }
    run.nb = (int)((R.n + EK_BLOCK - 1) / EK_BLOCK);
    R.sweep = (run.fused && (c->pass_sweep == 2 ||
                             (c->pass_sweep == 1 && ek_sweep_pays(R.n)))) ? 1 : 0;
    // (under a view no center is accepted at or below its guard: the stop rule
    // itself refuses it -- chain walk, plan and step kernel alike)
    R.cutoff = the_view ? std::max(run.dist_cutoff, run.view.guard) : run.dist_cutoff;
}

// the whole store again: what is pending applied, the view's results scattered
static void ek_run_leave_view(EkRun &run)
{
    if (run.pending) {
        ek_launch_round_flush(run.R, run.c->stream);
        run.pending = false;
    }
    ek_view_scatter_back(run.c, run.view);
    ek_run_use_store(run, false);
}

// ---- active view: enter, rebuild or stay, by the look the last batch carried ----------------
static int ek_run_enter_view(EkRun &run, int32_t left)
{
    ek_ctx *c = run.c;
    EkViewRun &view = run.view;
    run.looked = false;
    const EkViewPlan p =
        run.vp.decide(run.cr.last_max, run.rho, run.shrink, run.look_cnt,
                      view.on ? view.n : 0, c->n, left, run.per_round, run.forced);
    if (!p.build)
        return EK_OK;
    if (view.on) {
        ek_run_leave_view(run);
    } else if (run.pending) {
        ek_launch_round_flush(run.R, c->stream);
        run.pending = false;
    }
    uint32_t nv = 0;
    ek_launch_view_select(c->dist, c->n, p.theta, c->v_blockcnt, c->v_blockoff, c->v_act,
                          c->view_cap, c->v_selcnt, c->stream);
    EK_CHECK_LAUNCH();
    EK_HIP(hipMemcpyAsync(&nv, c->v_selcnt, sizeof(nv), hipMemcpyDeviceToHost, c->stream));
    EK_HIP(ek_wait(c));
    if (nv > 0 && (int64_t)nv < c->n && (int64_t)nv <= c->view_cap) {
        view.n = nv;
        view.label_lo = run.cr.n_done;
        view.guard = p.guard;
        if (run.view_mode == 3)
            EK_HIP(ek_view_poison(c));
        view.tiles_valid = ek_view_build(c, view.n);
        EK_CHECK_LAUNCH();
        view.on = true;
        ek_run_use_store(run, true);
        EK_HIP(hipMemsetAsync(c->vmask, 0, (size_t)(run.R.n_pad / EK_WAVE) * sizeof(uint32_t),
                              c->stream));
        c->view_stats[0]++;
    }
    run.held = -1;      // the pick in the new space, from a recomputed blockmax
    return EK_OK;
}

// ---- the record(s) a form starts from ---------------------------------------------------------
// from blockmax as it stands: one record for a step, the plan of a round (with_masks: and
// its triangle masks)
static void ek_run_pick_records(EkRun &run, int form, bool with_masks)
{
    ek_ctx *c = run.c;
    const EkRound &R = run.R;
    if (form == 1) {
        ek_launch_pick(c->blockmax, run.nb, R.dist, R.tiles, R.G, R.n, c->A, c->goff,
                       c->recsT, c->ctl, c->stream);
    } else if (run.fused) {
        ek_launch_round_chain(R, 1, c->stream);
        ek_launch_round_next(R, 1, c->stream);
        if (with_masks) {
            ek_launch_round_ti(R, run.goal, c->stream);
            run.masks_fresh = R.tmask != nullptr;
        }
    } else {
        ek_launch_pickT(c->blockmax, run.nb, R.tiles, R.G, R.assign, c->A, form, c->goff,
                        c->recsT, c->ctl, c->top, c->stream);
    }
}

static int ek_run_bootstrap(EkRun &run, int form)
{
    ek_ctx *c = run.c;
    if (run.pending) {          // leaving a fused form: the state as it stands
        ek_launch_round_flush(run.R, c->stream);
        run.pending = false;
    } else if (run.held <= 1) {
        // the step kernel's partials are per FPL frames
        ek_launch_blockmax(run.R.dist, run.R.n, c->blockmax, c->stream);
    }
    ek_run_pick_records(run, form, true);
    EK_CHECK_LAUNCH();
    if (form != 1)
        run.per_round = ek_per_round_guess(form);
    run.held = form;
    return EK_OK;
}

// ---- one batch: steps (one-center form), fused rounds or unfused rounds ---------------------
static int ek_run_enqueue_steps(EkRun &run, int32_t batch)
{
    ek_ctx *c = run.c;
    const EkRound &R = run.R;
    for (int32_t r = 0; r < batch; ++r) {
        const int label = run.cr.n_done + r;
        const bool skip = run.tri && label >= 1;
        if (skip)
            ek_launch_ti(R.aos, R.G, c->A, c->hist, label, c->goff, c->recsT, c->ti_D, R.dist,
                         R.assign, R.n, c->ctl, c->ti_skip, c->ti_stats, c->stream);
        ek_launch_step(run.fpl, 0, run.nt, R.tiles, R.G, R.dist, R.assign, c->scratch,
                       c->recsT, 1, R.n, c->A, label, R.cutoff, c->blockmax, c->hist, c->ctl,
                       c->stream, skip ? c->ti_skip : nullptr);
        ek_launch_pick(c->blockmax, ek_step_blocks(run.fpl, R.n), R.dist, R.tiles, R.G, R.n,
                       c->A, c->goff, c->recsT, c->ctl, c->stream);
        EK_CHECK_LAUNCH();
    }
    return EK_OK;
}

// sampled timing of the dominant kernel (bench.py): is the next pass one to time?
// (only passes over the whole store: bench.py's roofline multiplies the
// sampled time by the shard's frames per launch)
static bool ek_run_sample(EkRun &run, int form)
{
    ek_ctx *c = run.c;
    const bool sample =
        !run.view.on && c->samp_every > 0 && (c->samp_count++ % c->samp_every) == 0 &&
        2 * (size_t)c->samp_used + 1 < c->samp_ev.size();
    if (sample)
        c->samp_form[c->samp_used] = form;
    return sample;
}

static int ek_run_enqueue_fused(EkRun &run, int form, int32_t batch)
{
    ek_ctx *c = run.c;
    const EkRound &R = run.R;
    for (int32_t r = 0; r < batch; ++r) {
        const bool sample = ek_run_sample(run, form);
        if (sample)
            EK_HIP(hipEventRecord(c->samp_ev[2 * c->samp_used], c->stream));
        ek_launch_round_pass(R, c->stream);
        if (sample) {
            EK_HIP(hipEventRecord(c->samp_ev[2 * c->samp_used + 1], c->stream));
            c->samp_used++;
        }
        ek_launch_round_chain(R, 0, c->stream);
        ek_launch_round_next(R, 0, c->stream);
        ek_launch_round_ti(R, run.goal, c->stream);
        EK_CHECK_LAUNCH();
        run.pending = true;
    }
    return EK_OK;
}

static int ek_run_enqueue_unfused(EkRun &run, int form, int32_t batch)
{
    ek_ctx *c = run.c;
    const EkRound &R = run.R;
    const int nb = run.nb;
    for (int32_t r = 0; r < batch; ++r) {
        const bool sample = ek_run_sample(run, form);
        ek_launch_plan(c->recsT, form, c->A, form, R.cutoff, c->planD, c->plan, c->hist,
                       c->ctl, c->stream);
        if (sample)
            EK_HIP(hipEventRecord(c->samp_ev[2 * c->samp_used], c->stream));
        ek_launch_pass(form, R.tiles, R.qtiles, R.G, R.dist, R.assign, c->vecs, R.n, R.n_pad,
                       c->A, c->recsT, c->plan, c->blockmax, c->ctile, c->ctrace, c->stream);
        if (sample) {
            EK_HIP(hipEventRecord(c->samp_ev[2 * c->samp_used + 1], c->stream));
            c->samp_used++;
        }
        if (c->chain) {
            ek_launch_chain_max(R.dist, c->vecs, R.n, R.n_pad, c->plan, c->pm, 1, c->goff,
                                c->stream);
            ek_launch_chain_decide_local(c->blockmax, c->pm, nb, ek_chain_max_blocks(R.n),
                                         c->goff, R.cutoff, c->plan, c->hist, c->ctl,
                                         c->stream);
            ek_launch_chain_apply(c->vecs, R.n, R.n_pad, R.dist, R.assign, c->plan,
                                  c->blockmax, c->stream);
        } else {
            for (int j = 1; j < form; ++j) {
                ek_launch_localmax_check(c->blockmax, nb, c->goff, R.cutoff, c->plan, c->hist,
                                         c->ctl, c->stream);
                ek_launch_apply(c->vecs, R.G, R.n, R.n_pad, c->A, R.dist, R.assign, c->plan,
                                c->blockmax, c->stream);
            }
        }
        ek_launch_pickT(c->blockmax, nb, R.tiles, R.G, R.assign, c->A, form, c->goff, c->recsT,
                        c->ctl, c->top, c->stream);
        EK_CHECK_LAUNCH();
    }
    return EK_OK;
}

static int ek_run_enqueue_batch(EkRun &run, int form, int32_t batch)
{
    const EkRound &R = run.R;
    if (R.tmask && !run.masks_fresh) {  // (after a pause: the masks of the plan at hand)
        ek_launch_round_ti(R, run.goal, run.c->stream);
        run.masks_fresh = true;
    }
    if (!R.tmask)
        run.masks_fresh = false;        // (this batch's rounds do not make any)
    if (form == 1)
        return ek_run_enqueue_steps(run, batch);
    return run.fused ? ek_run_enqueue_fused(run, form, batch)
                     : ek_run_enqueue_unfused(run, form, batch);
}

// ---- the look for the next decision rides on the batch --------------------------------------
static int ek_run_carry_look(EkRun &run)
{
    ek_ctx *c = run.c;
    if (!run.view_mode || run.vp.pause.tick())
        return EK_OK;
    const int64_t want_cap =
        run.forced ? c->n : (int64_t)std::ceil(run.shrink * (double)c->n);
    if (ek_view_alloc(c, want_cap) != EK_OK) {
        (void)hipGetLastError();
        run.view_mode = 0;      // (no memory for it: the run is what it was without)
        return EK_OK;
    }
    // one launch: the store being streamed and, under a view, the shard's distances;
    // the counts into this look's pair of words, the last look's pair zeroed for the next
    const int parity = c->v_parity;
    ek_launch_view_look(run.R.dist, run.R.n, run.view.on ? c->dist : nullptr, c->n, c->ctl,
                        run.rho, EK_VIEW_REL, EK_VIEW_ABS, c->v_count, parity, c->stream);
    EK_CHECK_LAUNCH();
    c->v_parity = parity ^ 1;
    EK_HIP(hipMemcpyAsync(run.look_cnt, c->v_count + 2 * parity, sizeof(run.look_cnt),
                          hipMemcpyDeviceToHost, c->stream));
    run.looked = true;
    return EK_OK;
}

// ---- read back and account: the batch's one wait ------------------------------------------------
// -> got: centers the batch accepted, ran: passes that really ran
static int ek_run_read_back(EkRun &run, int form, int32_t &got, int32_t &ran)
{
    ek_ctx *c = run.c;
    const bool one = form == 1, masks = run.R.tmask != nullptr;
    const int32_t before = run.cr.n_done;
    EK_HIP(hipMemcpyAsync(&run.cr, c->ctl, sizeof(run.cr), hipMemcpyDeviceToHost, c->stream));
    unsigned long long ti_now[2] = {0, 0};
    if (masks)
        EK_HIP(hipMemcpyAsync(ti_now, c->ti_stats, sizeof(ti_now), hipMemcpyDeviceToHost,
                              c->stream));
    EK_HIP(ek_wait(c));
    if (masks)
        run.ti.look(ti_now);
    else if (!one)
        run.ti.skipped();
    got = run.cr.n_done - before;
    // (a step that finds the stop rule met returns at once)
    ran = one ? got : run.cr.n_rounds - run.rounds_before;
    run.rounds_before = run.cr.n_rounds;
    c->st_rounds[ek_form_slot(form)] += ran;
    c->st_centers[ek_form_slot(form)] += got;
    c->view_stats[1] += (int64_t)ran * run.R.n;
    c->view_stats[2] += (int64_t)ran * (c->n - run.R.n);
    return EK_OK;
}

// ---- leave a view on stop ---------------------------------------------------------------------
// The view's maximum is at or below its guard (or the cut-off): the
// centers from here on may move settled frames, and the shard's maximum
// may be one of them.  Back to the whole store, which decides whether
// this is the run's stop; the next look at the policy comes after a batch
// has given the shard's own maximum.
static int ek_run_leave_on_stop(EkRun &run)
{
    ek_ctx *c = run.c;
    if ((double)run.cr.last_max > run.dist_cutoff)
        c->view_stats[3]++;
    ek_run_leave_view(run);
    const int32_t zero = 0;     // (what the stop latched: the flag; the plan's
    // `go` is made again by the bootstrap, the limit never changed)
    EK_HIP(hipMemcpyAsync(&c->ctl->stopped, &zero, sizeof(zero), hipMemcpyHostToDevice,
                          c->stream));
    EK_HIP(ek_wait(c));
    run.cr.stopped = 0;
    run.held = -1;
    run.looked = false;         // (it counted in the view's space, against its maximum)
    return EK_OK;
}

// ---- finish: what is pending applied, the whole store, the records, the run's numbers ------
static int ek_run_finish(EkRun &run, int32_t max_new, int32_t *n_added,
                         int64_t *center_index_out, float *center_dist_out,
                         float *final_maxdist)
{
    ek_ctx *c = run.c;
    const int form = run.lad.form;
    if (run.pending) {          // the last round's accepted chain
        ek_launch_round_flush(run.R, c->stream);
        run.pending = false;
        EK_CHECK_LAUNCH();
    }
    if (run.view.on || (run.held < 0 && run.cr.n_done > run.first_label)) {
        // The run ends under a view (or just left one): results back, then the
        // records and the maximum of the state as the whole store has it -- what the
        // last round's pick leaves without a view.
        if (run.view.on)
            ek_run_leave_view(run);
        ek_launch_blockmax(run.R.dist, run.R.n, c->blockmax, c->stream);
        run.R.T = form;
        ek_run_pick_records(run, form, false);
        EK_CHECK_LAUNCH();
        run.held = form;
        EK_HIP(hipMemcpyAsync(&run.cr, c->ctl, sizeof(run.cr), hipMemcpyDeviceToHost,
                              c->stream));
        EK_HIP(ek_wait(c));
    }
    if (run.tri) {
        unsigned long long st[2] = {0, 0};
        EK_HIP(hipMemcpyAsync(st, c->ti_stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
        EK_HIP(ek_wait(c));
        c->ti_tiles = (int64_t)st[0];
        c->ti_skipped = (int64_t)st[1];
    }
    EK_HIP(hipEventRecord(c->ev1, c->stream));
    EK_HIP(ek_wait(c));
    EK_HIP(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    // leave the records describing the state: [0] = the shard's farthest point
    if (run.held == 1) {
        ek_launch_blockmax(c->dist, c->n, c->blockmax, c->stream);
        EK_CHECK_LAUNCH();
    }
    if (run.held >= 0)          // (nothing ran: the slot still describes the state)
        EK_HIP(hipMemcpyAsync(c->rec, c->recsT, ek_rec_bytes(c->A), hipMemcpyDeviceToDevice,
                              c->stream));
    EK_HIP(ek_wait(c));
    const int32_t added_t =
        std::min(max_new, std::max(0, run.cr.n_done - run.first_label));
    // (passes over the frames: a round of 32 is two)
    const int64_t passes = c->st_rounds[0] + c->st_rounds[1] + c->st_rounds[2] +
                           c->st_rounds[3] + 2 * c->st_rounds[4];
    c->last_launches = (int32_t)passes;
    c->last_passes = (int32_t)passes;
    if (n_added)
        *n_added = added_t;
    if (final_maxdist)
        *final_maxdist = run.cr.last_max;
    if (added_t > 0 && (center_index_out || center_dist_out))
        EK_RC(ek_history_download(c, run.first_label, added_t, center_index_out,
                                  center_dist_out, nullptr));
    return EK_OK;
}

static int ek_run_rounds_in(ek_ctx *c, int Tmax, int32_t first_label,
                            int32_t max_new, double dist_cutoff, int32_t *n_added,
                            int64_t *center_index_out, float *center_dist_out,
                            float *final_maxdist, EkViewRun &view)
{
    EK_RC(ek_spec_alloc(c));
    if (!c->evb0) {
        EK_HIP(ek_event_create(&c->evb0));
        EK_HIP(ek_event_create(&c->evb1));
    }
    const int32_t goal = first_label + max_new;
    EkCtl ctlw;
    memset(&ctlw, 0, sizeof(ctlw));
    ctlw.n_done = first_label;
    ctlw.limit = goal;
    EK_HIP(hipMemcpyAsync(c->ctl, &ctlw, sizeof(ctlw), hipMemcpyHostToDevice,
                          c->stream));
    EK_HIP(ek_wait(c));
    for (int m = 0; m < EK_N_FORMS; ++m)
        c->st_rounds[m] = c->st_centers[m] = 0;
    c->view_stats[0] = c->view_stats[1] = c->view_stats[2] = c->view_stats[3] = 0;
    // Triangle inequality (option key 11; reference `use_triangle_inequality`,
    // kcenters.py:287-296): one center at a time, tiles that cannot change are
    // not read.  Needs every frame's distance to be the one to the center its
    // label names (a fresh run) and distances that behave like a metric.
    const bool tri = c->tri && c->state_exact && first_label == 0 && c->A >= 3;
    if (tri)
        EK_RC(ek_run_reserve_tri(c, goal));
    c->ti_tiles = c->ti_skipped = 0;
    // three launches per round (ek_round.hip) when the pieces it is built from
    // are the ones selected; rounds of 32 exist in that form only
    const bool fused = c->fused && c->chain == 1;
    if (Tmax == 32 && !fused)
        Tmax = EK_LEGACY_CANDS;
    if (Tmax >= 16) {
        const int eq = ek_ensure_qtiles(c);
        if (eq == EK_ENOMEM)
            Tmax = 8;
        else if (eq != EK_OK)
            return eq;
    }
    // an explicit request (option key 4 = 4, 8 or 16) pins the wide form
    const bool adaptive = c->cands == -1 && c->adapt;
    // Active view (option key 24): needs distances that ARE the distance to the center
    // the label names, a metric, the fused rounds, and the triangle option off (its
    // kernels read hist[].gidx as positions of old centers)
    const int view_mode =
        (c->state_exact && c->A >= 3 && fused && !c->tri && !c->view_nomem) ? c->active_view
                                                                             : 0;
    EkRun run(c, view, adaptive, tri, Tmax);
    run.first_label = first_label;
    run.goal = goal;
    run.dist_cutoff = dist_cutoff;
    run.fused = fused;
    run.fpl = ek_pick_fpl(c);
    run.nt = ek_pick_nt(c);
    run.view_mode = view_mode;
    run.forced = view_mode >= 2;
    run.rho = c->view_rho / 1000.0;
    run.shrink = c->view_ratio / 1000.0;
    run.cr.n_done = first_label;
    EkRound &R = run.R;
    ek_round_of(c, Tmax, dist_cutoff, R);
    R.ti_tab = tri ? c->ti_rtab : nullptr;
    R.ti_stats = tri ? c->ti_stats : nullptr;
    ek_run_use_store(run, false);
    // (only a round of exactly 16 candidates has the pass sweep: ek_round_chain_kernel)
    ek_note_run_form(c, run.fpl, run.nt, fused, Tmax, R.sweep && Tmax == 16, R.fm != nullptr);
    EK_HIP(hipEventRecord(c->ev0, c->stream));
    while (run.cr.n_done < goal) {
        const int32_t left = goal - run.cr.n_done;
        const int form = run.lad.form;
        const bool one = form == 1;
        R.T = form;
        const bool masks = tri && fused && form >= 4 && !run.ti.paused();
        R.tmask = masks ? c->ti_tmask : nullptr;
        R.pick_cap = run.cap.cap;
        if (run.view_mode && run.looked && std::isfinite(run.cr.last_max))
            EK_RC(ek_run_enter_view(run, left));
        run.looked = false;
        // (a view's frame-minor tiles are made when a kernel that reads them runs under
        // it: the rounds of 8, the one-center step and its pick)
        if (view.on && !view.tiles_valid && form < 16) {
            ek_launch_view_tiles(c->v_qtiles, R.n_pad / EK_TILE, c->A, c->v_tiles, c->stream);
            EK_CHECK_LAUNCH();
            view.tiles_valid = true;
        }
        if (run.held != form)
            EK_RC(ek_run_bootstrap(run, form));
        const int32_t batch =
            ek_batch_single(form, left, run.lad.due(left), run.per_round, run.lad.probing,
                            run.forced, !run.view_mode ? 0 : (run.vp.pause.left > 0 ? 2 : 1));
        EK_HIP(hipEventRecord(c->evb0, c->stream));
        EK_RC(ek_run_enqueue_batch(run, form, batch));
        EK_HIP(hipEventRecord(c->evb1, c->stream));
        EK_RC(ek_run_carry_look(run));
        int32_t got = 0, ran = 0;
        EK_RC(ek_run_read_back(run, form, got, ran));
        if (view.on && run.cr.stopped) {
            EK_RC(ek_run_leave_on_stop(run));
            if (run.cr.n_done < goal)
                continue;
        }
        if (run.cr.stopped || run.cr.n_done >= goal)
            break;
        if (!one)
            run.per_round = std::max(1.0, (double)got / std::max(ran, 1));
        // (the pick cap: not while a form is being probed, fused rounds only)
        if (!one && fused && !run.lad.probing)
            run.cap.update(form, got, ran, left);
        if (!adaptive)
            continue;
        float bms = 0.f;
        EK_HIP(hipEventElapsedTime(&bms, c->evb0, c->evb1));
        run.lad.update(got, bms, run.per_round);
    }
    return ek_run_finish(run, max_new, n_added, center_index_out, center_dist_out,
                         final_maxdist);
}

static int ek_run_rounds(ek_ctx *c, int Tmax, int32_t first_label,
                         int32_t max_new, double dist_cutoff, int32_t *n_added,
                         int64_t *center_index_out, float *center_dist_out,
                         float *final_maxdist)
{
    EkViewRun view;
    const int rc = ek_run_rounds_in(c, Tmax, first_label, max_new, dist_cutoff, n_added,
                                    center_index_out, center_dist_out, final_maxdist, view);
    if (rc != EK_OK && view.on) {
        // an error under a view: distances, labels and history back in the shard's
        // own space all the same (what is pending stays unapplied, as without a view)
        ek_view_scatter_back(c, view);
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
    }
    return rc;
}

extern "C" int ek_kcenters_run(ek_ctx *c, int32_t first_label, int32_t max_new,
                               double dist_cutoff, int32_t *n_added,
                               int64_t *center_index_out,
                               float *center_dist_out, float *final_maxdist)
{
    if (!c)
        return ek_fail(EK_EARG, "NULL context");
    if (!c->loaded)
        return ek_fail(EK_ESTATE, "ek_kcenters_run: no frames loaded");
    if (first_label < 0 || max_new < 0)
        return ek_fail(EK_EARG, "ek_kcenters_run: negative argument");
    EK_HIP(hipSetDevice(c->device));
    int rc = ek_ensure_hist(c, first_label + max_new);
    if (rc)
        return rc;
    // the accepted-label counter restarts at first_label for this run
    EkCtl ctl0;
    memset(&ctl0, 0, sizeof(ctl0));
    ctl0.n_done = first_label;
    EK_HIP(hipMemcpyAsync(c->ctl, &ctl0, offsetof(EkCtl, last_max),
                          hipMemcpyHostToDevice, c->stream));
    EK_HIP(ek_wait(c));

    const int T = ek_pick_cands(c, true);
    // (the triangle inequality's bookkeeping lives in ek_run_rounds, also for one
    // center per pass)
    if ((T > 1 || c->tri) && c->n > 0)
        return ek_run_rounds(c, T, first_label, max_new, dist_cutoff, n_added,
                             center_index_out, center_dist_out, final_maxdist);

    // With no distance cut-off the trip count is known: enqueue everything.
    // With a cut-off, enqueue in batches and look at the stop flag in between
    // (steps enqueued past the stopping point are no-ops on the device).
    ek_note_run_form(c, ek_pick_fpl(c), ek_pick_nt(c), false, 1, 0, false);
    // (this loop has no view: ek_view_stats must not go on telling of an earlier run's)
    c->view_stats[0] = c->view_stats[1] = c->view_stats[2] = c->view_stats[3] = 0;
    const bool open_loop = !(dist_cutoff > 0.0);
    const int32_t batch = open_loop ? max_new : 16;
    int32_t issued = 0;
    EkCtl ctl;
    memset(&ctl, 0, sizeof(ctl));
    ctl.n_done = first_label;
    EK_HIP(hipEventRecord(c->ev0, c->stream));
    while (issued < max_new) {
        const int32_t todo = std::min(batch, max_new - issued);
        for (int32_t i = 0; i < todo; ++i) {
            rc = ek_kcenters_step(c, nullptr, 1, first_label + issued + i,
                                  dist_cutoff, nullptr);
            if (rc)
                return rc;
        }
        issued += todo;
        if (!open_loop) {
            EK_HIP(hipMemcpyAsync(&ctl, c->ctl, sizeof(ctl),
                                  hipMemcpyDeviceToHost, c->stream));
            EK_HIP(ek_wait(c));
            if (ctl.stopped)
                break;
        }
    }
    EK_HIP(hipEventRecord(c->ev1, c->stream));
    EK_HIP(hipMemcpyAsync(&ctl, c->ctl, sizeof(ctl), hipMemcpyDeviceToHost,
                          c->stream));
    EK_HIP(ek_wait(c));
    EK_HIP(hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
    const int32_t added = std::max(0, ctl.n_done - first_label);
    c->last_launches = added;
    if (n_added)
        *n_added = added;
    if (final_maxdist)
        *final_maxdist = ctl.last_max;
    if (added > 0 && (center_index_out || center_dist_out)) {
        rc = ek_history_download(c, first_label, added, center_index_out,
                                 center_dist_out, nullptr);
        if (rc)
            return rc;
    }
    return EK_OK;
}

extern "C" int ek_view_layout_check(ek_ctx *c, float theta, int64_t *out)
{
    if (!c || !out)
        return ek_fail(EK_EARG, "ek_view_layout_check: NULL argument");
    if (!c->loaded || c->n <= 0)
        return ek_fail(EK_ESTATE, "ek_view_layout_check: no frames loaded");
    EK_HIP(hipSetDevice(c->device));
    out[0] = out[1] = out[2] = out[3] = 0;
    int rc = ek_view_alloc(c, c->n);
    if (rc)
        return rc;
    uint32_t nv = 0;
    ek_launch_view_select(c->dist, c->n, theta, c->v_blockcnt, c->v_blockoff, c->v_act,
                          c->view_cap, c->v_selcnt, c->stream);
    EK_CHECK_LAUNCH();
    EK_HIP(hipMemcpyAsync(&nv, c->v_selcnt, sizeof(nv), hipMemcpyDeviceToHost, c->stream));
    EK_HIP(ek_wait(c));
    out[0] = nv;
    if (nv == 0 || (int64_t)nv > c->view_cap)
        return EK_OK;
    const size_t nt = ((size_t)nv + EK_TILE - 1) / EK_TILE, A3 = (size_t)3 * c->A;
    const size_t tile_words = nt * A3 * EK_TILE;
    const size_t quad_bytes = ek_quad_tiles_bytes((int64_t)nt, c->A);
    // the earlier path into scratch: gather -> frame-minor tiles -> quad copy
    float *r_tiles = nullptr, *r_qtiles = nullptr, *r_dist = nullptr;
    double *r_G = nullptr;
    int32_t *r_assign = nullptr;
    unsigned long long *diff = nullptr, got[3] = {0, 0, 0};
    hipError_t e = ek_dev_malloc((void **)&r_tiles, tile_words * sizeof(float));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&r_qtiles, quad_bytes);
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&r_G, (size_t)nv * sizeof(double));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&r_dist, (size_t)nv * sizeof(float));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&r_assign, (size_t)nv * sizeof(int32_t));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&diff, sizeof(got));
    if (e == hipSuccess)
        e = hipMemsetAsync(diff, 0, sizeof(got), c->stream);
    if (e == hipSuccess)
        e = ek_view_poison(c);
    if (e == hipSuccess) {
        ek_launch_view_gather(c->v_act, nv, c->A, c->aos, c->G, c->dist, c->assign, r_tiles,
                              r_G, r_dist, r_assign, c->stream);
        ek_launch_quad_tiles(r_tiles, (int64_t)nt, c->A, r_qtiles, c->stream);
        // a rebuild, and the tiles a reader under the view would ask for
        if (!ek_view_build(c, nv))
            ek_launch_view_tiles(c->v_qtiles, (int64_t)nt, c->A, c->v_tiles, c->stream);
        if (c->qt_valid)
            ek_launch_view_diff(c->v_qtiles, r_qtiles, quad_bytes / 4, diff, c->stream);
        ek_launch_view_diff(c->v_tiles, r_tiles, tile_words, diff + 1, c->stream);
        ek_launch_view_diff(c->v_G, r_G, (size_t)nv * 2, diff + 2, c->stream);
        ek_launch_view_diff(c->v_dist, r_dist, (size_t)nv, diff + 2, c->stream);
        ek_launch_view_diff(c->v_assign, r_assign, (size_t)nv, diff + 2, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(got, diff, sizeof(got), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess)
        e = ek_wait(c);
    else
        (void)hipStreamSynchronize(c->stream);
    (void)ek_dev_free(r_tiles);
    (void)ek_dev_free(r_qtiles);
    (void)ek_dev_free(r_G);
    (void)ek_dev_free(r_dist);
    (void)ek_dev_free(r_assign);
    (void)ek_dev_free(diff);
    EK_HIP(e);
    out[1] = (int64_t)got[0];
    out[2] = (int64_t)got[1];
    out[3] = (int64_t)got[2];
    return EK_OK;
}

extern "C" int ek_last_run_form(ek_ctx *c, int64_t *out)
{
    if (!c || !out)
        return ek_fail(EK_EARG, "ek_last_run_form: NULL argument");
    for (int k = 0; k < 6; ++k)
        out[k] = c->last_form[k];
    return EK_OK;
}

extern "C" int ek_view_stats(ek_ctx *c, int64_t *stats)
{
    if (!c || !stats)
        return ek_fail(EK_EARG, "ek_view_stats: NULL argument");
    for (int k = 0; k < 4; ++k)
        stats[k] = c->view_stats[k];
    return EK_OK;
}
