// ek_api_pam.hip -- the C ABI of include/enspara_hip.h: PAM (k-medoids) entry points.
#include "ek_ctx.h"

// ---- PAM (k-medoids) proposals ----------------------------------------------------------
// working set of a sweep over K medoids
static int ek_pam_alloc(ek_ctx *c, int32_t K)
{
    const size_t nn = (size_t)std::max<int64_t>(c->n, 1);
    const size_t nb = (nn + EK_BLOCK - 1) / EK_BLOCK;
    c->med_K = 0;       // (no working set until this call is through: the entry points test it)
    // (tested by its last member, each buffer made only if it is missing: a call that
    // failed part-way leaves what it got with the context, and the next call makes the rest)
    if (!c->pam_win_host) {
        if (!c->ndist)
            EK_HIP(ek_dev_malloc((void **)&c->ndist, nn * sizeof(float)));
        if (!c->nassign)
            EK_HIP(ek_dev_malloc((void **)&c->nassign, nn * sizeof(int32_t)));
        if (!c->amb)
            EK_HIP(ek_dev_malloc((void **)&c->amb, nn * sizeof(uint32_t)));
        if (!c->amb_best)
            EK_HIP(ek_dev_malloc((void **)&c->amb_best, nn * sizeof(unsigned long long)));
        // [0] ambiguous members, [1] their reach (float bits), [2] listed medoids
        if (!c->amb_count)
            EK_HIP(ek_dev_malloc((void **)&c->amb_count, 4 * sizeof(unsigned int)));
        if (!c->blockcnt)
            EK_HIP(ek_dev_malloc((void **)&c->blockcnt, nb * sizeof(int32_t)));
        if (!c->scan)
            EK_HIP(ek_dev_malloc((void **)&c->scan, nb * sizeof(int64_t)));
        if (!c->sel)
            EK_HIP(ek_dev_malloc((void **)&c->sel, 2 * sizeof(int64_t)));
        {
            EkPwShape hs[2];
            const int64_t n_full = c->n / EK_PW_CHUNK;
            const int last_len = (int)(c->n - n_full * EK_PW_CHUNK);
            ek_pw_build_shape(n_full > 0 ? EK_PW_CHUNK : 0, &hs[0]);
            ek_pw_build_shape(last_len, &hs[1]);
            // the one-launch cost sums (ek_pw_window_kernel) add a full chunk's
            // 64 leaves of 128 as a perfect in-order binary tree: true for
            // numpy's pairwise split of 8192 elements, checked here
            {
                bool ok = n_full == 0 ||
                          (hs[0].n_leaves == EK_PW_FULL_LEAVES && hs[0].n_levels == 6);
                for (int i = 0; ok && n_full > 0 && i < EK_PW_FULL_LEAVES; ++i)
                    ok = hs[0].leaf_off[i] == 128 * i && hs[0].leaf_len[i] == 128;
                for (int k = 0; ok && n_full > 0 && k < hs[0].n_nodes; ++k) {
                    // level-ordered nodes: level 1 joins leaves (2j, 2j+1), ..
                    const int lev_start[7] = {0, 32, 48, 56, 60, 62, 63};
                    int lev = 0;
                    while (k >= lev_start[lev + 1])
                        ++lev;
                    const int j = k - lev_start[lev];
                    const int base = lev == 0 ? 0 : hs[0].n_leaves + lev_start[lev - 1];
                    ok = hs[0].node_l[k] == base + 2 * j &&
                         hs[0].node_r[k] == base + 2 * j + 1;
                }
                c->pw_tail_ok = ok;
            }
            c->pw_n_full = (int)n_full;
            c->pw_leaves = (int)n_full * EK_PW_FULL_LEAVES + hs[1].n_leaves;
            c->pw_chunks = (int)n_full + (last_len > 0 ? 1 : 0);
            if (!c->pw_shapes)
                EK_HIP(ek_dev_malloc((void **)&c->pw_shapes, sizeof(hs)));
            EK_HIP(hipMemcpy(c->pw_shapes, hs, sizeof(hs), hipMemcpyHostToDevice));
            if (!c->sq_part)
                EK_HIP(ek_dev_malloc((void **)&c->sq_part,
                             (2 * (size_t)std::max(c->pw_leaves, 1) +
                              2 * (size_t)std::max(c->pw_chunks, 1)) *
                                 sizeof(double)));
        }
        if (!c->sq_out)
            EK_HIP(ek_dev_malloc((void **)&c->sq_out, 2 * sizeof(double)));
        if (!c->bat_blockcnt)
            EK_HIP(ek_dev_malloc((void **)&c->bat_blockcnt,
                         (size_t)EK_PAM_WIN * nb * sizeof(int32_t)));
        if (!c->bat_scan)
            EK_HIP(ek_dev_malloc((void **)&c->bat_scan,
                         (size_t)EK_PAM_WIN * nb * sizeof(int64_t)));
        // [0,8) counts, [8,16) selected frames, [16,24) requested member ranks
        if (!c->bat_sel)
            EK_HIP(ek_dev_malloc((void **)&c->bat_sel,
                         3 * EK_PAM_WIN * sizeof(int64_t)));
        if (!c->moved)
            EK_HIP(ek_dev_malloc((void **)&c->moved, sizeof(unsigned int)));
        EK_HIP(hipMemsetAsync(c->moved, 0, sizeof(unsigned int), c->stream));
        if (!c->pam_out_dev)
            EK_HIP(ek_dev_malloc((void **)&c->pam_out_dev, sizeof(EkPamOut)));
        if (!c->pam_out_host)
            EK_HIP(ek_pinned_malloc((void **)&c->pam_out_host, sizeof(EkPamOut),
                             hipHostMallocDefault));
        if (!c->pam_win_dev)
            EK_HIP(ek_dev_malloc((void **)&c->pam_win_dev, sizeof(EkPamWin)));
        // (coherent and mapped: the window's kernel writes the record there itself)
        if (!c->pam_win_host)
            EK_HIP(ek_pinned_malloc((void **)&c->pam_win_host, sizeof(EkPamWin),
                             hipHostMallocCoherent | hipHostMallocMapped));
    }
    c->tab.restore = -1;
    c->sp.begin();
    c->cnt.invalidate_batch();
    c->pf.begin();
    if (K > c->med_cap) {
        EK_HIP(ek_wait(c));
        (void)ek_dev_free(c->med_aos);
        (void)ek_dev_free(c->med_G);
        (void)ek_dev_free(c->med_idx);
        (void)ek_dev_free(c->med_list);
        (void)ek_dev_free(c->dtab);
        c->med_list = nullptr;
        c->dtab = nullptr;
        c->med_aos = nullptr;
        c->med_G = nullptr;
        c->med_idx = nullptr;
        c->med_cap = 0;
        EK_HIP(ek_dev_malloc((void **)&c->med_aos,
                         (size_t)(K + 1) * 3 * c->A * sizeof(float)));
        EK_HIP(ek_dev_malloc((void **)&c->med_G, (size_t)(K + 1) * sizeof(double)));
        EK_HIP(ek_dev_malloc((void **)&c->med_idx, (size_t)(K + 1) * sizeof(int64_t)));
        EK_HIP(ek_dev_malloc((void **)&c->med_list, (size_t)(K + 1) * sizeof(int32_t)));
        EK_HIP(ek_dev_malloc((void **)&c->dtab,
                         (size_t)3 * EK_PAM_WIN * (K + 1) * sizeof(float)));
        c->med_cap = K;
    }
    c->med_K = K;
    c->pam_cid = -1;
    c->cnt.invalidate_one();
    c->tab.invalidate();
    return EK_OK;
}

static int ek_tmp_idx(ek_ctx *c, int64_t count)
{
    if (count <= c->tmp_idx_cap)
        return EK_OK;
    EK_HIP(ek_wait(c));
    (void)ek_dev_free(c->tmp_idx);
    c->tmp_idx = nullptr;
    c->tmp_idx_cap = 0;
    const int64_t cap = std::max<int64_t>(1024, count);
    EK_HIP(ek_dev_malloc((void **)&c->tmp_idx, (size_t)cap * sizeof(int64_t)));
    c->tmp_idx_cap = cap;
    return EK_OK;
}

extern "C" int ek_pam_begin(ek_ctx *c, const int64_t *medoid_frames, int32_t K)
{
    if (!c || !medoid_frames || K < 1)
        return ek_fail(EK_EARG, "ek_pam_begin: bad argument");
    if (!c->loaded)
        return ek_fail(EK_ESTATE, "ek_pam_begin: no frames loaded");
    for (int32_t i = 0; i < K; ++i)
        if (medoid_frames[i] < 0 || medoid_frames[i] >= c->n)
            return ek_fail(EK_EARG, "ek_pam_begin: medoid %d = frame %lld out "
                                    "of range", i, (long long)medoid_frames[i]);
    EK_HIP(hipSetDevice(c->device));
    int rc = ek_pam_alloc(c, K);
    if (rc)
        return rc;
    EK_HIP(hipMemcpyAsync(c->med_idx, medoid_frames, (size_t)K * sizeof(int64_t),
                          hipMemcpyHostToDevice, c->stream));
    EK_HIP(ek_wait(c));
    ek_launch_gather_frames(c->tiles, c->G, c->A, c->med_idx, K, 0, c->med_aos,
                            c->med_G, c->stream);
    EK_CHECK_LAUNCH();
    return EK_OK;
}

// ---- PAM with medoids / proposals that live on other shards ---------------------------
extern "C" int ek_centered_frames(ek_ctx *c, const int64_t *local_frames,
                                  const int32_t *rows, int32_t count,
                                  float *aos_dev, double *G_dev)
{
    if (!c || count < 0 || (count > 0 && (!local_frames || !rows)) || !aos_dev ||
        !G_dev)
        return ek_fail(EK_EARG, "ek_centered_frames: bad argument");
    if (!c->loaded)
        return ek_fail(EK_ESTATE, "ek_centered_frames: no frames loaded");
    if (count == 0)
        return EK_OK;
    for (int32_t i = 0; i < count; ++i)
        if (local_frames[i] < 0 || local_frames[i] >= c->n || rows[i] < 0)
            return ek_fail(EK_EARG, "ek_centered_frames: item %d (frame %lld, "
                                    "row %d) out of range", i,
                           (long long)local_frames[i], rows[i]);
    EK_HIP(hipSetDevice(c->device));
    int rc = ek_tmp_idx(c, 2 * (int64_t)count);
    if (rc)
        return rc;
    std::vector<int64_t> h(2 * (size_t)count);
    for (int32_t i = 0; i < count; ++i) {
        h[i] = local_frames[i];
        h[(size_t)count + i] = rows[i];
    }
    EK_HIP(hipMemcpyAsync(c->tmp_idx, h.data(), h.size() * sizeof(int64_t),
                          hipMemcpyHostToDevice, c->stream));
    EK_HIP(ek_wait(c));
    ek_launch_gather_rows(c->tiles, c->G, c->A, c->tmp_idx, c->tmp_idx + count,
                          count, aos_dev, G_dev, c->stream);
    EK_CHECK_LAUNCH();
    return EK_OK;
}

extern "C" int ek_pam_begin_table(ek_ctx *c, const float *aos_dev,
                                  const double *G_dev, int32_t K)
{
    if (!c || !aos_dev || !G_dev || K < 1)
        return ek_fail(EK_EARG, "ek_pam_begin_table: bad argument");
    if (!c->loaded)
        return ek_fail(EK_ESTATE, "ek_pam_begin_table: no frames loaded");
    EK_HIP(hipSetDevice(c->device));
    int rc = ek_pam_alloc(c, K);
    if (rc)
        return rc;
    EK_HIP(hipMemcpyAsync(c->med_aos, aos_dev, (size_t)K * 3 * c->A * sizeof(float),
                          hipMemcpyDeviceToDevice, c->stream));
    EK_HIP(hipMemcpyAsync(c->med_G, G_dev, (size_t)K * sizeof(double),
                          hipMemcpyDeviceToDevice, c->stream));
    return EK_OK;
}

extern "C" int ek_pam_count_members(ek_ctx *c, int32_t cid, int64_t *count)
{
    if (!c || !count)
        return ek_fail(EK_EARG, "ek_pam_count_members: NULL argument");
    if (!c->ndist || c->med_K < 1)
        return ek_fail(EK_ESTATE, "ek_pam_count_members: call ek_pam_begin first");
    EK_HIP(hipSetDevice(c->device));
    ek_launch_count_members(c->assign, c->n, cid, c->blockcnt, c->scan, c->sel,
                            c->stream);
    EK_CHECK_LAUNCH();
    EK_HIP(hipMemcpyAsync(count, c->sel, sizeof(int64_t), hipMemcpyDeviceToHost,
                          c->stream));
    EK_HIP(ek_wait(c));
    c->cnt.one(cid, *count);
    return EK_OK;
}

extern "C" int ek_pam_select_member(ek_ctx *c, int32_t cid, int64_t j,
                                    int64_t *frame_index)
{
    if (!c || !frame_index)
        return ek_fail(EK_EARG, "ek_pam_select_member: NULL argument");
    if (!c->ndist || c->med_K < 1)
        return ek_fail(EK_ESTATE, "ek_pam_select_member: call ek_pam_begin first");
    EK_HIP(hipSetDevice(c->device));
    // relies on the scan left by the preceding ek_pam_count_members(cid)
    ek_launch_select_member(c->assign, c->n, cid, c->scan, j, c->sel + 1,
                            c->stream);
    EK_CHECK_LAUNCH();
    EK_HIP(hipMemcpyAsync(frame_index, c->sel + 1, sizeof(int64_t),
                          hipMemcpyDeviceToHost, c->stream));
    EK_HIP(ek_wait(c));
    if (*frame_index < 0)
        return ek_fail(EK_EARG, "ek_pam_select_member: cluster %d has no "
                                "member %lld", cid, (long long)j);
    return EK_OK;
}

// Everything of a proposal after the distance vector `newd` is known and the
// trial medoid table holds the proposal in row cid (ek_pam_trial_kernel, which
// also clears the counters): classification, the ambiguous subset against all
// medoids, both cost sums and the moved-cluster mask, packed into *out (device).
// No read-back.  max_amb bounds the ambiguous set (a subset of cluster cid's
// members) and sizes the follow-up launches.
// decide != nullptr (a slot of the window run): three launches -- the
// classification first takes over the trial state of the slot before if
// *prev_accept says it was accepted, ambiguous members stay marked in the trial
// state until the cost-sum launch resolves them, and that launch's last
// workgroup decides the proposal (EkPamDecide) -- and nothing else to do
static int ek_pam_tail(ek_ctx *c, int32_t cid, const float *newd,
                       int64_t max_amb, int32_t win_lo, int32_t win_count,
                       EkPamOut *out, const EkPamDecide *decide = nullptr,
                       const int32_t *prev_accept = nullptr)
{
    const int K = c->med_K;
    const int fuse = decide != nullptr;
    c->sp.invalidate();         // c->amb is the ambiguous members' list from here on
    const bool prune = ek_pam_prune_ok(c->prune, c->state_exact, c->A);
    // inside a window whose distance tables are in place the classification's
    // last workgroup lists the medoids within reach itself
    const bool tabs = fuse && prune && c->tab.lo == cid - decide->slot &&
                      decide->slot < c->tab.n;
    if (fuse) {
        const size_t tb = (size_t)EK_PAM_WIN * (c->med_cap + 1);
        EkPamClsWin w;
        w.prev_accept = prev_accept;
        w.frames_aos = c->aos;
        w.G = c->G;
        w.A = c->A;
        w.ambt = c->ambt;
        w.ambG = c->ambG;
        w.cap = c->ambt_cap;
        w.O = tabs ? c->dtab + tb + (size_t)decide->slot * K : nullptr;
        w.T = c->dtab;
        w.accepted = decide->win->accept;
        w.K = K;
        w.cid0 = cid - decide->slot;
        w.slot = decide->slot;
        w.list = c->med_list;
        w.tick = c->tick + 192;
        ek_launch_pam_classify_window(c->dist, c->assign, newd, c->n, cid, c->ndist,
                                      c->nassign, c->amb, c->amb_best,
                                      c->amb_count, w, c->stream);
    } else {
        ek_launch_pam_classify(c->dist, c->assign, newd, c->n, cid, c->ndist,
                               c->nassign, c->amb, c->amb_best, c->amb_count,
                               c->amb_count + 1, c->stream, 0);
    }
    if (prune && !tabs)
        ek_launch_pam_prune(c->med_aos, c->med_G, c->A, K, cid, c->amb_count + 1,
                            c->med_list, c->amb_count + 2, c->stream);
    ek_launch_subset_assign(c->tiles, c->G, c->A, c->amb, c->amb_count, max_amb,
                            c->ambt, c->ambG, c->ambt_cap, c->med_aos, c->med_G,
                            K, prune ? c->med_list : nullptr, c->amb_count + 2,
                            newd, cid, c->amb_best, c->stream, fuse != 0);
    if (!fuse)
        ek_launch_pam_scatter(c->amb, c->amb_best, c->amb_count, max_amb, c->ndist,
                              c->nassign, c->stream);
    ek_launch_sumsq_pack(c->dist, c->ndist, c->assign, c->nassign, c->n, win_lo,
                         win_count, c->pw_shapes, c->pw_n_full, c->pw_leaves,
                         c->pw_chunks, c->sq_part, c->amb_count, c->moved, out,
                         c->stream, fuse ? c->amb_best : nullptr,
                         fuse ? c->tick + 128 : nullptr, decide);
    EK_CHECK_LAUNCH();
    return EK_OK;
}

// room for the compacted ambiguous members (before anything of the proposal is
// enqueued: growing it synchronises)
static int ek_pam_amb_room(ek_ctx *c, int64_t max_amb)
{
    if (max_amb <= c->ambt_cap)
        return EK_OK;
    EK_HIP(ek_wait(c));
    (void)ek_dev_free(c->ambt);
    (void)ek_dev_free(c->ambG);
    c->ambt = nullptr;
    c->ambG = nullptr;
    c->ambt_cap = 0;
    const int64_t cap = std::max<int64_t>(
        4096, (max_amb * 5 / 4 + EK_BLOCK - 1) / EK_BLOCK * EK_BLOCK);
    EK_HIP(ek_dev_malloc((void **)&c->ambt, (size_t)cap * 3 * c->A * sizeof(float)));
    EK_HIP(ek_dev_malloc((void **)&c->ambG, (size_t)cap * sizeof(double)));
    c->ambt_cap = cap;
    return EK_OK;
}

// the prefetched distance vector of a local frame, or nullptr
static const float *ek_pam_prefetched(ek_ctx *c, int64_t frame_index)
{
    if (frame_index < 0 || c->pf.external)
        return nullptr;
    for (int32_t j = 0; j < c->pf.count; ++j)
        if (c->pf.frames[j] == frame_index)
            return c->pam_vecs + (size_t)j * c->n_pad;
    return nullptr;
}

// shared body of the local-frame proposal entry points.  The proposed frame's
// index is either `frame_index` (>= 0) or already on the device in c->sel[1].
static int ek_pam_propose_impl(ek_ctx *c, int32_t cid, int64_t frame_index,
                               int64_t max_amb, int64_t *frame_out,
                               double *old_cost, double *new_cost,
                               int64_t *n_ambiguous, int32_t win_lo = 0,
                               int32_t win_count = 0,
                               uint32_t *moved_mask = nullptr)
{
    const int K = c->med_K;
    int rc = ek_pam_amb_room(c, max_amb);
    if (rc)
        return rc;
    const float *newd = ek_pam_prefetched(c, frame_index);
    if (newd)
        ++c->pf.hits;
    else
        ++c->pf.misses;
    const int64_t *idx_dev = c->sel + 1;    // read only when frame_index < 0
    if (!newd) {
        // distances of every frame to the proposed medoid (kmedoids.py:637)
        ek_launch_record_from_frame(c->tiles, c->G, c->A,
                                    frame_index >= 0 ? frame_index : 0,
                                    frame_index >= 0 ? nullptr : idx_dev, c->goff,
                                    c->rec_tmp, c->stream);
        ek_launch_step(ek_pick_fpl(c), 1, ek_pick_nt(c), c->tiles, c->G, c->dist,
                       c->assign, c->scratch, c->rec_tmp, 1, c->n, c->A, 0, 0.0,
                       c->blockmax, c->hist, c->ctl, c->stream);
        EK_CHECK_LAUNCH();
        newd = c->scratch;
    }
    // trial medoid table (undoing a rejected proposal's row first), counters
    c->tab.invalidate();
    ek_launch_pam_trial(c->tiles, c->G, c->A, c->med_aos, c->med_G, K, cid,
                        c->tab.restore, frame_index, idx_dev, nullptr, nullptr,
                        c->amb_count, c->moved, c->stream);
    c->tab.restore = -1;
    rc = ek_pam_tail(c, cid, newd, max_amb, win_lo, moved_mask ? win_count : 0,
                     c->pam_out_dev);
    if (rc)
        return rc;
    int64_t fidx = frame_index;
    EK_HIP(hipMemcpyAsync(c->pam_out_host, c->pam_out_dev, sizeof(EkPamOut),
                          hipMemcpyDeviceToHost, c->stream));
    if (frame_index < 0)
        EK_HIP(hipMemcpyAsync(&fidx, idx_dev, sizeof(int64_t),
                              hipMemcpyDeviceToHost, c->stream));
    EK_HIP(ek_wait(c));
    const EkPamOut r = *c->pam_out_host;
    c->pam_cid = cid;           // pending even if the check below fails
    c->pam_frame = fidx;
    if ((int64_t)r.n_amb > max_amb)
        return ek_fail(EK_EARG, "PAM proposal: cluster %d has %u members that "
                                "stay put, more than the %lld members declared",
                       cid, r.n_amb, (long long)max_amb);
    if (old_cost)
        *old_cost = r.sum_old / (double)c->n;
    if (new_cost)
        *new_cost = r.sum_new / (double)c->n;
    if (n_ambiguous)
        *n_ambiguous = r.n_amb;
    if (moved_mask)
        *moved_mask = r.moved;
    if (frame_out)
        *frame_out = fidx;
    return EK_OK;
}

static int ek_pam_precheck(ek_ctx *c, int32_t cid, const char *who)
{
    if (!c)
        return ek_fail(EK_EARG, "NULL context");
    if (!c->ndist || c->med_K < 1)
        return ek_fail(EK_ESTATE, "%s: call ek_pam_begin first", who);
    if (c->pam_cid >= 0)
        return ek_fail(EK_ESTATE, "%s: previous proposal not committed", who);
    if (cid < 0 || cid >= c->med_K)
        return ek_fail(EK_EARG, "%s: cid=%d out of range", who, cid);
    if ((size_t)3 * c->A * 8 * sizeof(float) > 150 * 1024)
        return ek_fail(EK_EARG, "%s: %d atoms exceed the LDS center tile "
                                "(limit 1600)", who, c->A);
    return EK_OK;
}

extern "C" int ek_pam_propose(ek_ctx *c, int32_t cid, int64_t frame_index,
                              double *old_cost, double *new_cost,
                              int64_t *n_ambiguous)
{
    int rc = ek_pam_precheck(c, cid, "ek_pam_propose");
    if (rc)
        return rc;
    if (frame_index < 0 || frame_index >= c->n)
        return ek_fail(EK_EARG, "ek_pam_propose: frame %lld out of range",
                       (long long)frame_index);
    EK_HIP(hipSetDevice(c->device));
    int64_t m = 0;
    if (c->cnt.cid == cid) {
        m = c->cnt.m;
    } else {
        rc = ek_pam_count_members(c, cid, &m);
        if (rc)
            return rc;
    }
    c->cnt.invalidate_one();
    return ek_pam_propose_impl(c, cid, frame_index, m, nullptr, old_cost,
                               new_cost, n_ambiguous);
}

extern "C" int ek_pam_propose_member(ek_ctx *c, int32_t cid, int64_t j,
                                     int64_t *frame_index, double *old_cost,
                                     double *new_cost, int64_t *n_ambiguous)
{
    int rc = ek_pam_precheck(c, cid, "ek_pam_propose_member");
    if (rc)
        return rc;
    if (c->cnt.cid != cid)
        return ek_fail(EK_ESTATE, "ek_pam_propose_member: call "
                                  "ek_pam_count_members(%d) first", cid);
    if (j < 0 || j >= c->cnt.m)
        return ek_fail(EK_EARG, "ek_pam_propose_member: member %lld of %lld",
                       (long long)j, (long long)c->cnt.m);
    EK_HIP(hipSetDevice(c->device));
    ek_launch_select_member(c->assign, c->n, cid, c->scan, j, c->sel + 1,
                            c->stream);
    EK_CHECK_LAUNCH();
    const int64_t m = c->cnt.m;
    c->cnt.invalidate_one();
    return ek_pam_propose_impl(c, cid, -1, m, frame_index, old_cost, new_cost,
                               n_ambiguous);
}

extern "C" int ek_pam_commit(ek_ctx *c, int accept)
{
    if (!c)
        return ek_fail(EK_EARG, "NULL context");
    if (c->pam_cid < 0)
        return ek_fail(EK_ESTATE, "ek_pam_commit: no proposal pending");
    EK_HIP(hipSetDevice(c->device));
    if (accept) {
        std::swap(c->dist, c->ndist);
        std::swap(c->assign, c->nassign);
    } else {
        // the trial row is put back by the next proposal's first kernel
        c->tab.restore = c->pam_cid;
    }
    c->pam_cid = -1;
    c->cnt.invalidate_one();
    return EK_OK;
}

extern "C" int32_t ek_pam_window_max(void)
{
    return EK_PAM_WIN;
}

// ---- PAM proposal prefetch ------------------------------------------------------------
// A sweep visits clusters 0..K-1 in order and an accepted proposal rarely
// touches the clusters visited next, so the host draws the next few proposals
// ahead of time, gets their distance vectors from ONE pass over the frames
// (ek_pass_kernel<T,false>), and checks each guess when its turn comes.
extern "C" int ek_pam_count_members_batch(ek_ctx *c, int32_t cid0, int32_t count,
                                          int64_t *counts)
{
    if (!c || !counts)
        return ek_fail(EK_EARG, "ek_pam_count_members_batch: NULL argument");
    if (!c->ndist || c->med_K < 1)
        return ek_fail(EK_ESTATE, "ek_pam_count_members_batch: call ek_pam_begin "
                                  "first");
    if (count < 1 || count > EK_PAM_WIN || cid0 < 0 || cid0 + count > c->med_K)
        return ek_fail(EK_EARG, "ek_pam_count_members_batch: clusters [%d,+%d) "
                                "outside [0,%d) or more than %d", cid0, count,
                       c->med_K, EK_PAM_WIN);
    EK_HIP(hipSetDevice(c->device));
    ek_launch_count_members_multi(c->assign, c->n, cid0, count, c->bat_blockcnt,
                                  c->bat_scan, c->bat_sel, c->stream);
    EK_CHECK_LAUNCH();
    EK_HIP(hipMemcpyAsync(counts, c->bat_sel, (size_t)count * sizeof(int64_t),
                          hipMemcpyDeviceToHost, c->stream));
    EK_HIP(ek_wait(c));
    c->cnt.batch(cid0, count);
    return EK_OK;
}

extern "C" int ek_pam_select_members_batch(ek_ctx *c, int32_t cid0, int32_t count,
                                           const int64_t *js, int64_t *frames)
{
    if (!c || !js || !frames)
        return ek_fail(EK_EARG, "ek_pam_select_members_batch: NULL argument");
    if (!c->cnt.batch_covers(cid0, count))
        return ek_fail(EK_ESTATE, "ek_pam_select_members_batch: call "
                                  "ek_pam_count_members_batch(%d, >=%d) first",
                       cid0, count);
    EK_HIP(hipSetDevice(c->device));
    // (a negative rank: that member lives on another shard)
    EK_HIP(hipMemcpyAsync(c->bat_sel + 2 * EK_PAM_WIN, js,
                          (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice,
                          c->stream));
    ek_launch_select_member_multi(c->assign, c->n, cid0, count, c->bat_scan,
                                  c->bat_sel + 2 * EK_PAM_WIN,
                                  c->bat_sel + EK_PAM_WIN, c->stream);
    EK_CHECK_LAUNCH();
    EK_HIP(hipMemcpyAsync(frames, c->bat_sel + EK_PAM_WIN,
                          (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost,
                          c->stream));
    EK_HIP(ek_wait(c));
    c->cnt.invalidate_batch();
    for (int32_t j = 0; j < count; ++j)
        if (frames[j] < 0 && js[j] >= 0)
            return ek_fail(EK_EARG, "ek_pam_select_members_batch: cluster %d has "
                                    "no member %lld", cid0 + j, (long long)js[j]);
    return EK_OK;
}

// A pinned host buffer of `count` elements the device can address, made when first
// asked for, and (want) its device view: nullptr where the mapping fails -- the caller
// copies instead.
template <class T>
static int ek_mapped(T **host, size_t count, bool want, T **dev_view)
{
    *dev_view = nullptr;
    if (!*host)
        EK_HIP(ek_pinned_malloc((void **)host, count * sizeof(T),
                                hipHostMallocCoherent | hipHostMallocMapped));
    void *dp = nullptr;
    if (want && hipHostGetDevicePointer(&dp, *host, 0) == hipSuccess)
        *dev_view = (T *)dp;
    else if (want)
        (void)hipGetLastError();
    return EK_OK;
}

static int ek_pam_vecs_alloc(ek_ctx *c)
{
    if (!c->pam_dprop) {     // (as in ek_pam_alloc: by the last, each only if missing)
        if (!c->pam_vecs)
            EK_HIP(ek_dev_malloc((void **)&c->pam_vecs,
                         (size_t)EK_PAM_WIN * std::max<int64_t>(c->n_pad, 1) *
                             sizeof(float)));
        if (!c->pam_recs)
            EK_HIP(ek_dev_malloc((void **)&c->pam_recs,
                         (size_t)EK_PAM_WIN * ek_rec_bytes(c->A)));
        if (!c->pam_plan)
            EK_HIP(ek_dev_malloc((void **)&c->pam_plan, sizeof(EkPlan)));
        if (!c->pam_dprop)
            EK_HIP(ek_dev_malloc((void **)&c->pam_dprop, EK_PAM_WIN * sizeof(float)));
    }
    return EK_OK;
}

// the three blocks of c->dtab: T, O at + tb, dmin at + 2 tb
static size_t ek_pam_tab_block(const ek_ctx *c) { return (size_t)EK_PAM_WIN * (c->med_cap + 1); }

// The window's tables and, from them, the list of the frames its proposals can touch
// (c->act_list), its length read back: one wait.  Tables made as bounds that list too
// many are made again exactly (the policy's retry).
static int ek_pam_list_within_reach(ek_ctx *c, int count, int32_t win_lo, int32_t win_count,
                                    bool slots, bool prepared, bool bounds, int64_t *n_act)
{
    const int K = c->med_K;
    const size_t tb = ek_pam_tab_block(c);
    const int groups = (count + EK_PAM_GROUP - 1) / EK_PAM_GROUP;
    for (int attempt = 0;; ++attempt) {
        // O (old medoids of the window's clusters) only where the window's slots
        // and the proposals coincide: ek_pam_window_run's pruning reads it
        ek_launch_pam_tables(c->med_aos, c->med_G, c->A, K, c->tab.restore,
                             c->pam_recs, count, win_lo, slots ? count : 0, c->dtab,
                             c->dtab + tb, c->dtab + 2 * tb, c->stream,
                             bounds ? c->pam_dprop : nullptr);
        c->tab.made(win_lo, slots ? count : 0);
        if (attempt > 0)    // (the counter the set-up kernel cleared has been used)
            EK_HIP(hipMemsetAsync(c->amb_count + 3, 0, sizeof(unsigned int), c->stream));
        ek_launch_pam_active(c->dist, c->assign, c->n, c->dtab + 2 * tb, groups, K,
                             win_lo, win_count, c->act_list, c->amb_count + 3,
                             c->stream, prepared || attempt > 0);
        EK_CHECK_LAUNCH();
        EK_HIP(hipMemcpyAsync(c->act_n_host, c->amb_count + 3, sizeof(unsigned int),
                              hipMemcpyDeviceToHost, c->stream));
        EK_HIP(ek_wait(c));
        *n_act = *c->act_n_host;
        if (!c->pf.form.retry_exact(bounds, *n_act, c->n))
            return EK_OK;
        bounds = false;
    }
}

// The restricted form: exact distances at the listed frames only, +inf elsewhere
// (ek_pam.hip, "proposal prefetch restricted ...").  *done = false: the list came out
// too long, nothing was written -- the pass over all frames follows.
static int ek_pam_prefetch_restricted(ek_ctx *c, int count, int32_t win_lo, int32_t win_count,
                                      bool local, bool prepared, bool *done)
{
    *done = false;
    if (!c->act_n_host)
        EK_HIP(ek_pinned_malloc((void **)&c->act_n_host, sizeof(unsigned int),
                             hipHostMallocDefault));
    const bool slots = local && win_count == count;
    // (proposals drawn among their clusters' members, ek_pam_sweep: the
    // proposal-to-medoid table only as the lower bounds the old medoids'
    // table gives, half the pairs -- ek_pam_pairs_kernel<0>)
    const bool bounds =
        c->pf.form.use_bounds(slots && prepared && c->pf.members && c->pam_bounds);
    if (!c->act_list)
        EK_HIP(ek_dev_malloc((void **)&c->act_list,
                         (size_t)std::max<int64_t>(c->n, 1) * sizeof(uint32_t)));
    // the vectors go back to +inf: the entries the window before wrote, if
    // that is all there is (before the list is overwritten)
    const bool sparse_reset = c->pf.vecs.sparse_reset(count);
    if (sparse_reset)
        ek_launch_pam_vecs_reset(c->act_list, c->pf.vecs.rows, c->pf.vecs.cols, c->n_pad,
                                 c->pam_vecs, c->stream);
    c->pf.vecs.whole();
    int64_t n_act = 0;
    int rc = ek_pam_list_within_reach(c, count, win_lo, win_count, slots, prepared, bounds, &n_act);
    if (rc)
        return rc;
    if (!ek_pf_short(n_act, c->n)) {
        c->pf.form.too_many();
        return EK_OK;
    }
    // straight from the frame-major copy, 64 frames x the proposals per workgroup,
    // results scattered into the full vectors
    if (!sparse_reset)
        EK_HIP(hipMemsetD32Async((hipDeviceptr_t)c->pam_vecs, 0x7f800000,
                                 (size_t)count * c->n_pad, c->stream));
    ek_launch_pam_list_dist(c->aos, c->G, c->A, c->act_list, n_act, c->pam_recs,
                            count, c->pam_vecs, c->n_pad, c->stream);
    EK_CHECK_LAUNCH();
    c->pf.vecs.listed(n_act, count, sparse_reset);
    ++c->pf.restricted;
    // the list stays in c->amb until something else uses it: a window run
    // right away may work from it (ek_pam_sparse.hip)
    c->sp.ready = ek_sp_list_ok(slots, n_act);
    c->sp.n_act = n_act;
    *done = true;
    return EK_OK;
}

// a pass over all frames per group of EK_PAM_GROUP proposals
static int ek_pam_prefetch_full(ek_ctx *c, int count, bool prepared)
{
    c->pf.vecs.whole();
    const size_t rstride = ek_rec_bytes(c->A);
    for (int g0 = 0; g0 < count; g0 += EK_PAM_GROUP)
        ek_launch_pass_dist(std::min(count - g0, EK_PAM_GROUP), c->tiles, c->G,
                            c->pam_vecs + (size_t)g0 * c->n_pad, c->n, c->n_pad,
                            c->A, c->pam_recs + (size_t)g0 * rstride, c->pam_plan,
                            c->ctile, c->ctrace, c->stream, prepared && g0 == 0);
    EK_CHECK_LAUNCH();
    ++c->pf.full;
    return EK_OK;
}

// The distance vectors of the `count` records in c->pam_recs.  When the state is
// exact (every frame's distance is the distance to the medoid its label names)
// and the window of clusters being worked through is known, only the frames a
// proposal can touch get exact distances: the others get +inf.
// local: the proposals are frames of this shard, proposal j for cluster
// win_lo + j when win_count == count (the layout ek_pam_window_run expects)
// prepared: ek_launch_pam_setup made the records (plan, candidate tile and the
// cleared active-frame counter come with them)
// *waited: the host waited for the stream on the way (the restricted form's read-back)
static int ek_pam_prefetch_vectors(ek_ctx *c, int count, int32_t win_lo, int32_t win_count,
                                   bool local, bool prepared = false, bool *waited = nullptr)
{
    if (waited)
        *waited = false;
    c->tab.invalidate();
    c->sp.invalidate();
    if (c->pf.form.try_restricted(c->prune, c->state_exact, c->A, win_count, c->n)) {
        bool done = false;
        int rc = ek_pam_prefetch_restricted(c, count, win_lo, win_count, local, prepared, &done);
        if (rc)
            return rc;
        if (waited)
            *waited = true;
        if (done)
            return EK_OK;
    }
    return ek_pam_prefetch_full(c, count, prepared);
}

static int ek_pam_prefetch_frames(ek_ctx *c, const int64_t *frames, int32_t count,
                                  int32_t win_lo, int32_t win_count)
{
    if (!c || (!frames && count > 0))
        return ek_fail(EK_EARG, "ek_pam_prefetch: NULL argument");
    if (!c->ndist || c->med_K < 1)
        return ek_fail(EK_ESTATE, "ek_pam_prefetch: call ek_pam_begin first");
    if (count < 0 || count > EK_PAM_WIN)
        return ek_fail(EK_EARG, "ek_pam_prefetch: count=%d outside [0,%d]", count,
                       EK_PAM_WIN);
    for (int32_t j = 0; j < count; ++j)
        if (frames[j] < 0 || frames[j] >= c->n)
            return ek_fail(EK_EARG, "ek_pam_prefetch: frame %lld out of range",
                           (long long)frames[j]);
    EK_HIP(hipSetDevice(c->device));
    c->pf.invalidate();
    if (count == 0)
        return EK_OK;
    int rc = ek_pam_vecs_alloc(c);
    if (rc)
        return rc;
    const bool prepared = c->ctile != nullptr;
    if (prepared)
        ek_launch_pam_setup(c->aos, c->G, c->A, frames, count, c->goff, c->pam_recs,
                            c->ctile, c->ctrace, c->pam_plan, c->amb_count + 3,
                            c->stream, c->dist, c->pam_dprop);
    else
        ek_launch_records_from_frames(c->aos, c->G, c->A, frames, count, c->goff,
                                      c->pam_recs, c->stream);
    rc = ek_pam_prefetch_vectors(c, count, win_lo, win_count, true, prepared);
    if (rc)
        return rc;
    for (int32_t j = 0; j < count; ++j)
        c->pf.frames[j] = frames[j];
    c->pf.count = count;
    c->pf.external = false;
    return EK_OK;
}

extern "C" int ek_pam_prefetch_window(ek_ctx *c, const int64_t *frames, int32_t count,
                                      int32_t win_lo, int32_t win_count)
{
    if (c && (win_lo < 0 || win_count < 0 || win_lo + win_count > c->med_K))
        return ek_fail(EK_EARG, "ek_pam_prefetch_window: clusters [%d,+%d) outside "
                                "[0,%d)", win_lo, win_count, c->med_K);
    return ek_pam_prefetch_frames(c, frames, count, win_lo, win_count);
}

extern "C" int ek_pam_prefetch(ek_ctx *c, const int64_t *frames, int32_t count)
{
    return ek_pam_prefetch_frames(c, frames, count, 0, 0);
}

// Round 5: the window's proposals without a wait of their own.  The selected frames
// stay where ek_select_member_multi_kernel leaves them -- the set-up kernel reads
// them there -- and travel to the host behind it; they have arrived when the
// prefetch's own wait (the length of the list of frames within reach) is over, or
// one is made here.  Then they are checked like ek_pam_select_members_batch and
// ek_pam_prefetch do.  One wait per window less (three were two thirds of the
// ~60 us a window spends outside its kernels).
static int ek_pam_select_prefetch(ek_ctx *c, int32_t cid0, int32_t count,
                                  const int64_t *js, int32_t win_count, int64_t *frames)
{
    if (!c->cnt.batch_covers(cid0, count))
        return ek_fail(EK_ESTATE, "ek_pam_sweep: member counts of clusters [%d,+%d) "
                                  "are not the ones at hand", cid0, count);
    EK_HIP(hipSetDevice(c->device));
    int rc = ek_pam_vecs_alloc(c);
    if (rc)
        return rc;
    // (the drawn ranks are read by the selection from mapped host memory, the selected
    // frames written into it: no copy either way -- both, or neither)
    int64_t *sel_view = nullptr, *js_view = nullptr;
    rc = ek_mapped(&c->sel_host, EK_PAM_WIN, c->pam_zero_copy != 0, &sel_view);
    if (!rc && c->pam_zero_copy)
        rc = ek_mapped(&c->js_host, EK_PAM_WIN, true, &js_view);
    if (rc)
        return rc;
    if (!sel_view || !js_view)
        sel_view = js_view = nullptr;
    for (int32_t j = 0; js_view && j < count; ++j)
        c->js_host[j] = js[j];
    if (!js_view)
        EK_HIP(hipMemcpyAsync(c->bat_sel + 2 * EK_PAM_WIN, js,
                              (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice,
                              c->stream));
    ek_launch_select_member_multi(c->assign, c->n, cid0, count, c->bat_scan,
                                  js_view ? js_view : c->bat_sel + 2 * EK_PAM_WIN,
                                  c->bat_sel + EK_PAM_WIN, c->stream, sel_view);
    EK_CHECK_LAUNCH();
    if (!sel_view)
        EK_HIP(hipMemcpyAsync(c->sel_host, c->bat_sel + EK_PAM_WIN,
                              (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost,
                              c->stream));
    c->cnt.invalidate_batch();
    c->pf.invalidate();
    ek_launch_pam_setup_dev(c->aos, c->G, c->A, c->bat_sel + EK_PAM_WIN, count, c->goff,
                            c->pam_recs, c->ctile, c->ctrace, c->pam_plan, c->amb_count + 3,
                            c->stream, c->dist, c->pam_dprop);
    bool waited = false;
    rc = ek_pam_prefetch_vectors(c, count, cid0, win_count, true, true, &waited);
    if (rc)
        return rc;
    if (!waited)
        EK_HIP(ek_wait(c));
    for (int32_t j = 0; j < count; ++j) {
        frames[j] = c->sel_host[j];
        if (frames[j] < 0 || frames[j] >= c->n)
            return ek_fail(EK_EARG, "ek_pam_sweep: cluster %d has no member %lld",
                           cid0 + j, (long long)js[j]);
        c->pf.frames[j] = frames[j];
    }
    c->pf.count = count;
    c->pf.external = false;
    return EK_OK;
}

// ---- a window of proposals decided on the device --------------------------------------
// c->sp_buf: the slots' buckets | their lengths (at EK_SP_O_BCNT) | the records and lists
// of the evaluation ahead (at EK_SP_O_SPEC, ek_sp_spec_bytes() of them)
static constexpr size_t EK_SP_O_BCNT = (size_t)EK_PAM_WIN * EK_SP_CAP * sizeof(uint2);
static constexpr size_t EK_SP_O_SPEC = EK_SP_O_BCNT + 256;

// the one-workgroup window's arguments, all of them
static EkSpArgs ek_sp_args(ek_ctx *c, int32_t cid0, int32_t count, const int64_t *frames,
                           const int64_t *n_members, int32_t win_count, EkPamWin *win_host)
{
    const size_t tb = ek_pam_tab_block(c);
    EkSpArgs a = {};
    a.dist = c->dist;
    a.assign = c->assign;
    a.n = c->n;
    a.n_total = (double)c->n;
    a.A = c->A;
    a.K = c->med_K;
    a.cid0 = cid0;
    a.count = count;
    a.win_count = win_count;
    a.bucket = (const uint2 *)c->sp_buf;
    a.bcnt = (const unsigned int *)(c->sp_buf + EK_SP_O_BCNT);
    a.bcap = (int64_t)EK_SP_CAP;
    for (int32_t i = 0; i < EK_PAM_WIN; ++i) {
        a.frames[i] = i < count ? frames[i] : 0;
        a.max_amb[i] = i < count ? n_members[i] : 0;
    }
    a.O = c->dtab + tb;
    a.T = c->dtab;
    a.med_aos = c->med_aos;
    a.med_G = c->med_G;
    a.med_idx = c->med_idx;
    a.restore = c->tab.restore;
    a.frames_aos = c->aos;
    a.G = c->G;
    a.leaf = c->sq_part;
    a.chunk = c->sq_part + 2 * (size_t)c->pw_leaves;
    a.shapes = c->pw_shapes;
    a.n_full = c->pw_n_full;
    a.n_leaves = c->pw_leaves;
    a.n_chunks = c->pw_chunks;
    a.max_pairs = c->sp_max_pairs;
    a.exact_always = c->sp_exact;
    a.win = c->pam_win_dev;
    a.win_host = win_host;
    // every slot evaluated at once on the state the window opens with (not while a
    // rejected proposal's row of the medoid table is still to be put back)
    a.use_spec = (c->pam_spec && c->tab.restore < 0 && count > 1) ? 1 : 0;
    a.spec = (EkSpSpecRec *)(c->sp_buf + EK_SP_O_SPEC);
    a.spec_lists = (uint32_t *)(c->sp_buf + EK_SP_O_SPEC + EK_PAM_WIN * sizeof(EkSpSpecRec));
    a.marks = c->sp_marks;
    a.finish_later = a.use_spec;
    a.act_list = c->act_list;
    a.n_act = c->sp.n_act;
    a.n_pad = c->n_pad;
    a.vecs = c->pf.vecs.reset_there(a.finish_later, c->sp.n_act, count) ? c->pam_vecs : nullptr;
    return a;
}

#ifdef EK_SP_PROF
// measurement builds: the window kernel's 10 ns ticks per step, printed every 100 windows
static int ek_sp_prof(ek_ctx *c, EkSpArgs *a)
{
    static unsigned long long *prof_dev = nullptr;
    static unsigned long long prof_tot[16];
    static int prof_n = 0;
    if (!prof_dev) {
        EK_HIP(ek_dev_malloc((void **)&prof_dev, 16 * sizeof(unsigned long long)));
        EK_HIP(hipMemset(prof_dev, 0, 16 * sizeof(unsigned long long)));
    }
    a->prof = prof_dev;
    if (++prof_n % 100 == 0) {
        EK_HIP(ek_wait(c));
        EK_HIP(hipMemcpy(prof_tot, prof_dev, sizeof(prof_tot), hipMemcpyDeviceToHost));
        fprintf(stderr, "sp prof after %d windows (us per window): before the slots %.1f  "
                        "evaluation / take-over %.1f  apply %.1f  leaves %.1f  chunks %.1f  "
                        "total %.1f  verdict %.1f  end of slot %.1f  loop exit %.1f  after the slots %.1f\n",
                prof_n, prof_tot[8] * 1e-2 / prof_n, prof_tot[1] * 1e-2 / prof_n,
                prof_tot[2] * 1e-2 / prof_n, prof_tot[3] * 1e-2 / prof_n,
                prof_tot[4] * 1e-2 / prof_n, prof_tot[5] * 1e-2 / prof_n,
                prof_tot[6] * 1e-2 / prof_n, prof_tot[7] * 1e-2 / prof_n,
                prof_tot[0] * 1e-2 / prof_n, prof_tot[9] * 1e-2 / prof_n);
    }
    return EK_OK;
}
#endif

// The window worked through by one workgroup (ek_pam_sparse.hip): possible when the
// prefetch just made was restricted to a list of frames (still in c->amb) and the
// window's tables are in place.  Enqueues; the caller reads the window record back.
static int ek_pam_window_one_wg(ek_ctx *c, int32_t cid0, int32_t count, const int64_t *frames,
                                const int64_t *n_members, int32_t win_count, EkSpArgs *args)
{
    if (!c->sp_buf) {
        EK_HIP(ek_dev_malloc((void **)&c->sp_buf, EK_SP_O_SPEC + ek_sp_spec_bytes()));
        c->sp.bcnt_clean = false;
    }
    if (c->pam_spec && !c->sp_marks) {
        EK_HIP(ek_dev_malloc((void **)&c->sp_marks, (size_t)c->n * sizeof(unsigned long long)));
        EK_HIP(hipMemsetAsync(c->sp_marks, 0, (size_t)c->n * sizeof(unsigned long long),
                              c->stream));
    }
    // the state's cost tree, the slots' frames
    ek_launch_pw_tree(c->dist, c->assign, c->n, c->pw_shapes, c->pw_n_full,
                      c->pw_leaves, c->pw_chunks, c->sq_part, c->moved, c->stream);
    ek_launch_sp_bucket(c->act_list, c->sp.n_act, c->dist, c->assign, c->pam_vecs, c->n_pad,
                        cid0, count, (uint2 *)c->sp_buf,
                        (unsigned int *)(c->sp_buf + EK_SP_O_BCNT), (int64_t)EK_SP_CAP,
                        c->stream, c->sp.bcnt_clean);
    c->sp.bcnt_clean = false;
    EkPamWin *win_host = nullptr;
    int rc = ek_mapped(&c->pam_win_host, 1, c->pam_zero_copy != 0, &win_host);
    if (rc)
        return rc;
    EkSpArgs a = ek_sp_args(c, cid0, count, frames, n_members, win_count, win_host);
#ifdef EK_SP_PROF
    rc = ek_sp_prof(c, &a);
    if (rc)
        return rc;
#endif
    if (a.use_spec)
        ek_launch_sp_spec(a, c->stream);
    ek_launch_sp_window(a, c->stream);
    EK_CHECK_LAUNCH();
    *args = a;
    c->tab.restore = -1;
    c->sp.invalidate();
    c->pf.hits += count;
    ++c->sp.windows;
    return EK_OK;
}

// the window's arguments checked; newd[i]: slot i's prefetched vector, *max_m: the
// longest member list
static int ek_pam_window_validate(ek_ctx *c, int32_t cid0, int32_t count, const int64_t *frames,
                                  const int64_t *n_members, int32_t win_lo, int32_t win_count,
                                  bool outputs, const float **newd, int64_t *max_m)
{
    int rc = ek_pam_precheck(c, cid0, "ek_pam_window_run");
    if (rc)
        return rc;
    if (count < 1 || count > EK_PAM_WIN || cid0 + count > c->med_K || !frames || !n_members ||
        !outputs)
        return ek_fail(EK_EARG, "ek_pam_window_run: bad window [%d,+%d)", cid0, count);
    // bit i of a proposal's moved-cluster mask is cluster win_lo + i, and the
    // device reads it as slot i of this run
    if (win_lo != cid0 || win_count < count || win_count > 32)
        return ek_fail(EK_EARG, "ek_pam_window_run: the stale-mask window "
                                "[%d,+%d) must start at cid0 = %d and cover the "
                                "%d slots", win_lo, win_count, cid0, count);
    if (!c->pw_tail_ok)
        return ek_fail(EK_ESTATE, "ek_pam_window_run: the pairwise-sum shape of a "
                                  "full chunk is not the expected perfect tree");
    EK_HIP(hipSetDevice(c->device));
    *max_m = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (frames[i] < 0 || frames[i] >= c->n || n_members[i] < 0 ||
            n_members[i] > c->n)
            return ek_fail(EK_EARG, "ek_pam_window_run: slot %d: frame %lld, %lld "
                                    "members", i, (long long)frames[i],
                           (long long)n_members[i]);
        newd[i] = ek_pam_prefetched(c, frames[i]);
        if (!newd[i])
            return ek_fail(EK_ESTATE, "ek_pam_window_run: frame %lld was not "
                                      "prefetched", (long long)frames[i]);
        *max_m = std::max(*max_m, n_members[i]);
    }
    return EK_OK;
}

// one workgroup, or three launches per slot?  (a window has gone by for the wait)
static bool ek_pam_window_form(ek_ctx *c, int32_t cid0, int32_t count, const float *const *newd)
{
    const bool wait_over = c->sp.wait.over(c->sp_max_pairs);
    bool columns = true;
    for (int32_t i = 0; columns && i < count; ++i)
        columns = newd[i] == c->pam_vecs + (size_t)i * c->n_pad;
    return ek_sp_eligible(c->pam_sparse != 0, c->sp.ready,
                          ek_pam_tables_cover(c->tab.lo, c->tab.n, cid0, count),
                          ek_pam_prune_ok(c->prune, c->state_exact, c->A), c->aos != nullptr,
                          c->pw_chunks, c->pw_leaves, wait_over, columns);
}

// Three launches per slot (ek_pam_tail), every slot's enqueued at once; then the last
// slot's trial state, if accepted.
static int ek_pam_window_slots(ek_ctx *c, int32_t cid0, int32_t count, const int64_t *frames,
                               const int64_t *n_members, const float *const *newd,
                               int64_t max_m, int32_t win_count)
{
    int rc = ek_pam_amb_room(c, max_m);  // may synchronise: before anything is enqueued
    if (rc)
        return rc;
    const int K = c->med_K;
    for (int32_t i = 0; i < count; ++i) {
        const int32_t cid = cid0 + i;
        // the first proposal's trial table (and the window record: `count`
        // slots, nothing decided); the others' are set up by the last workgroup
        // of the proposal before
        if (i == 0)
            ek_launch_pam_trial(c->tiles, c->G, c->A, c->med_aos, c->med_G, K, cid,
                                c->tab.restore, frames[i], nullptr, nullptr,
                                nullptr, c->amb_count, c->moved, c->stream,
                                c->pam_win_dev, count);
        c->tab.restore = -1;
        const bool more = i + 1 < count;
        EkPamDecide dc;
        dc.win = c->pam_win_dev;
        dc.slot = i;
        dc.n_total = (double)c->n;
        dc.aos = c->med_aos;
        dc.Gm = c->med_G;
        dc.A = c->A;
        dc.K = K;
        dc.cid = cid;
        dc.med_idx = c->med_idx;
        dc.frame = frames[i];
        dc.max_amb = n_members[i];
        dc.next_cid = more ? cid + 1 : -1;
        dc.next_frame = more ? frames[i + 1] : 0;
        dc.frames_aos = c->aos;
        dc.G = c->G;
        dc.amb_count = c->amb_count;
        dc.moved = c->moved;
        rc = ek_pam_tail(c, cid, newd[i], n_members[i], cid0, win_count,
                         &c->pam_win_dev->out[i], &dc,
                         i > 0 ? &c->pam_win_dev->accept[i - 1] : &c->pam_win_dev->pad);
        if (rc)
            return rc;
        ++c->pf.hits;
    }
    // (the others were taken over by the classification of the slot after them)
    ek_launch_pam_apply(&c->pam_win_dev->accept[count - 1], c->dist, c->ndist,
                        c->assign, c->nassign, c->n, c->stream);
    EK_CHECK_LAUNCH();
    return EK_OK;
}

// The member counts of clusters next_cid0 .. +next_count, taken on the state the window
// leaves, right behind its kernels: into mapped host memory (*view) or copied back.
static int ek_pam_window_next_counts(ek_ctx *c, int32_t next_cid0, int32_t next_count,
                                     int64_t *next_counts, int64_t **view)
{
    *view = nullptr;
    if (next_count <= 0)
        return EK_OK;
    if (c->pam_zero_copy) {
        int rc = ek_mapped(&c->cnt_host, EK_PAM_WIN, true, view);
        if (rc)
            return rc;
    }
    ek_launch_count_members_multi(c->assign, c->n, next_cid0, next_count,
                                  c->bat_blockcnt, c->bat_scan, c->bat_sel, c->stream,
                                  *view);
    EK_CHECK_LAUNCH();
    if (!*view)
        EK_HIP(hipMemcpyAsync(next_counts, c->bat_sel,
                              (size_t)next_count * sizeof(int64_t),
                              hipMemcpyDeviceToHost, c->stream));
    return EK_OK;
}

// The host's one wait of a window: for the stream, or -- sp: a one-workgroup window
// whose finish kernel comes later -- for the event in front of that kernel (the accepted
// proposals' rows of the medoid table and the slots' marks: behind what the host waits
// for).
static int ek_pam_window_wait(ek_ctx *c, const EkSpArgs *sp)
{
    if (!sp || !sp->finish_later) {
        EK_HIP(ek_wait(c));
        return EK_OK;
    }
    if (!c->win_ev)
        EK_HIP(ek_event_create_flags(&c->win_ev, hipEventDisableTiming));
    EK_HIP(hipEventRecord(c->win_ev, c->stream));
    ek_launch_sp_finish(*sp, c->stream);
    EK_CHECK_LAUNCH();
    c->sp.bcnt_clean = sp->count == EK_PAM_WIN;     // (all of the lengths)
    for (;;) {
        const hipError_t e = hipEventQuery(c->win_ev);
        if (e == hipSuccess)
            return EK_OK;
        if (e != hipErrorNotReady)
            return ek_fail(EK_EHIP, "ek_pam_window_run: %s", hipGetErrorString(e));
    }
}

// The record is on the host: what it says about the context's state, then the caller's
// outputs.  sp: the window was one workgroup's.
static int ek_pam_window_account(ek_ctx *c, int32_t cid0, int32_t count, const int64_t *n_members,
                                 const EkSpArgs *sp, int32_t *n_done, int32_t *accept,
                                 double *old_cost, double *new_cost, int64_t *n_ambiguous)
{
    const EkPamWin &w = *c->pam_win_host;
    if (c->pf.vecs.finished(sp && sp->finish_later && sp->vecs, w.stop, count))
        c->pf.invalidate();
    c->tab.invalidate();
    c->pam_cid = -1;
    c->cnt.invalidate_one();
    c->pf.hits -= count - w.stop;       // the slots past the stop were not served
    if (sp) {
        c->sp.ahead += w.pad >> 8;      // slots taken over as evaluated ahead
        if (w.pad & 0xff) {             // a proposal handed back
            ++c->sp.bailed;
            c->sp.wait.handed_back();
        } else {
            c->sp.wait.clean();
        }
    }
    if (w.err)
        return ek_fail(EK_EARG, "PAM proposal: cluster %d has more members that "
                                "stay put than the %lld members declared",
                       cid0 + w.err - 1, (long long)n_members[w.err - 1]);
    *n_done = w.stop;
    for (int32_t i = 0; i < count; ++i) {
        accept[i] = i < w.stop ? w.accept[i] : 0;
        if (old_cost)
            old_cost[i] = w.out[i].sum_old / (double)c->n;
        if (new_cost)
            new_cost[i] = w.out[i].sum_new / (double)c->n;
        if (n_ambiguous)
            n_ambiguous[i] = w.out[i].n_amb;
    }
    return EK_OK;
}

// A window of proposals without a host round trip each (reference
// kmedoids.py:575-699 for clusters cid0 .. cid0 + count - 1, in order).  frames[i]
// is the frame proposed for cluster cid0 + i -- the caller drew it from the
// member list as it stood when the window was opened -- and n_members[i] that
// list's length; all of them must have been prefetched (ek_pam_prefetch_window).
// Every proposal's kernels are enqueued at once; the device decides each
// (mean of squares, float64, strict <), commits or undoes it, and stops the
// window at the first cluster whose membership an accepted proposal changed:
// *n_done slots were decided, the caller handles slot *n_done one at a time
// (its member list has to be counted again) and opens a new window after it.
// next_count > 0: the member counts of clusters next_cid0 .. +next_count (what the
// window after this one starts with) are taken on the state this window leaves,
// right behind its kernels, and come back with its record -- one wait less per
// window; they stand if the window runs to its end (the caller checks)
static int ek_pam_window_run_impl(ek_ctx *c, int32_t cid0, int32_t count, const int64_t *frames,
                                  const int64_t *n_members, int32_t win_lo, int32_t win_count,
                                  int32_t *n_done, int32_t *accept, double *old_cost,
                                  double *new_cost, int64_t *n_ambiguous, int32_t next_cid0,
                                  int32_t next_count, int64_t *next_counts)
{
    const float *newd[EK_PAM_WIN];
    int64_t max_m = 0;
    int rc = ek_pam_window_validate(c, cid0, count, frames, n_members, win_lo, win_count,
                                    n_done && accept, newd, &max_m);
    if (rc)
        return rc;
    const bool sparse = ek_pam_window_form(c, cid0, count, newd);
    EkSpArgs sp_args = {};
    const EkSpArgs *sp = sparse ? &sp_args : nullptr;
    rc = sparse ? ek_pam_window_one_wg(c, cid0, count, frames, n_members, win_count, &sp_args)
                : ek_pam_window_slots(c, cid0, count, frames, n_members, newd, max_m, win_count);
    if (rc)
        return rc;
    // (the window's kernel and the scan write their results into mapped host memory
    // themselves where they can: a copy kernel each, in the chain the host waits for)
    if (!(sp && sp->win_host))
        EK_HIP(hipMemcpyAsync(c->pam_win_host, c->pam_win_dev, sizeof(EkPamWin),
                              hipMemcpyDeviceToHost, c->stream));
    int64_t *cnt_view = nullptr;
    rc = ek_pam_window_next_counts(c, next_cid0, next_count, next_counts, &cnt_view);
    if (rc)
        return rc;
    rc = ek_pam_window_wait(c, sp);
    if (rc)
        return rc;
    c->cnt.invalidate_batch();
    for (int32_t i = 0; cnt_view && i < next_count; ++i)
        next_counts[i] = c->cnt_host[i];
    rc = ek_pam_window_account(c, cid0, count, n_members, sp, n_done, accept, old_cost,
                               new_cost, n_ambiguous);
    // the state the counts were taken on is the one the next window opens with
    if (!rc && next_count > 0 && *n_done == count)
        c->cnt.batch(next_cid0, next_count);
    return rc;
}

extern "C" int ek_pam_window_run(ek_ctx *c, int32_t cid0, int32_t count, const int64_t *frames,
                                 const int64_t *n_members, int32_t win_lo, int32_t win_count,
                                 int32_t *n_done, int32_t *accept, double *old_cost,
                                 double *new_cost, int64_t *n_ambiguous)
{
    return ek_pam_window_run_impl(c, cid0, count, frames, n_members, win_lo, win_count, n_done,
                                  accept, old_cost, new_cost, n_ambiguous, 0, 0, nullptr);
}

// ---- a whole sweep's window loop on the host side of the library ------------------------
// numpy's draws (ek_draw_at, ek_pam_policy.h), exposed for tests that hold them against
// numpy itself (no device involved): out[i] = RandomState.choice(m[i]) taken from `raw`
// at *pos on.
// -> how many were made (fewer than count: the outputs ran out, or m[i] < 1)
extern "C" int64_t ek_np_choice_draws(const uint32_t *raw, int64_t n_raw, int64_t *pos,
                                      const int64_t *m, int64_t count, int64_t *out)
{
    if (!raw || !pos || !m || !out || *pos < 0)
        return -1;
    int64_t i = 0;
    for (; i < count; ++i) {
        if (m[i] < 1 || (uint64_t)m[i] > 0x100000000ull)
            break;
        if (ek_draw_at(raw, n_raw, pos, m[i], &out[i]))
            break;
    }
    return i;
}

// what a sweep is given and gives back, cluster by cluster
struct EkSweep {
    int32_t K, width;
    const uint32_t *raw;        // the next outputs of the caller's RandomState
    int64_t n_raw, *pos;        // ... how many the draws made so far have consumed
    const int64_t *proposals;   // or the proposals themselves: nothing is drawn
    int64_t *medoids;
    int32_t *accept;
    double *old_cost, *new_cost;
    int64_t *n_amb;
    void note(int32_t cid, int a, double o, double nw, int64_t amb, int64_t frame) const
    {
        accept[cid] = a;
        old_cost[cid] = o;
        new_cost[cid] = nw;
        n_amb[cid] = amb;
        if (a)
            medoids[cid] = frame;
    }
};

// A window's proposals: the draws the real stream will produce if the counts still hold
// when each cluster's turn comes (up to the first empty cluster), or the caller's;
// selected and prefetched.  -> *n_slots of them; *status = 1: the outputs ran out
static int ek_sweep_open(ek_ctx *c, const EkSweep &s, int32_t cid, int32_t cnt,
                         const int64_t *counts, int64_t *js, int64_t *frames,
                         int32_t *n_slots, int32_t *status)
{
    int32_t n = 0;
    if (!s.proposals) {
        int64_t p = *s.pos;
        for (; n < cnt && counts[n] > 0; ++n)
            if (ek_draw_at(s.raw, s.n_raw, &p, counts[n], &js[n])) {
                *status = 1;
                return EK_OK;
            }
    } else {
        n = cnt;
        for (int32_t i = 0; i < cnt; ++i)
            frames[i] = s.proposals[cid + i];
    }
    *n_slots = n;
    int rc = EK_OK;
    // (drawn proposals are members of their clusters: see ek_pam_prefetch_restricted)
    c->pf.members = !s.proposals;
    if (!s.proposals && n > 0 && c->ctile)
        rc = ek_pam_select_prefetch(c, cid, n, js, cnt, frames);
    else {
        if (!s.proposals && n > 0)
            rc = ek_pam_select_members_batch(c, cid, n, js, frames);
        if (!rc)
            rc = ek_pam_prefetch_window(c, frames, n, cid, cnt);
    }
    c->pf.members = false;
    return rc;
}

// The cluster a window stopped at: its members changed under an accepted proposal (or
// it is empty) -- counted and drawn now, one proposal on its own.
// *status = 1: the outputs ran out; 2: the cluster has no member
static int ek_sweep_single(ek_ctx *c, const EkSweep &s, int32_t cid, int32_t *status)
{
    int64_t prop = -1, amb = 0;
    double o = 0.0, nw = 0.0;
    int rc;
    if (!s.proposals) {
        int64_t m = 0, j = 0;
        rc = ek_pam_count_members(c, cid, &m);
        if (rc)
            return rc;
        if (m <= 0) {
            *status = 2;
            return EK_OK;
        }
        if (ek_draw_at(s.raw, s.n_raw, s.pos, m, &j)) {
            *status = 1;
            return EK_OK;
        }
        rc = ek_pam_propose_member(c, cid, j, &prop, &o, &nw, &amb);
    } else {
        prop = s.proposals[cid];
        rc = ek_pam_propose(c, cid, prop, &o, &nw, &amb);
    }
    if (rc)
        return rc;
    const int a = nw < o;                               // kmedoids.py:683
    rc = ek_pam_commit(c, a);
    if (rc)
        return rc;
    s.note(cid, a, o, nw, amb, prop);
    return EK_OK;
}

// One window of the sweep, from cluster *cid on: its counts, its proposals, the run, the
// real draws behind the slots decided, the cluster it stopped at.  `ahead`: the counts
// that rode along with the window before, *have_counts: they are this window's.
static int ek_sweep_window(ek_ctx *c, const EkSweep &s, int32_t *cid_io, int64_t *ahead,
                           bool *have_counts, int32_t *status)
{
    const int32_t cid = *cid_io;
    const EkSweepWin win(cid, s.K, s.width);
    int64_t counts[EK_PAM_WIN], js[EK_PAM_WIN], frames[EK_PAM_WIN], na[EK_PAM_WIN];
    int32_t acc[EK_PAM_WIN];
    double oc[EK_PAM_WIN], nc[EK_PAM_WIN];
    int rc = EK_OK;
    if (*have_counts && c->cnt.bat_cid0 == cid && c->cnt.bat_count == win.cnt)
        std::copy(ahead, ahead + win.cnt, counts);
    else
        rc = ek_pam_count_members_batch(c, cid, win.cnt, counts);
    *have_counts = false;
    if (rc)
        return rc;
    int32_t n_slots = 0, n_done = 0;
    rc = ek_sweep_open(c, s, cid, win.cnt, counts, js, frames, &n_slots, status);
    if (rc || *status)
        return rc;
    if (n_slots > 0) {
        const int32_t ncnt = win.ride_along(n_slots, s.K, s.width);
        rc = ek_pam_window_run_impl(c, cid, n_slots, frames, counts, cid, win.cnt, &n_done,
                                    acc, oc, nc, na, win.hi, ncnt, ahead);
        if (rc)
            return rc;
        *have_counts = ek_sweep_counts_stand(ncnt, n_done, n_slots);
    }
    for (int32_t i = 0; i < n_done; ++i) {
        // the real draws, in order: the member lists are the ones the
        // guesses were drawn from, so they are the same draws
        int64_t j = -1;
        if (!s.proposals && (ek_draw_at(s.raw, s.n_raw, s.pos, counts[i], &j) || j != js[i]))
            return ek_fail(EK_ESTATE, "ek_pam_sweep: draw %lld for cluster %d, "
                                      "guessed %lld", (long long)j, cid + i,
                           (long long)js[i]);
        s.note(cid + i, acc[i], oc[i], nc[i], na[i], frames[i]);
    }
    *cid_io = cid + n_done;
    if (*cid_io < win.hi) {
        rc = ek_sweep_single(c, s, *cid_io, status);
        if (!rc && !*status)
            ++*cid_io;
    }
    return rc;
}

// The loop of kmedoids.py:575-699 over clusters *cid .. K - 1 in windows of up to
// `width` proposals decided on the device (ek_pam_window_run), the cluster a
// window stops at one proposal at a time -- what enspara_amd/cluster/kmedoids.py's
// _pam_sweep_device_on does call by call, without the interpreter between the
// calls (four read-backs per window, and as many waits for the host to come
// back).  The draws are numpy's: `raw` holds the next outputs of the caller's
// RandomState (RandomState.randint(0, 2**32, dtype=uint32)), *pos how many of
// them the draws made so far have consumed.
// *status: 0 the sweep is through (*cid == K); 1 more random outputs are needed
// (call again with a longer `raw`: *cid, *pos and the outputs so far stand);
// 2 cluster *cid has no member to draw (RandomState.choice raises there).
extern "C" int ek_pam_sweep(ek_ctx *c, int32_t K, int32_t width, const uint32_t *raw,
                            int64_t n_raw, int64_t *pos, const int64_t *proposals,
                            int32_t *cid_io, int64_t *medoids, int32_t *accept,
                            double *old_cost, double *new_cost, int64_t *n_amb,
                            int32_t *status)
{
    if (!c || !pos || !cid_io || !medoids || !accept || !old_cost || !new_cost ||
        !n_amb || !status || (!raw && n_raw > 0))
        return ek_fail(EK_EARG, "ek_pam_sweep: NULL argument");
    if (!c->ndist || c->med_K != K)
        return ek_fail(EK_ESTATE, "ek_pam_sweep: call ek_pam_begin with these %d "
                                  "medoids first", K);
    if (width < 2 || width > EK_PAM_WIN)
        return ek_fail(EK_EARG, "ek_pam_sweep: windows of 2..%d proposals", EK_PAM_WIN);
    if (*cid_io < 0 || *cid_io > K || *pos < 0)
        return ek_fail(EK_EARG, "ek_pam_sweep: cluster %d, position %lld", *cid_io,
                       (long long)*pos);
    if (n_raw > 0 && (uint64_t)c->n > 0xffffffffull)
        return ek_fail(EK_EARG, "ek_pam_sweep: member lists of 2**32 frames and more");
    const EkSweep s = {K, width, raw, n_raw, pos, proposals, medoids, accept,
                       old_cost, new_cost, n_amb};
    int64_t ahead[EK_PAM_WIN];
    bool have_counts = false;       // `ahead` holds the counts of the window at *cid_io
    *status = 0;
    int32_t cid = *cid_io;
    while (cid < K && !*status) {
        int rc = ek_sweep_window(c, s, &cid, ahead, &have_counts, status);
        if (rc)
            return rc;
    }
    *cid_io = cid;
    return EK_OK;
}


extern "C" int ek_pam_propose_ex(ek_ctx *c, int32_t cid, int64_t frame_index,
                                 int64_t n_members, int32_t win_lo,
                                 int32_t win_count, double *old_cost,
                                 double *new_cost, int64_t *n_ambiguous,
                                 uint32_t *moved_mask)
{
    int rc = ek_pam_precheck(c, cid, "ek_pam_propose_ex");
    if (rc)
        return rc;
    if (frame_index < 0 || frame_index >= c->n)
        return ek_fail(EK_EARG, "ek_pam_propose_ex: frame %lld out of range",
                       (long long)frame_index);
    if (n_members < 0 || n_members > c->n)
        return ek_fail(EK_EARG, "ek_pam_propose_ex: n_members=%lld",
                       (long long)n_members);
    if (win_count < 0 || win_count > 32 || (win_count > 0 && !moved_mask))
        return ek_fail(EK_EARG, "ek_pam_propose_ex: bad window");
    EK_HIP(hipSetDevice(c->device));
    c->cnt.invalidate_one();
    return ek_pam_propose_impl(c, cid, frame_index, n_members, nullptr, old_cost,
                               new_cost, n_ambiguous, win_lo, win_count,
                               win_count > 0 ? moved_mask : nullptr);
}

static int ek_pam_prefetch_centers_impl(ek_ctx *c, const float *aos_dev,
                                        const double *G_dev, int32_t count,
                                        int32_t win_lo, int32_t win_count)
{
    if (!c || (count > 0 && (!aos_dev || !G_dev)))
        return ek_fail(EK_EARG, "ek_pam_prefetch_centers: NULL argument");
    if (!c->ndist || c->med_K < 1)
        return ek_fail(EK_ESTATE, "ek_pam_prefetch_centers: call ek_pam_begin[_table] "
                                  "first");
    if (count < 0 || count > EK_PAM_GROUP)
        return ek_fail(EK_EARG, "ek_pam_prefetch_centers: count=%d outside [0,%d]",
                       count, EK_PAM_GROUP);
    EK_HIP(hipSetDevice(c->device));
    c->pf.invalidate();
    c->pf.external = true;
    if (count == 0)
        return EK_OK;
    int rc = ek_pam_vecs_alloc(c);
    if (rc)
        return rc;
    const size_t rstride = ek_rec_bytes(c->A);
    for (int32_t j = 0; j < count; ++j)
        ek_launch_record_from_center(aos_dev + (size_t)j * 3 * c->A, G_dev + j, c->A,
                                     c->pam_recs + j * rstride, c->stream);
    rc = ek_pam_prefetch_vectors(c, count, win_lo, win_count, false);
    if (rc)
        return rc;
    for (int32_t j = 0; j < count; ++j)
        c->pf.frames[j] = -1;
    c->pf.count = count;
    return EK_OK;
}

extern "C" int ek_pam_prefetch_centers(ek_ctx *c, const float *aos_dev,
                                       const double *G_dev, int32_t count)
{
    return ek_pam_prefetch_centers_impl(c, aos_dev, G_dev, count, 0, 0);
}

extern "C" int ek_pam_prefetch_centers_window(ek_ctx *c, const float *aos_dev,
                                              const double *G_dev, int32_t count,
                                              int32_t win_lo, int32_t win_count)
{
    if (c && (win_lo < 0 || win_count < 0 || win_lo + win_count > c->med_K))
        return ek_fail(EK_EARG, "ek_pam_prefetch_centers_window: clusters [%d,+%d) "
                                "outside [0,%d)", win_lo, win_count, c->med_K);
    return ek_pam_prefetch_centers_impl(c, aos_dev, G_dev, count, win_lo, win_count);
}

extern "C" int ek_pam_propose_center(ek_ctx *c, int32_t cid, int32_t slot,
                                     const float *center_aos_dev,
                                     const double *center_G_dev,
                                     int64_t n_members_local, int32_t win_lo,
                                     int32_t win_count, void *out_dev)
{
    int rc = ek_pam_precheck(c, cid, "ek_pam_propose_center");
    if (rc)
        return rc;
    if (!center_aos_dev || !center_G_dev || !out_dev)
        return ek_fail(EK_EARG, "ek_pam_propose_center: NULL argument");
    if (n_members_local < 0 || n_members_local > c->n)
        return ek_fail(EK_EARG, "ek_pam_propose_center: n_members_local=%lld",
                       (long long)n_members_local);
    if (win_count < 0 || win_count > 32)
        return ek_fail(EK_EARG, "ek_pam_propose_center: bad window");
    if (slot >= 0 && (!c->pf.external || slot >= c->pf.count))
        return ek_fail(EK_ESTATE, "ek_pam_propose_center: slot %d was not "
                                  "prefetched", slot);
    EK_HIP(hipSetDevice(c->device));
    c->cnt.invalidate_one();
    rc = ek_pam_amb_room(c, n_members_local);
    if (rc)
        return rc;
    const int K = c->med_K;
    const float *newd;
    if (slot >= 0) {
        newd = c->pam_vecs + (size_t)slot * c->n_pad;
        ++c->pf.hits;
    } else {
        ek_launch_record_from_center(center_aos_dev, center_G_dev, c->A, c->rec_tmp,
                                     c->stream);
        ek_launch_step(ek_pick_fpl(c), 1, ek_pick_nt(c), c->tiles, c->G, c->dist,
                       c->assign, c->scratch, c->rec_tmp, 1, c->n, c->A, 0, 0.0,
                       c->blockmax, c->hist, c->ctl, c->stream);
        EK_CHECK_LAUNCH();
        newd = c->scratch;
        ++c->pf.misses;
    }
    ek_launch_pam_trial(c->tiles, c->G, c->A, c->med_aos, c->med_G, K, cid,
                        c->tab.restore, -1, nullptr, center_aos_dev, center_G_dev,
                        c->amb_count, c->moved, c->stream);
    c->tab.restore = -1;
    rc = ek_pam_tail(c, cid, newd, n_members_local, win_lo, win_count,
                     (EkPamOut *)out_dev);
    if (rc)
        return rc;
    c->pam_cid = cid;
    c->pam_frame = -1;
    return EK_OK;
}

extern "C" int ek_pam_prefetch_passes(ek_ctx *c, int64_t *restricted,
                                      int64_t *full)
{
    if (!c)
        return ek_fail(EK_EARG, "NULL context");
    if (restricted)
        *restricted = c->pf.restricted;
    if (full)
        *full = c->pf.full;
    return EK_OK;
}

extern "C" int ek_pam_sparse_stats(ek_ctx *c, int64_t *windows, int64_t *ended_early)
{
    if (!c)
        return ek_fail(EK_EARG, "NULL context");
    if (windows)
        *windows = c->sp.windows;
    if (ended_early)
        *ended_early = c->sp.bailed;
    return EK_OK;
}

extern "C" int ek_pam_ahead_stats(ek_ctx *c, int64_t *slots_taken_over)
{
    if (!c)
        return ek_fail(EK_EARG, "NULL context");
    if (slots_taken_over)
        *slots_taken_over = c->sp.ahead;
    return EK_OK;
}

extern "C" int ek_pam_prefetch_stats(ek_ctx *c, int64_t *hits, int64_t *misses)
{
    if (!c)
        return ek_fail(EK_EARG, "NULL context");
    if (hits)
        *hits = c->pf.hits;
    if (misses)
        *misses = c->pf.misses;
    return EK_OK;
}


// ---- the window's distance kernels on the caller's arrays (tests) -----------------------
// The shipped launchers ek_launch_pam_tables / ek_launch_pam_list_dist on host arrays:
// rows [n_rows][3A] (centred) with their traces, columns [n_col][3A] made into records
// here.  list == NULL: the tables of a window (rows: the medoid table [K + 1], row K the
// held medoid); else the listed rows against the columns.  Every output array is copied
// in before the launch and out after it, so the caller's prefill shows what no kernel
// wrote.  One device allocation; the form of the pairs kernels is the caller's for the
// length of the call.
extern "C" int ek_pam_pairs_probe(int device, int32_t form, int32_t n_atoms,
                                  const float *rows, const double *rows_G, int64_t n_rows,
                                  const float *cols, const double *cols_G, int32_t n_col,
                                  int32_t K, int32_t held, int32_t old_lo, int32_t n_old,
                                  const float *dprop, float *T, float *O, float *dmin,
                                  const uint32_t *list, int64_t n_list, int64_t n_pad,
                                  float *vecs)
{
    const int A = n_atoms;
    if (!rows || !rows_G || n_rows < 1 || n_rows > ((int64_t)1 << 24) || A < 1 ||
        A > EK_MAX_ATOMS || n_col < 0 || n_col > EK_PAM_WIN || (n_col > 0 && (!cols || !cols_G)))
        return ek_fail(EK_EARG, "ek_pam_pairs_probe: bad argument");
    const bool tables = list == nullptr;
    int n_grp = 0;      // groups of EK_PAM_GROUP columns dmin has
    if (tables) {
        if (K < 1 || n_rows != (int64_t)K + 1 || held < -1 || held >= K || old_lo < 0 ||
            n_old < 0 || n_old > EK_PAM_WIN || old_lo + n_old > K || n_col + n_old < 1 ||
            (dprop && (n_old != n_col || n_col < 1)) || (n_col > 0 && (!T || !dmin)) ||
            (n_old > 0 && !O))
            return ek_fail(EK_EARG, "ek_pam_pairs_probe: tables: K=%d held=%d old=[%d,+%d) "
                                    "n_col=%d", K, held, old_lo, n_old, n_col);
        n_grp = (n_col + EK_PAM_GROUP - 1) / EK_PAM_GROUP;
    } else {
        if (n_list < 1 || n_list > ((int64_t)1 << 24) || n_col < 1 || n_pad < n_rows ||
            n_pad > ((int64_t)1 << 24) || !vecs)
            return ek_fail(EK_EARG, "ek_pam_pairs_probe: list: n_list=%lld n_pad=%lld "
                                    "n_col=%d", (long long)n_list, (long long)n_pad, n_col);
        for (int64_t i = 0; i < n_list; ++i)
            if ((int64_t)list[i] >= n_rows)
                return ek_fail(EK_EARG, "ek_pam_pairs_probe: list[%lld]=%u outside the %lld "
                                        "rows", (long long)i, list[i], (long long)n_rows);
    }
    // the columns as records
    const size_t rstride = ek_rec_bytes(A);
    std::vector<unsigned char> recs((size_t)std::max(n_col, 1) * rstride, 0);
    for (int j = 0; j < n_col; ++j) {
        EkRecHdr h = {};
        h.valid = 1;
        h.gidx = j;
        h.trace = cols_G[j];
        memcpy(recs.data() + (size_t)j * rstride, &h, sizeof(h));
        memcpy(recs.data() + (size_t)j * rstride + sizeof(h), cols + (size_t)j * 3 * A,
               (size_t)12 * A);
    }
    EK_HIP(hipSetDevice(device));
    // traces | records | rows | list | dprop | T | O | dmin | vecs, each at a multiple of 16
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t b_G = (size_t)n_rows * 8, b_recs = recs.size(),
                 b_rows = (size_t)n_rows * 12 * A,
                 b_list = tables ? 0 : (size_t)n_list * 4,
                 b_dprop = (tables && dprop) ? (size_t)n_col * 4 : 0,
                 b_T = tables ? (size_t)n_col * K * 4 : 0,
                 b_O = tables ? (size_t)n_old * K * 4 : 0,
                 b_dmin = tables ? (size_t)n_grp * K * 4 : 0,
                 b_vecs = tables ? 0 : (size_t)n_col * (size_t)n_pad * 4;
    const size_t off_G = 0, off_recs = off_G + up16(b_G), off_rows = off_recs + up16(b_recs),
                 off_list = off_rows + up16(b_rows), off_dprop = off_list + up16(b_list),
                 off_T = off_dprop + up16(b_dprop), off_O = off_T + up16(b_T),
                 off_dmin = off_O + up16(b_O), off_vecs = off_dmin + up16(b_dmin),
                 total = off_vecs + up16(b_vecs);
    unsigned char *buf = nullptr;
    EK_HIP(ek_dev_malloc((void **)&buf, total));
    struct Piece {
        void *host;
        size_t off, bytes;
        bool in, out;
    };
    const Piece pieces[] = {
        {(void *)rows_G, off_G, b_G, true, false},
        {(void *)recs.data(), off_recs, b_recs, true, false},
        {(void *)rows, off_rows, b_rows, true, false},
        {(void *)list, off_list, b_list, true, false},
        {(void *)dprop, off_dprop, b_dprop, true, false},
        {(void *)T, off_T, b_T, true, true},
        {(void *)O, off_O, b_O, true, true},
        {(void *)dmin, off_dmin, b_dmin, true, true},
        {(void *)vecs, off_vecs, b_vecs, true, true},
    };
    hipError_t e = hipSuccess;
    for (const Piece &q : pieces)
        if (e == hipSuccess && q.in && q.bytes > 0)
            e = hipMemcpy(buf + q.off, q.host, q.bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const int saved = ek_pam_pairs_form;
        ek_pam_pairs_form = form ? 1 : 0;
        if (tables)
            ek_launch_pam_tables((const float *)(buf + off_rows), (const double *)(buf + off_G),
                                 A, K, held, buf + off_recs, n_col, old_lo, n_old,
                                 (float *)(buf + off_T), (float *)(buf + off_O),
                                 (float *)(buf + off_dmin), 0,
                                 dprop ? (const float *)(buf + off_dprop) : nullptr);
        else
            ek_launch_pam_list_dist((const float *)(buf + off_rows),
                                    (const double *)(buf + off_G), A,
                                    (const uint32_t *)(buf + off_list), n_list,
                                    buf + off_recs, n_col, (float *)(buf + off_vecs), n_pad, 0);
        ek_pam_pairs_form = saved;
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    for (const Piece &q : pieces)
        if (e == hipSuccess && q.out && q.bytes > 0)
            e = hipMemcpy(q.host, buf + q.off, q.bytes, hipMemcpyDeviceToHost);
    (void)ek_dev_free(buf);
    if (e != hipSuccess)
        return ek_fail(EK_EHIP, "ek_pam_pairs_probe: %s", hipGetErrorString(e));
    return EK_OK;
}
