/*
 * enspara_hip.h -- C ABI of the MI355X (gfx950) k-centers / RMSD hot path.
 *
 * Drop-in boundary.  The reference (bowman-lab/enspara) has no FFI for this
 * path: its plug-in point is a Python callable `metric(X, y) -> distances`
 * (enspara/cluster/kcenters.py:132-137, resolved from the string 'rmsd' to
 * mdtraj.rmsd at enspara/cluster/util.py:289-291), driven by pure-Python /
 * numpy loops.  This header is the binding a maintainer would add underneath
 * those loops (INTEGRATION.md shows the ctypes stub).  Each entry point cites
 * the reference code it replaces.  Paths are relative to /root/reference.
 *
 * Conventions
 *   - every function returns 0 on success, a negative EK_E* code otherwise;
 *     ek_last_error() returns a thread-local human readable message;
 *   - plain pointers and sizes only; "host" pointers are ordinary memory,
 *     "dev" pointers are HIP device memory of the context's device;
 *   - a context owns one shard of frames resident in HBM, its k-centers state
 *     (float32 distance and int32 assignment per frame) and one HIP stream;
 *     all work is enqueued on that stream; functions that return data to host
 *     memory synchronise the stream, the others do not;
 *   - a context is not thread-safe; different contexts are independent.
 *
 * Data layout in HBM: centred coordinates in tiles of
 * EK_TILE frames, frame-minor: element (frame f, atom a, axis k) lives at
 * float index ((f / EK_TILE) * 3A + 3a + k) * EK_TILE + f % EK_TILE.
 */
#ifndef ENSPARA_HIP_H
#define ENSPARA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EK_ABI_VERSION 1
#define EK_TILE 256

#define EK_OK 0
#define EK_EARG (-1)     /* bad argument */
#define EK_EHIP (-2)     /* HIP runtime error (message has the hipError_t) */
#define EK_ESTATE (-3)   /* call sequence error (e.g. frames not loaded) */
#define EK_ENOMEM (-4)

typedef struct ek_ctx ek_ctx;

int ek_abi_version(void);
const char *ek_last_error(void);
/* number of visible HIP devices, or a negative error */
int ek_device_count(void);

/* ---- context ----------------------------------------------------------- */
/* n_frames frames of n_atoms atoms will live on `device`.  `global_offset`
 * is the index of this shard's first frame in the whole data set (0 on one
 * GPU); candidate records carry global indices.  `stream` is a hipStream_t to
 * enqueue on (e.g. torch.cuda.current_stream().cuda_stream) or NULL to let
 * the context create its own. */
int ek_ctx_create(int device, int64_t n_frames, int32_t n_atoms,
                  int64_t global_offset, void *stream, ek_ctx **out);
int ek_ctx_destroy(ek_ctx *ctx);
int ek_ctx_sync(ek_ctx *ctx);
/* the hipStream_t the context enqueues on */
void *ek_ctx_stream(ek_ctx *ctx);

/* ---- loading frames ---------------------------------------------------- */
/* Replaces the per-call centring mdtraj.rmsd does (precentered=False) and
 * the md.Trajectory.center_coordinates() enspara does once before
 * reassignment (enspara/cluster/util.py:624-629).
 * xyz: float32 [count][n_atoms][3] (the md.Trajectory.xyz layout,
 * enspara/util/load.py:211-216), host or device memory.  Frames
 * [first, first+count) of the shard are centred (float64 mean), their traces
 * computed, and stored frame-minor.  `first` must be a multiple of EK_TILE
 * unless it is 0.
 * Host memory (any: pageable numpy arrays) goes through two pinned buffers of
 * <= 256 MiB filled by a few host threads and a DMA behind each (16 -> 45 GB/s
 * measured; EK_UPLOAD_THREADS, EK_UPLOAD_CHUNK_MB).  On return the caller's
 * array has been read completely; the centring / layout kernels may still be
 * running on the context's stream, where everything that follows is ordered
 * behind them (ek_ctx_sync to wait). */
int ek_load_frames(ek_ctx *ctx, const float *xyz, int64_t first,
                   int64_t count, int src_is_device);

/* ---- metric parity: one center vs all frames --------------------------- */
/* Replaces `distance_method(traj, new_center)` (kcenters.py:298,
 * kmedoids.py:637) for metric 'rmsd'.  The center is either frame
 * `frame_index` of this shard (>= 0) or, if frame_index < 0, the float32
 * [n_atoms][3] host coordinates `center_xyz` (centred here).  Writes float32
 * [n_frames] RMSDs to out_host.  Does not touch the k-centers state. */
int ek_rmsd_to_center(ek_ctx *ctx, int64_t frame_index,
                      const float *center_xyz, float *out_host);

/* ---- k-centers state ---------------------------------------------------- */
/* kcenters.py:198-199: assignments = -1, distances = +inf */
int ek_state_reset(ek_ctx *ctx);
/* float32 distances / int32 assignments, [n_frames] each, host memory */
int ek_state_download(ek_ctx *ctx, float *dist_host, int32_t *assign_host);
int ek_state_upload(ek_ctx *ctx, const float *dist_host,
                    const int32_t *assign_host);

/* ---- candidate records --------------------------------------------------
 * A record describes a shard's farthest frame: what one rank contributes to
 * the exchange of kcenters.py:332-348 (two allgathers + Bcast of the frame)
 * folded into one message.  Layout (little endian):
 *   float  maxdist;  int32 valid;  int64 global_index;  double trace;
 *   int64  reserved;  float centred_xyz[3 * n_atoms];   padded to 16 bytes.
 */
size_t ek_record_bytes(int32_t n_atoms);
/* Reduce the shard's distances to (max, first index) -- np.argmax semantics,
 * kcenters.py:282 -- gather that frame, write the record to rec_dev (device
 * memory, ek_record_bytes long; NULL = the context's own slot). */
int ek_local_candidate(ek_ctx *ctx, void *rec_dev);
/* device address of the context's own record slot */
void *ek_own_record(ek_ctx *ctx);

/* One k-centers iteration on this shard (kcenters.py:243-311; the MPI
 * variant :314-378): pick the winning record among n_recs contiguous records
 * at recs_dev (largest maxdist, lowest position on ties = lowest rank,
 * kcenters.py:337); if winner.maxdist <= dist_cutoff (stop rule,
 * kcenters.py:217) do nothing; otherwise distance pass against the winner's
 * frame, strict-< update of distances/assignments with `label`
 * (kcenters.py:304-306), history[label] = winner, then refresh the context's
 * own record (as ek_local_candidate(ctx, own_rec_out)).  recs_dev == NULL
 * means "the context's own record" (single shard).  own_rec_out == NULL means
 * the context's own slot.  Entirely asynchronous. */
int ek_kcenters_step(ek_ctx *ctx, const void *recs_dev, int32_t n_recs,
                     int32_t label, double dist_cutoff, void *own_rec_out);

/* Single-shard driver: the whole loop of kcenters.py:217-231 on the device.
 * Starts at label `first_label`, adds at most `max_new` centers, stops early
 * when the maximum distance is <= dist_cutoff.  Returns the number of centers
 * added in *n_added, their frame indices in center_index_out[0..n_added) and
 * the distance each had to its nearest earlier center in
 * center_dist_out[0..n_added) (either may be NULL).  *final_maxdist receives
 * distances.max() after the last update (kcenters.py:226). */
int ek_kcenters_run(ek_ctx *ctx, int32_t first_label, int32_t max_new,
                    double dist_cutoff, int32_t *n_added,
                    int64_t *center_index_out, float *center_dist_out,
                    float *final_maxdist);

/* ---- several candidate centers per pass ("speculative" rounds) ------------------
 * The same sequential algorithm (identical centers, labels, distances) with
 * the frames streamed once per ROUND against T candidates (DESIGN.md
 * section 4a).  ek_kcenters_run uses it on one shard automatically.  Across
 * shards the caller moves two kinds of messages:
 *   per round:   T candidate records per rank (T * ek_record_bytes, T =
 *                ek_spec_candidates) -> all-gather -> ek_spec_round
 *   per center:  one 16-byte header {float maxdist; int32 valid; int64 global
 *                index} per rank (ek_spec_localmax) -> all-gather ->
 *                ek_spec_apply, T-1 times per round
 * ek_spec_begin(first_label, limit): accept centers first_label..limit-1, then
 * make every further call a no-op; writes this shard's first T records.
 * ek_spec_round_end writes the records for the next round.  ek_spec_progress
 * synchronises and reports how many centers exist and whether the stop rule
 * (maximum distance <= dist_cutoff, kcenters.py:217) fired. */
int ek_spec_candidates(ek_ctx *ctx);
/* the widest round ek_kcenters_run / ek_ms_run may use (option key 4; 16 by
 * default, 32 on request): ek_spec_candidates is the same for the ek_spec_*
 * protocol (<= 16) */
int ek_round_candidates(ek_ctx *ctx);
/* Rounds of 16 / 32 candidates stream a third copy of the frames (the quad copy,
 * 12 * n_atoms bytes per frame), made when first needed.  1: it exists or could
 * be made now; 0: no memory for it (a single shard then runs rounds of 8 on its
 * own).  Shards of a GROUP must all run the same form: the multi-shard entry
 * points (ek_ms_*, ek_spec_*) never narrow their rounds on their own -- they fail
 * with EK_ENOMEM -- and the caller agrees on the form first: every rank asks
 * this, and if any says 0 all set option key 4 to 8 (sharded.kcenters_sharded). */
int ek_quad_copy_ready(ek_ctx *ctx);
int ek_spec_begin(ek_ctx *ctx, int32_t first_label, int32_t limit,
                  void *recs_out);
int ek_spec_round(ek_ctx *ctx, const void *recs_all, int32_t n_recs,
                  double dist_cutoff);
int ek_spec_localmax(ek_ctx *ctx, void *hdr_out);
int ek_spec_apply(ek_ctx *ctx, const void *hdrs_all, int32_t n_hdrs,
                  double dist_cutoff);
int ek_spec_round_end(ek_ctx *ctx, void *recs_out);
int ek_spec_progress(ek_ctx *ctx, int32_t *n_done, int32_t *stopped);
/*
 * The cheap steps of a round can also be taken all at once ("chained",
 * csrc/ek_chain.hip): between ek_spec_round and ek_spec_round_end, instead of
 * up to T-1 times (ek_spec_localmax, all-gather, ek_spec_apply),
 *   ek_spec_chain_rows(ctx, my_rows)      this shard's view of the candidate
 *                                         frames it owns: current distance and
 *                                         distance to every candidate
 *   all-gather my_rows -> all_rows        (rows_bytes per shard)
 *   ek_spec_chain_max(ctx, all_rows, n_shards, my_hdrs)
 *                                         the order in which the candidates
 *                                         would be accepted, and this shard's
 *                                         (max distance, global index) of the
 *                                         state each prefix of it would leave
 *   all-gather my_hdrs -> all_hdrs        (hdrs_bytes per shard)
 *   ek_spec_chain_apply(ctx, all_hdrs, n_shards, dist_cutoff)
 *                                         accept the longest prefix whose every
 *                                         member is the farthest point when its
 *                                         turn comes, and apply it
 * -- two exchanges per round instead of one per accepted center, same centers,
 * labels and distances.  Buffers are device memory; ek_spec_chain_bytes gives
 * their per-shard sizes (320 and 128 bytes). */
int ek_spec_chain_bytes(int32_t *rows_bytes, int32_t *hdrs_bytes);
int ek_spec_chain_rows(ek_ctx *ctx, void *rows_out);
int ek_spec_chain_max(ek_ctx *ctx, const void *rows_all, int32_t n_shards,
                      void *hdrs_out);
int ek_spec_chain_apply(ek_ctx *ctx, const void *hdrs_all, int32_t n_shards,
                        double dist_cutoff);
/* ---- rounds across shards with ONE exchange per round (csrc/ek_mshard.hip) -------
 * Replaces, per ROUND of up to 16 candidates (~15 accepted centers), what the
 * reference's MPI iteration moves per CENTER: two pickled allgathers
 * (kcenters.py:332-335), the owner's frame (mpi/ops.py:169-212) and the
 * allreduce of the stop test (mpi/ops.py:128-140).  A shard's message holds its
 * (max distance, global index) in the state every prefix of the round's chain
 * would leave and its farthest frames of the state the whole chain would leave
 * (16 + 32 * 16 + offer * ek_record_bytes bytes, offer = min(64, 128 / world)).  Results are
 * those of the single-shard run bit for bit: every accepted center is the
 * global first-index arg-max of the state before it (lowest rank on ties,
 * kcenters.py:337).
 *
 *   ek_ms_setup(ctx, world, rank, &message_bytes)      once per group
 * Exchange by the caller (any all-gather: RCCL, gloo):
 *   ek_ms_begin(ctx, first_label, limit)
 *   repeat:  ek_ms_local(ctx, cutoff, my_message)       pass + chain -> message
 *            all-gather my_message -> all_messages      (message_bytes per shard)
 *            ek_ms_global(ctx, cutoff, all_messages)    decision + next plan
 *            (ek_spec_progress now and then; calls past the end are no-ops)
 *   ek_ms_end(ctx)                                      pending chain applied
 * Exchange on the device (peer mailboxes, no host and no collective in a
 * round): every shard publishes its mailbox (ek_ms_mailbox: addresses for
 * contexts of one process, hipIpc handles of 64 bytes each across processes),
 * connects every shard's including its own (ek_ms_connect), then
 *   ek_ms_run(ctx, first_label, max_new, cutoff, ...)   as ek_kcenters_run
 * on every shard at the same time.  A message that does not arrive within 10 s
 * (of the device's constant 100 MHz clock) is reported as an error (a peer
 * died), not waited for.  With the default option key 4 = -1 the run moves
 * between rounds of 8 and 16 (with key 4 = 32: and 32) candidates by the centers the rounds of a batch
 * accepted -- numbers every shard sees alike, so every shard takes the same
 * decision at the same round; ek_run_stats reports the mix.  A round of 32 is
 * two passes of 16 over the frames behind ONE plan, chain and exchange (the
 * message carries EK_MAX_CANDS = 32 per-prefix headers).  ek_ms_begin's loop
 * (exchange by the caller) runs one form: 16 unless key 4 names another. */
int ek_ms_setup(ek_ctx *ctx, int32_t world, int32_t rank, size_t *message_bytes);
int ek_ms_mailbox(ek_ctx *ctx, void **mbox, void **flags, void *ipc_mbox,
                  void *ipc_flags);
int ek_ms_connect(ek_ctx *ctx, int32_t peer, void *mbox, void *flags,
                  const void *ipc_mbox, const void *ipc_flags);
/* Allocates, NOW, everything a run of the rounds to n_centers centers needs (the
 * accepted centers' history, the rounds' working set, the third copy of the
 * frames for rounds of 16): an allocation inside ek_ms_run waits for the whole
 * device, and with peers already polling for this shard's message on the same
 * GPU that is a deadlock until the mailbox time-out.  Call it on every shard
 * before the first of them enters ek_ms_run.  No reference counterpart. */
int ek_reserve_centers(ek_ctx *ctx, int32_t n_centers);
int ek_ms_begin(ek_ctx *ctx, int32_t first_label, int32_t limit);
int ek_ms_local(ek_ctx *ctx, double dist_cutoff, void *message_out);
int ek_ms_global(ek_ctx *ctx, double dist_cutoff, const void *messages_all);
int ek_ms_end(ek_ctx *ctx);
/* What the last ek_ms_run spent where -- counts[5]: exchanges, exchanges without a
 * pass (a broken chain offered again), 10 ns ticks waited for the peers' messages
 * (per exchange the longest wait), ... for the shard's own flag (the floor),
 * rounds sampled; ms[3]: mean milliseconds of a sampled round's pass, chain
 * kernel (the exchange's wait inside) and plan kernels.  No reference counterpart
 * (its MPI iteration, kcenters.py:314-378, is not instrumented). */
int ek_ms_diag(ek_ctx *ctx, int64_t *counts, double *ms);
/* mode (0: the run is over), exchanges completed since ek_ms_setup, error */
int ek_ms_state(ek_ctx *ctx, int32_t *mode, int32_t *exchanges, int32_t *err);
int ek_ms_run(ek_ctx *ctx, int32_t first_label, int32_t max_new,
              double dist_cutoff, int32_t *n_added, int64_t *center_index_out,
              float *center_dist_out, float *final_maxdist);
/* rounds (passes over the frames) that really ran since ek_spec_begin /
 * ek_kcenters_run started */
int ek_spec_rounds(ek_ctx *ctx, int32_t *rounds);
/* How the last ek_kcenters_run / ek_ms_run spent its rounds:
 * passes[i] / centers[i] = rounds run with 1, 4, 8, 16, 32 candidate centers
 * (i = 0 .. 4: both arrays hold FIVE entries since round 5) and the centers
 * those rounds accepted.  A round of 32 streams the frames twice (two passes of
 * 16 behind one plan, one chain and one exchange); every other form once.  The loop of
 * kcenters.py:217-231 has no such notion (one metric call per center); the
 * forms give identical centers, labels and distances, and the run moves
 * between them by the centers per millisecond each achieves. */
int ek_run_stats(ek_ctx *ctx, int64_t *passes, int64_t *centers);
/* Triangle inequality (ek_set_option key 11; the reference's
 * `use_triangle_inequality`, kcenters.py:287-296 / :351-364): how many
 * (center, tile of 256 frames) pairs the last ek_kcenters_run looked at and
 * how many of them it did not have to read because no frame of the tile could
 * come closer to the new center than it is to its own. */
int ek_ti_stats(ek_ctx *ctx, int64_t *tiles, int64_t *skipped);
/* Active view (EK_OPT_ACTIVE_VIEW) of the last ek_kcenters_run: stats[0] views built,
 * [1] frames x rounds streamed, [2] frames x rounds left out, [3] views ended by
 * their guard (the maximum fell to it before the run stopped). */
int ek_view_stats(ek_ctx *ctx, int64_t *stats);
/* Which form the last ek_kcenters_run took where the kernels change form with the number
 * of frames.  Read-only: no launch, no allocation.  out[6], all for the shard's whole
 * store (an active view has frame counts of its own) and the widest form of the run:
 *   [0] frames per lane of the one-center step kernel (1, 2, 4; automatic from 524 161
 *       and 1 048 321 frames)
 *   [1] non-temporal frame loads, 0 / 1
 *   [2] rounds of 16 take the per-prefix maxima in the pass, 0 / 1 (EK_OPT_PASS_SWEEP;
 *       automatic up to 524 288 frames; always 0 unless the widest form is 16 in fused
 *       rounds)
 *   [3] the candidate pick reads maxima per 64 frames, 0 / 1 (EK_OPT_FINE_PICK, fused
 *       rounds, up to 524 288 frames)
 *   [4] entries of the coarse list: blocks of 256 frames
 *   [5] entries of the longest list the pick reads: 4 x [4] with [3] on, [4] in other
 *       rounds, the step kernel's workgroups (256 x [0] frames each) where the run takes
 *       one center per pass only
 * All zero before the first run.  No reference counterpart. */
int ek_last_run_form(ek_ctx *ctx, int64_t *out);
/* TEST entry.  Selects the frames whose distance is above theta, builds their view as a
 * rebuild does (into buffers filled with 0xFF bytes; the frame-minor tiles on demand
 * from the quad copy where the context has one) and, in scratch of its own, the same
 * layouts by the earlier path (gather -> frame-minor tiles -> quad copy), and
 * compares on the device word for word: out[0] frames in the view, out[1] words of the
 * quad copy that differ (whole tiles, padding included; 0 without a quad copy), out[2]
 * words of the frame-minor tiles, out[3] words of the traces, distances and labels of
 * the live frames (a view holds no frame-major copy).  Not during a run; the run state
 * is left as it was. */
int ek_view_layout_check(ek_ctx *ctx, float theta, int64_t *out);

/* history written by ek_kcenters_step: for labels [first, first+count) the
 * global frame index and pre-update distance of each accepted center;
 * *n_done = 1 + the highest label accepted so far (0 if none). */
int ek_history_download(ek_ctx *ctx, int32_t first, int32_t count,
                        int64_t *center_index_out, float *center_dist_out,
                        int32_t *n_done);
int ek_history_reset(ek_ctx *ctx);

/* ---- nearest-center assignment ----------------------------------------- */
/* Replaces assign_to_nearest_center (enspara/cluster/util.py:159-205,
 * center-major branch :199-203; strict <, lowest center index wins ties,
 * assignments start at 0) for metric 'rmsd': centers_xyz is float32
 * [n_centers][n_atoms][3] host memory.  Overwrites the context's k-centers
 * state with the result (so predict / warm start / reassign read it back
 * with ek_state_download). */
int ek_assign_nearest(ek_ctx *ctx, const float *centers_xyz,
                      int32_t n_centers);

/* ---- PAM (k-medoids) proposals ------------------------------------------------
 * Replace the O(n) passes of one proposal of _kmedoids_pam_update
 * (enspara/cluster/kmedoids.py:610-690) for metric 'rmsd'.  The host keeps the
 * random stream (RandomState.choice, :514) and the accept test (:683).
 *
 * ek_pam_begin: medoid_frames[K] are the current medoids (frame indices of
 * this shard, :607); builds the device-side medoid table.  The k-centers
 * state (distances / assignments) must already be consistent with them.
 * ek_pam_count_members: len(where(assignments == cid)) (:611).
 * ek_pam_select_member: the j-th such frame in ascending order, so that
 * `state_inds[random_state.choice(len(state_inds))]` == the reference's
 * `random_state.choice(state_inds)`; call right after count_members(cid).
 * ek_pam_propose: distances to frame `frame_index` (:637), the three masks
 * (:644-658), nearest-medoid search for the ambiguous frames against the
 * trial medoid set (:666), and both costs mean(d^2) in float64 (:478,
 * :680-681).  The new state is held aside until
 * ek_pam_commit(accept != 0): adopt it (:687-689); accept == 0: drop it. */
int ek_pam_begin(ek_ctx *ctx, const int64_t *medoid_frames, int32_t n_medoids);
int ek_pam_count_members(ek_ctx *ctx, int32_t cid, int64_t *count);
int ek_pam_select_member(ek_ctx *ctx, int32_t cid, int64_t j,
                         int64_t *frame_index);
int ek_pam_propose(ek_ctx *ctx, int32_t cid, int64_t frame_index,
                   double *old_cost, double *new_cost, int64_t *n_ambiguous);
/* ek_pam_select_member + ek_pam_propose in one call (the selected frame index
 * never leaves the device before the final read-back): propose the j-th member
 * of cluster cid; needs ek_pam_count_members(cid) immediately before. */
int ek_pam_propose_member(ek_ctx *ctx, int32_t cid, int64_t j,
                          int64_t *frame_index, double *old_cost,
                          double *new_cost, int64_t *n_ambiguous);
int ek_pam_commit(ek_ctx *ctx, int accept);

/* Proposal prefetch.  A sweep (kmedoids.py:575-699) visits clusters 0..K-1 in
 * order, and an accepted proposal rarely changes the clusters visited next, so
 * the host may draw the next `count` (<= ek_pam_window_max(), 16) proposals
 * ahead of time and have their distance vectors computed together (one pass
 * over the frames per 8 of them, or -- ek_pam_prefetch_window -- only the
 * frames they can touch) instead of by one pass each; every guess is verified when its turn comes, so the sweep's
 * results do not change.
 *  ek_pam_count_members_batch: member counts of clusters cid0..cid0+count-1 in
 *    the current state (one read-back);
 *  ek_pam_select_members_batch: frames[i] = the js[i]-th member of cluster
 *    cid0+i, from the scans the batch count left (call it right after);
 *    js[i] < 0 skips cluster cid0+i (frames[i] = -1);
 *  ek_pam_prefetch: distances of every frame to frames[0..count) are computed
 *    and kept until the next ek_pam_prefetch / ek_pam_begin (count = 0 drops
 *    them); no read-back;
 *  ek_pam_propose_ex: ek_pam_propose with the member count of cluster cid
 *    supplied by the caller (n_members; it bounds the ambiguous set, the call
 *    fails if it was too small) and, when frame_index was prefetched, without
 *    the distance pass.  With win_count > 0 (<= 32), bit i of *moved_mask tells
 *    whether accepting the proposal changes the membership of cluster
 *    win_lo + i, i.e. whether member lists obtained earlier for that cluster
 *    are stale after ek_pam_commit(ctx, 1).
 *  ek_pam_prefetch_stats: proposals served from / not from a prefetched vector
 *    since the context was created. */
int ek_pam_count_members_batch(ek_ctx *ctx, int32_t cid0, int32_t count,
                               int64_t *counts);
int ek_pam_select_members_batch(ek_ctx *ctx, int32_t cid0, int32_t count,
                                const int64_t *js, int64_t *frames);
int ek_pam_prefetch(ek_ctx *ctx, const int64_t *frames, int32_t count);
/* The same when the caller works through clusters win_lo..win_lo+win_count-1
 * before the next prefetch (the sweep's window; the prefetched frames are
 * their proposals).  While the state is exact (ek_set_option key 6/7) exact
 * distances are then computed only for the frames a proposal can touch -- the
 * members of the window's clusters and every frame f with
 * D(its medoid, proposal) < 2 d(f) for some proposal; for the rest "not closer
 * than now" follows from the triangle inequality and the vector holds +inf --
 * instead of for all of them.  Same sweep results.  ek_pam_prefetch_passes
 * counts the prefetches of either kind. */
int ek_pam_prefetch_window(ek_ctx *ctx, const int64_t *frames, int32_t count,
                           int32_t win_lo, int32_t win_count);
int ek_pam_prefetch_passes(ek_ctx *ctx, int64_t *restricted, int64_t *full);
int ek_pam_propose_ex(ek_ctx *ctx, int32_t cid, int64_t frame_index,
                      int64_t n_members, int32_t win_lo, int32_t win_count,
                      double *old_cost, double *new_cost, int64_t *n_ambiguous,
                      uint32_t *moved_mask);
int ek_pam_prefetch_stats(ek_ctx *ctx, int64_t *hits, int64_t *misses);
/* A window of proposals without a host round trip each: the loop body of
 * kmedoids.py:597-699 for clusters cid0 .. cid0 + count - 1 (count <=
 * ek_pam_window_max()), in order.  frames[i] is the frame proposed for cluster cid0 + i, drawn by the
 * caller from that cluster's member list as it stood when the window was
 * opened, n_members[i] that list's length; every frames[i] must have been
 * prefetched with ek_pam_prefetch_window(ctx, frames, count, cid0, win_count).
 * All kernels are enqueued at once.  The device takes each decision --
 * mean(new^2) < mean(old^2) in float64, kmedoids.py:478-479, :683 --, commits
 * (:684-690) or undoes the proposal, and STOPS the window at the first cluster
 * whose member list an accepted proposal changed (its proposal was drawn from a
 * list that no longer holds, :611-614).  *n_done slots were decided; the caller
 * handles cluster cid0 + *n_done one proposal at a time and opens a new window
 * after it.  accept[i] (i < *n_done): 1 if proposal i was accepted; the costs
 * and ambiguous-member counts are returned for logging. */
/* windows ek_pam_window_run worked through in one workgroup (ek_set_option key
 * 12), and how many of them ended early because a proposal's ambiguous members
 * had more medoids within reach than one workgroup should search */
int ek_pam_sparse_stats(ek_ctx *ctx, int64_t *windows, int64_t *ended_early);
/* slots of those windows whose evaluation AHEAD of their turn was taken over
 * (ek_set_option key 19): every slot of a window is evaluated at once, one
 * workgroup each, on the state the window opens with; the window's workgroup
 * then goes through the slots in order (kmedoids.py:575-699 is sequential: a
 * proposal sees what the accepted ones before it changed) and takes a slot's
 * evaluation as it is unless an earlier slot it accepted changed a frame that
 * slot read or a medoid within its members' reach -- then the slot is
 * evaluated in its turn, as all were before round 5.  Same results either way. */
int ek_pam_ahead_stats(ek_ctx *ctx, int64_t *slots_taken_over);
/* the most proposals a window / a local-frame prefetch may hold */
int32_t ek_pam_window_max(void);
int ek_pam_window_run(ek_ctx *ctx, int32_t cid0, int32_t count,
                      const int64_t *frames, const int64_t *n_members,
                      int32_t win_lo, int32_t win_count, int32_t *n_done,
                      int32_t *accept, double *old_cost, double *new_cost,
                      int64_t *n_ambiguous);

/* The window loop of a whole sweep (kmedoids.py:575-699 for clusters *cid ..
 * n_medoids - 1, after ek_pam_begin): windows of up to `width` (2 ..
 * ek_pam_window_max()) proposals -- counted, drawn, selected, prefetched, decided
 * by ek_pam_window_run --, the cluster a window stops at one proposal at a time.
 * What the Python driver does call by call, without the interpreter between the
 * calls.  proposals == NULL: the draws are numpy's RandomState.choice(m) made on
 * `raw`, the next 32-bit outputs of the caller's RandomState
 * (randint(0, 2**32, dtype=uint32)); *pos counts the outputs consumed.
 * medoids[i] is replaced where proposal i was accepted; accept / old_cost /
 * new_cost / n_ambiguous [n_medoids] report every proposal.
 * *status: 0 done (*cid == n_medoids); 1 `raw` ran out -- call again with more
 * (everything returned so far stands); 2 cluster *cid is empty (choice raises). */
/* ek_pam_sweep's draws alone (host only, for tests): out[i] =
 * RandomState.choice(m[i]) -- 32-bit outputs masked to the bits of m - 1, values
 * above it rejected, m == 1 consumes nothing -- taken from `raw` from *pos on.
 * Returns how many draws were made: fewer than `count` if the outputs ran out or
 * an m[i] is < 1; -1 on a NULL argument. */
int64_t ek_np_choice_draws(const uint32_t *raw, int64_t n_raw, int64_t *pos,
                           const int64_t *m, int64_t count, int64_t *out);
int ek_pam_sweep(ek_ctx *ctx, int32_t n_medoids, int32_t width, const uint32_t *raw,
                 int64_t n_raw, int64_t *pos, const int64_t *proposals, int32_t *cid,
                 int64_t *medoids, int32_t *accept, double *old_cost,
                 double *new_cost, int64_t *n_ambiguous, int32_t *status);

/* PAM when the frames are sharded over several contexts (one per GPU; the
 * reference's MPI branch of kmedoids.py:575-699 with mpi/ops.py:143-212).  A
 * medoid or a proposal may then be a frame of another shard, so centers are
 * passed as centred center-major coordinates [3 * n_atoms] float32 + trace
 * (float64) in DEVICE memory -- the form ek_centered_frames produces and a
 * collective can move between ranks.
 *  ek_centered_frames: for i < count, row rows[i] of aos_dev / G_dev := centred
 *    coordinates and trace of LOCAL frame local_frames[i];
 *  ek_pam_begin_table: like ek_pam_begin, the medoid table given as
 *    n_medoids rows of aos_dev / G_dev;
 *  ek_pam_prefetch_centers: like ek_pam_prefetch for `count` centers given as
 *    rows of aos_dev / G_dev; the vectors are addressed by slot = row;
 *  ek_pam_propose_center: this shard's part of a proposal (distances of its
 *    frames to the center -- from prefetch slot `slot`, or computed when
 *    slot < 0 --, classification, ambiguous members against the trial table,
 *    cost sums).  n_members_local: members of cluster cid among this shard's
 *    frames.  No read-back: the 32-byte result
 *      { double sum_old, sum_new; int64 n_frames; uint32 n_ambiguous, moved }
 *    is written to out_dev (device memory) for the caller to exchange; the
 *    caller adds the sums over shards (cost = sum / total frames, kmedoids.py:
 *    478-479 with mpi/ops.py:143-166), ORs `moved`, checks n_ambiguous <=
 *    n_members_local, and then calls ek_pam_commit on every shard. */
int ek_centered_frames(ek_ctx *ctx, const int64_t *local_frames,
                       const int32_t *rows, int32_t count, float *aos_dev,
                       double *G_dev);
int ek_pam_begin_table(ek_ctx *ctx, const float *aos_dev, const double *G_dev,
                       int32_t n_medoids);
int ek_pam_prefetch_centers(ek_ctx *ctx, const float *aos_dev,
                            const double *G_dev, int32_t count);
int ek_pam_prefetch_centers_window(ek_ctx *ctx, const float *aos_dev,
                                   const double *G_dev, int32_t count,
                                   int32_t win_lo, int32_t win_count);
int ek_pam_propose_center(ek_ctx *ctx, int32_t cid, int32_t slot,
                          const float *center_aos_dev,
                          const double *center_G_dev, int64_t n_members_local,
                          int32_t win_lo, int32_t win_count, void *out_dev);

/* ---- MSM construction (secondary kernel) -------------------------------------
 * ek_msm_counts replaces assigns_to_counts
 * (enspara/msm/transition_matrices.py:113-170 with _transitions_helper
 * :310-321).  assigns: int32 state index per frame, trajectories concatenated
 * (host memory); lengths[n_trj]: frames per trajectory.  Frames equal to -1
 * are removed from their trajectory first (:156), then state[t] is paired
 * with state[t+lag_time] (sliding_window != 0) or every lag_time-th frame
 * with the next (:316-319).  Every other state must lie in [0, n_states).
 * Output: the count matrix as COO sorted by (row, col) with duplicates summed,
 * at most `capacity` entries (the number of frames is always enough). */
int ek_msm_counts(int device, const int32_t *assigns, const int64_t *lengths,
                  int64_t n_trj, int32_t lag_time, int32_t sliding_window,
                  int32_t n_states, int64_t capacity, int32_t *rows_out,
                  int32_t *cols_out, int64_t *counts_out, int64_t *nnz_out);
/* The same count over the labels a fit left in the context's HBM (the
 * reference pipes result.assignments into assigns_to_counts,
 * transition_matrices.py:113: here they need not leave the device in between).
 * lengths[n_trj]: how the context's frames, in order, split into trajectories
 * (they must add up to its frame count). */
int ek_msm_counts_ctx(ek_ctx *ctx, const int64_t *lengths, int64_t n_trj,
                      int32_t lag_time, int32_t sliding_window, int32_t n_states,
                      int64_t capacity, int32_t *rows_out, int32_t *cols_out,
                      int64_t *counts_out, int64_t *nnz_out);
/* ek_msm_row_normalize replaces _row_normalize's sparse branch
 * (enspara/msm/builders.py:188-196) on a CSR matrix (host arrays):
 * probs = diag(1/rowsum) * data, empty rows stay zero.  rowsum_out may be
 * NULL. */
int ek_msm_row_normalize(int device, const int64_t *indptr, const double *data,
                         int64_t n_rows, double *probs_out, double *rowsum_out);
/* ek_msm_mle_prinz replaces the iteration of builders.mle
 * (enspara/msm/builders.py:215-318): Prinz's reversible maximum-likelihood
 * sweeps over n states, all of them in one launch.  All arrays are host
 * memory.  The off-diagonal pairs i < j to update (those with
 * C[i,j] + C[j,i] > 0) are given level-major: level l holds pairs
 * [level_ptr[l], level_ptr[l+1]), no two pairs of a level share a state, and
 * two pairs that share a state lie in levels ordered as the pairs are
 * lexicographically -- then the result is the lexicographic sweep's bit for
 * bit (enspara_amd/msm/builders.py builds the levels; the call checks the
 * indices and the first property and returns EK_EARG otherwise).
 * c_ij[p] = C[i,j], c_ji[p] = C[j,i]; c_diag[s] = C[s,s]; c_rs = row sums of C.
 * x_pairs (X[i,j] = X[j,i]), x_diag, x_rs (row sums of X) hold X = C + C^T on
 * entry and the iterate on return.  A sweep is followed by another while
 * |logl - logl of the sweep before| > tol (0 before the first), at most
 * max_iter >= 1 sweeps: a negative tol runs exactly max_iter.  *n_iter_out =
 * sweeps that ran, *logl_out = logl of the last (the reference's formula,
 * :266 and :296-299, summed in a fixed order of the device's own). */
int ek_msm_mle_prinz(int device, int32_t n, int64_t n_pairs, int32_t n_levels,
                     const int64_t *level_ptr, const int32_t *pair_i,
                     const int32_t *pair_j, const double *c_ij,
                     const double *c_ji, const double *c_diag,
                     const double *c_rs, double *x_pairs, double *x_diag,
                     double *x_rs, double tol, int64_t max_iter,
                     int64_t *n_iter_out, double *logl_out);
/* BACE coarse-graining (enspara/msm/bace.py; Bowman, J. Chem. Phys. 137, 134111
 * (2012)).  All arrays are host memory; c is dense, row-major [n][n], finite and
 * not negative, n at most 16384.
 * ek_msm_bace_prune replaces the Bayes factors of baysean_prune (:341-369):
 * d_out[s] = the float32 value of state s against the pseudo-state
 * (multiDistHelper with c1 = float32(1) / float32(n), w1 = 1, c2 = c[s, :] +
 * 1 / n, w2 = w[s]), the sum taken in float64. */
int ek_msm_bace_prune(int device, int32_t n, const double *c, const double *w,
                      float *d_out);
/* ek_msm_bace_run replaces calcDMat and mergeTwoClosestStates (:122-213): the
 * initial matrix of inverse Bayes factors over the pairs s < d, s kept,
 * c[s, d] > 1, then n_merges merges, each followed by the recomputation of row
 * minX and the arg-max of the whole float32 matrix (first row-major index on
 * ties), without a host round trip in between.  c: the pruned counts; w: their
 * row sums + 1 on kept states; kept[n_kept]: the kept states, increasing;
 * n_merges must be max(n_kept - n_macrostates, 0).  records_out: n_merges + 1
 * records of 16 bytes { int32 minX, int32 minY, float32 1 / dMat[minX, minY],
 * int32 status }, one for the initial matrix and one after every merge; status 0:
 * a pair, 1: no pair with c > 1 was left (the matrix's maximum is 0: the factor
 * is 1 / 0 and nothing is merged after it), 2: not run for that reason.
 * dmat_steps > 0 (tests): dmat_out[step][n][n] receives the matrix as steps
 * 0 .. dmat_steps - 1 leave it. */
int ek_msm_bace_run(int device, int32_t n, const double *c, const double *w,
                    const int32_t *kept, int32_t n_kept, int32_t n_macrostates,
                    int32_t n_merges, void *records_out, int32_t dmat_steps,
                    float *dmat_out);

/* ---- dense float64 solve and transition path theory ------------------------------
 * ek_lu_solve: X = A^-1 B by a blocked LU with partial pivoting (the largest |a|
 * of a column, the lowest row on ties), the trailing update on the matrix cores.
 * All arrays are host memory, row-major: A [n][n], B and X [n][nrhs], 1 <= nrhs <=
 * n <= 32768.  pivots_out (may be null) [n]: the row exchanged with row k at step
 * k.  *info_out = -1, or the first column (from 0) whose pivot was zero or NaN: A
 * is singular to working precision and X is not a solution.  EK_ENOMEM (and no
 * allocation) if the device has not the memory for the padded [A | B].
 * ek_lu_set_timing(1) makes the calls below record, per kind of launch, the time
 * between HIP events; ek_lu_last_timing gives the last call's sums: ms_out[7] =
 * assembly and epilogue, panel, exchange, block-row solve, trailing update, back
 * substitution diagonal blocks, back substitution updates; gemm_flops_out[2] = the
 * flops of the trailing updates and of the back substitution's.  Tools only: one
 * call at a time. */
int ek_lu_solve(int device, int32_t n, const double *A, int32_t nrhs, const double *B,
                double *X, int32_t *pivots_out, int32_t *info_out);
int ek_lu_set_timing(int on);
int ek_lu_last_timing(double *ms_out, double *gemm_flops_out);
/* Transition path theory (enspara/tpt/core.py, enspara/tpt/tpt.py).  T is dense,
 * row-major [n][n], host memory, n at most 32768; sources / sinks are state
 * indices below n, at least one each, no state in both (EK_EARG otherwise).  T is
 * uploaded once, the system assembled, solved (as ek_lu_solve) and the result
 * finished on the device; *info_out as ek_lu_solve's.  EK_ENOMEM if the device
 * has not the memory (all-to-all: about 3 n^2 doubles).
 * ek_tpt_committors replaces committors (core.py:40-102): sources and sinks made
 * absorbing (_I_m_Q, :25-37), (I - Q) q = r with r = the sum over the sinks, in
 * the order given, of T[:, s], r[sinks] = 1, r[sources] = 0 -- one solve where
 * the reference takes one per sink and sums; q_out[n], q[sinks] = 1 and
 * q[sources] = 0 exactly.
 * ek_tpt_mfpts_sinks replaces mfpts with sinks (:143-154): t_out[n] = lagtime *
 * (I - Q)^-1 c, c = 1 off the sinks, 0 on them.
 * ek_tpt_mfpts_all replaces mfpts without (:133-139): Z = ((I - T) + W)^-1, every
 * row of W = pops[n]; mfpt_out[n][n] = (lagtime * (Z_jj - Z_ij)) / pops[j].
 * ek_tpt_fluxes replaces reactive_fluxes and net_fluxes (tpt.py:48-125): the
 * committors as above into q_out[n], then flux_out[n][n] = (T_ij * (pops[i] *
 * (1 - q_i))) * q_j with a zero diagonal, or with net != 0 max(f_ij - f_ji, 0). */
int ek_tpt_committors(int device, int32_t n, const double *T, const int32_t *sources,
                      int32_t n_sources, const int32_t *sinks, int32_t n_sinks,
                      double *q_out, int32_t *info_out);
int ek_tpt_mfpts_sinks(int device, int32_t n, const double *T, const int32_t *sinks,
                       int32_t n_sinks, double lagtime, double *t_out,
                       int32_t *info_out);
int ek_tpt_mfpts_all(int device, int32_t n, const double *T, const double *pops,
                     double lagtime, double *mfpt_out, int32_t *info_out);
int ek_tpt_fluxes(int device, int32_t n, const double *T, const int32_t *sources,
                  int32_t n_sources, const int32_t *sinks, int32_t n_sinks,
                  const double *pops, int32_t net, double *q_out, double *flux_out,
                  int32_t *info_out);
/* The highest-flux pathways of a net-flux matrix (enspara/tpt/path.py: top_path :46-160,
 * paths :197-320; csrc/ek_tpt_path.hip states the rule the reference's queue follows).  A
 * handle keeps the matrix on the device as a CSR of n <= 65535 rows, which removing a path
 * edits in place, and the running explained flux.  All arrays are host memory.
 * ek_tpt_paths_open: either dense [n][n] row-major (compacted on the device to its entries
 * > 0) or, with dense null, CSR arrays: indptr [n + 1] ascending from 0 to nnz < 2^31, cols
 * [nnz] in [0, n) and strictly ascending within a row, vals [nnz] (entries <= 0 are kept
 * and never followed).  Finite values are the caller's to check.  sources, sinks: indices
 * below n, at least one each; repeats and a state in both are allowed.  mode 0 keeps the
 * matrix and yields one path whatever its flux (top_path: an unreachable sink gives the
 * sink alone with flux -inf); 1 'subtract' and 2 'bottleneck' remove each path and stop
 * before a path of infinite flux, or after the one with which the number of paths reaches
 * num_paths or the sum of flux / total_flux, added up in that order, reaches flux_cutoff.
 * max_paths, max_nodes: paths (at most 4096) and nodes of one batch, 0 the defaults; a
 * batch's first path is taken whatever its length.  caps_out (may be null) [2] = the paths
 * of a batch and the length of nodes_out.  EK_EARG otherwise, also for a dense matrix with
 * 2^31 or more entries > 0; EK_ENOMEM if the device has not the memory.
 * ek_tpt_paths_next: the next batch, one launch: *count_out paths, path p = nodes_out[
 * offsets_out[p] .. offsets_out[p + 1]) from a source to a sink, fluxes_out[p] its flux;
 * nodes_out [caps[1]], offsets_out [caps[0] + 1], fluxes_out [caps[0]].  *done_out != 0:
 * no further path follows.  *info_out: 0, or 1 / 2 if a search / a walk back along a path
 * took more steps than there are states (the handle is done then; neither can happen).
 * ek_tpt_paths_stats: counts_out[4] = entries of the CSR, pops of all searches, paths
 * returned, 1 if the searches keep their state in the LDS; ms_out[2] = the compaction's
 * kernels and the search launches so far, between HIP events. */
typedef struct ek_tpt_paths ek_tpt_paths;
int ek_tpt_paths_open(int device, int32_t n, const double *dense, const int64_t *indptr,
                      const int32_t *cols, const double *vals, const int32_t *sources,
                      int32_t n_sources, const int32_t *sinks, int32_t n_sinks, int32_t mode,
                      int64_t num_paths, double total_flux, double flux_cutoff,
                      int32_t max_paths, int32_t max_nodes, int32_t *caps_out,
                      ek_tpt_paths **out);
int ek_tpt_paths_next(ek_tpt_paths *h, int32_t *nodes_out, int32_t *offsets_out,
                      double *fluxes_out, int32_t *count_out, int32_t *done_out,
                      int32_t *info_out);
int ek_tpt_paths_stats(ek_tpt_paths *h, int64_t *counts_out, double *ms_out);
int ek_tpt_paths_close(ek_tpt_paths *h);

/* ---- joint counts and mutual information of discrete features ----------------------
 * Replaces libinfo.matrix_bincount2d / bincount2d (enspara/info_theory/libinfo.pyx)
 * and the arithmetic of mutual_information (mutual_info.py:290-327).  A handle owns
 * the counts jc [fx][fy][nx][ny] uint32 on the device, zero when opened; 1 <= nx,
 * ny <= 255 (code 255 pads the frame axis and is no state), fx, fy <= 65535 * 64
 * (EK_EARG naming the limit).  All arrays are host memory.
 * ek_mi_add counts one trajectory into them: X [frames][fx], Y [frames][fy] state
 * codes as bytes, row-major, Y null = X against itself (fx == fy, nx == ny); 0 <=
 * frames < 2^31 - 64, and the frames of all calls stay below 2^32 (EK_EARG).  A code
 * that is no state of its feature (>= nx resp. ny) counts nowhere; the caller
 * validates.  The product of the two one-hot matrices runs on the int8 matrix cores
 * and its partial sums are added with integer atomics: the counts do not depend on
 * how the frames are split.  EK_ENOMEM if the device has not the memory for the
 * codes twice over.
 * ek_mi_load_counts replaces the counts by uploaded ones; n_obs is the largest sum
 * over a feature pair's cells, below 2^32 (the caller's to compute), and what later
 * ek_mi_add calls count on from.  ek_mi_counts downloads them.
 * ek_mi_information: mi_out [fx][fy] float64, per pair the sum over u (outer) and v
 * (inner) of P_uv * log(P_uv / (P_u * P_v)) with P = count / n_obs and the marginals
 * exact integer sums; terms with a zero P are skipped, nothing is fused; a pair
 * without observations gives 0.
 * ek_mi_last_timing: ms_out[3] = the last ek_mi_add's upload and pack, its count
 * kernel, the last ek_mi_information's kernel, between HIP events. */
typedef struct ek_mi ek_mi;
int ek_mi_open(int device, int32_t fx, int32_t fy, int32_t nx, int32_t ny, ek_mi **out);
int ek_mi_add(ek_mi *h, const uint8_t *X, const uint8_t *Y, int64_t frames);
int ek_mi_load_counts(ek_mi *h, const uint32_t *jc, uint64_t n_obs);
int ek_mi_counts(ek_mi *h, uint32_t *jc_out);
int ek_mi_information(ek_mi *h, double *mi_out);
int ek_mi_last_timing(ek_mi *h, double *ms_out);
int ek_mi_close(ek_mi *h);

/* ---- CARDS: transition statistics, disorder codes, four mutual-information matrices --
 * Replaces enspara/cards/disorder.py and the four mi_matrix calls of cards.py (csrc/
 * ek_cards.hip).  A handle keeps the rotamer codes S and the disorder codes D of every
 * trajectory added to it on the device, in ek_mi's packed layout; f features of
 * n_states <= 255 states each.  All arrays are host memory.
 * ek_cards_open: EK_EARG on ek_mi_open's limits, EK_ENOMEM if the four count arrays
 * ([f][f][n][n], [f][f][2][2], [f][f][n][2], [f][f][2][n] uint32) do not fit.
 * ek_cards_add: X [frames][f] state codes as bytes (the caller validates them), 1 <=
 * frames < 2^26, the frames of all calls below 2^32 (EK_EARG); uploads, packs, keeps
 * the codes and computes the trajectory's statistics.  EK_ENOMEM if the resident codes
 * (2 f frames bytes) do not fit.
 * ek_cards_stats: out [trajectories][f][4] int64 = (n, first, last, s2) per trajectory
 * and feature: the number of transitions (X[t] != X[t + 1], t + 1 < frames), the first
 * and the last transition frame and s2 = the sum of w (w + 1) / 2 over the waiting times
 * w = [first, differences ...]; without a transition (0, -1, -1, 0).
 * ek_cards_disorder: lo, hi [f] int64; D[t][j] = 1 exactly where neighbouring
 * transitions a < b of feature j exist with a <= t < b and lo[j] <= b - a <= hi[j], 0
 * elsewhere (before the first transition, from the last one on).
 * ek_cards_disorder_codes: out [frames][f] uint8 of trajectory `traj` (EK_ESTATE before
 * ek_cards_disorder).
 * ek_cards_matrices: mi_out [4][f][f] float64 = the mutual information (as
 * ek_mi_information's, not normalised) of S-S, D-D, S-D and D-S over all trajectories;
 * the D-S counts are the integer transpose of the S-D counts.  ek_cards_counts downloads
 * the counts of matrix `which` (0 .. 3) afterwards.
 * ek_cards_last_timing: ms_out[8] between HIP events = the last add's upload and pack,
 * its statistics kernels, the last ek_cards_disorder's kernels, and of the last
 * ek_cards_matrices the S-S, D-D and S-D count passes, the transpose, the four
 * information kernels.  ek_cards_scan_chunk: the frames of one scan chunk. */
typedef struct ek_cards ek_cards;
int ek_cards_open(int device, int32_t f, int32_t n_states, ek_cards **out);
int ek_cards_add(ek_cards *h, const uint8_t *X, int64_t frames);
int ek_cards_stats(ek_cards *h, int64_t *stats_out);
int ek_cards_disorder(ek_cards *h, const int64_t *lo, const int64_t *hi);
int ek_cards_disorder_codes(ek_cards *h, int32_t traj, uint8_t *out);
int ek_cards_matrices(ek_cards *h, double *mi_out);
int ek_cards_counts(ek_cards *h, int32_t which, uint32_t *jc_out);
int ek_cards_last_timing(ek_cards *h, double *ms_out);
int ek_cards_close(ek_cards *h);
int ek_cards_scan_chunk(void);

/* ---- Shrake-Rupley solvent-accessible surface area -----------------------------------
 * Replaces mdtraj.shrake_rupley(mode='atom') as enspara/info_theory/exposons.py calls it,
 * and condense_sidechain_sasas (csrc/ek_sasa.hip).  A handle holds, on the device, R
 * [atoms] = radius + probe in nm (0 < R <= 4), the n_points <= 4096 sphere points
 * [n_points][3] and n_groups >= 0 groups of atoms: group g lists group_atoms[
 * group_offsets[g] .. group_offsets[g + 1]), none empty, every index in [0, atoms)
 * (EK_EARG otherwise).  All arrays are host memory.
 * ek_sasa_run: xyz [frames][atoms][3] float32 in nm, finite and within 128 nm of the
 * origin (EK_EARG).  In float32, nothing fused: p = (R_i * s_k) + x_i per component;
 * point k of atom i is blocked iff for some j != i (dx*dx + dy*dy) + dz*dz < R_j * R_j
 * with d = p - x_j; counts_out [frames][atoms] = the points not blocked; areas_out
 * [frames][atoms] = ((c * R_i) * R_i) * float(count), c = float(4 pi / n_points);
 * groups_out [frames][n_groups] = 0.0f plus the group's areas in the order listed.
 * Each output may be null.  Neighbours are culled at r_ij < R_i + R_j + 2^-13 nm, which
 * under the limits above never changes a count.  chunk_frames > 0: frames
 * of one upload and launch (at most 32768); 0: what fits half of the free device memory.
 * ek_sasa_last_timing: ms_out[3] = the last run's uploads, count kernels and group
 * kernels, summed over its chunks, between HIP events. */
typedef struct ek_sasa ek_sasa;
int ek_sasa_open(int device, int32_t atoms, const float *R, int32_t n_points,
                 const float *points, int32_t n_groups, const int32_t *group_offsets,
                 const int32_t *group_atoms, ek_sasa **out);
int ek_sasa_run(ek_sasa *h, const float *xyz, int64_t frames, int64_t chunk_frames,
                int32_t *counts_out, float *areas_out, float *groups_out);
int ek_sasa_last_timing(ek_sasa *h, double *ms_out);
int ek_sasa_close(ek_sasa *h);

/* ---- Superposition and weighted RMSF ---------------------------------------------------
 * Replaces enspara/geometry/rmsf.py and the md.Trajectory.superpose it calls
 * (csrc/ek_rmsf.hip, csrc/ek_superpose.h; the contract is DESIGN.md 4o).  A handle holds,
 * on the device, the n_sel >= 3 atoms `sel` (each in [0, atoms)) that define the fit, the
 * reference structure [atoms][3] (finite), its selection centred, and the running sums;
 * on the host n_groups >= 0 groups of atoms, group g = group_atoms[group_offsets[g] ..
 * group_offsets[g + 1]), none empty (EK_EARG otherwise).  All arrays are host memory.
 * ek_rmsf_run: xyz [frames][atoms][3] float32, finite (the caller's to check).  Every frame
 * is superposed on the reference over the selection: centroid in float64, centred
 * coordinates and the 3x3 inner products rounded to float32, the largest root by the
 * iteration of the RMSD kernels, the rotation from the adjugate of K - lambda I in float64;
 * aligned_out [frames][atoms][3] = float32(R (x - centroid) + the reference selection's
 * centroid), rotations_out [frames][9] row-major, rmsd_out [frames] over the selection;
 * each may be null.  flags_out [frames] (required): bit 0 = the rotation is not determined
 * (gap of the two largest eigenvalues <= 2e-5 (Gx + Gy)); such a frame gets the identity.
 * Frame ref_index (-1: none) is taken as it is: the identity, its own bits.  weights
 * [frames] float64 (null: no sums): sums_a += w_f |aligned_fa - reference_a|^2 in float64,
 * per tile of 32 frames (absolute indices over all runs of the handle) in frame order, the
 * tiles then in order: the bits do not depend on chunk_frames or on how the frames are cut
 * into runs.  chunk_frames > 0: frames of one upload and launch; 0: what fits half of the
 * free device memory.
 * ek_rmsf_fetch: atom_sums_out [atoms] and group_sums_out [n_groups] = the sum of a group's
 * atom sums in listed order, divided by their count; each may be null.
 * ek_rmsf_last_timing: ms_out[3] = the last run's uploads, kernels and downloads, summed
 * over its chunks, between HIP events. */
typedef struct ek_rmsf ek_rmsf;
int ek_rmsf_open(int device, int32_t atoms, int32_t n_sel, const int32_t *sel,
                 const float *reference, int32_t n_groups, const int32_t *group_offsets,
                 const int32_t *group_atoms, ek_rmsf **out);
int ek_rmsf_run(ek_rmsf *h, const float *xyz, int64_t frames, const double *weights,
                int64_t ref_index, int64_t chunk_frames, float *aligned_out,
                double *rotations_out, float *rmsd_out, uint32_t *flags_out);
int ek_rmsf_fetch(ek_rmsf *h, double *atom_sums_out, double *group_sums_out);
int ek_rmsf_last_timing(ek_rmsf *h, double *ms_out);
int ek_rmsf_close(ek_rmsf *h);

/* ---- Bootstrapped transition counts -----------------------------------------------------
 * Replaces the per-trial loop of enspara/msm/bootstrap.py (csrc/ek_msm_boot.hip; the
 * contract is DESIGN.md 4p).  A trial draws units (trajectories or blocks of them) with
 * replacement; its counts are sum_u mult[u][trial] * (counts of unit u) and live on the
 * sparsity pattern of the full data's counts.  All arrays are host memory.
 * ek_msm_boot_open: assigns = the units' frames one after the other (-1 = no state, dropped
 * per unit before pairing, as ek_msm_counts does), lengths [n_units] >= 0; the pattern as
 * CSR over n_states rows: indptr [n_states + 1], cols [nnz] ascending inside a row; mult
 * [n_units][R] int32, R = n_trials rounded up to a multiple of 64, the padding zero.  One
 * pass over the frames fills the table [nnz][R] int32, which stays on the device: the
 * caller guarantees that no cell of a trial reaches 2^31.  chunk = consecutive positions
 * one wave of the scatter walks (0: 256); the table's bytes do not depend on it.  A state
 * outside [0, n_states) is EK_EARG; a transition of the frames that the pattern does not
 * hold is EK_ESTATE.
 * ek_msm_boot_fetch: out [r1 - r0][nnz] int64 = the counts of trials r0 .. r1 - 1.
 * ek_msm_boot_build: row normalisation of every trial on the symmetrised pattern S (nnzS
 * cells, CSR indptrS over n_states rows): cell j of S is table cell idx_ij[j] plus table
 * cell idx_ji[j], each -1 for none; v = their integer sum, w = the row's exact sum,
 * probs_out [n_trials][nnzS] = ((w > 0) ? 1 / w : 0) * v, rowsum_out [n_trials][n_states]
 * = w: the two roundings of ek_msm_row_normalize.
 * ek_msm_boot_last_timing: ms_out[3] = squeeze and cells, the scatter, the last build,
 * between HIP events. */
typedef struct ek_msm_boot ek_msm_boot;
int ek_msm_boot_open(int device, const int32_t *assigns, const int64_t *lengths,
                     int64_t n_units, int32_t lag_time, int32_t sliding_window,
                     int32_t n_states, int64_t nnz, const int64_t *indptr,
                     const int32_t *cols, int32_t n_trials, const int32_t *mult,
                     int32_t chunk, ek_msm_boot **out);
int ek_msm_boot_fetch(ek_msm_boot *h, int32_t r0, int32_t r1, int64_t *out);
int ek_msm_boot_build(ek_msm_boot *h, int64_t nnzS, const int64_t *indptrS,
                      const int64_t *idx_ij, const int64_t *idx_ji, double *probs_out,
                      double *rowsum_out);
int ek_msm_boot_last_timing(ek_msm_boot *h, double *ms_out);
int ek_msm_boot_close(ek_msm_boot *h);

/* ---- LIGSITE pocket detection ---------------------------------------------------------
 * Replaces enspara/geometry/pockets.py (csrc/ek_pockets.hip; the contract is DESIGN.md
 * 4i).  A handle holds, on the device, cutoff [atoms] float64 = probe + radius in nm (> 0
 * and finite), the grid spacing (> 0 and finite) and min_rank.  All arrays are host memory.
 * ek_pockets_run: xyz [frames][atoms][3] float32 in nm, finite; origin [frames][3] float32
 * = each frame's smallest coordinates and dims [frames][3] = its grid (the caller takes
 * both from the coordinates), 0 <= dims <= 2048 per axis and at most 2^26 cells a frame
 * (EK_EARG), so that a flat index (ix * ny + iy) * nz + iz fits int32.  Cell i of an axis
 * lies at double(origin) + double(i) * spacing, not fused, and touches iff for some atom
 * (dx*dx + dy*dy) + dz*dz < cutoff * cutoff in float64, d = cell - double(x).  Along each
 * of the directions (1,0,0), (0,1,0), (0,0,1), (1,1,1), (-1,1,1), (-1,-1,1), (1,-1,1) a cell
 * that does not touch and lies strictly between its line's first and last touching cell
 * gains one rank; a diagonal line (sx, sy, 1) whose first cell has x and y on their start
 * faces (0 if s > 0, else n - 1) and z >= 1 is not scanned (the reference's enumeration
 * misses those lines).  Pocket cells are the ones with rank >= min_rank; a pocket is a
 * component of them under 18-connectivity (face and edge neighbours), labelled by its
 * smallest flat index.  A frame with a zero among its dims has no cells.
 * chunk_frames > 0: frames of one upload (at most 32768; EK_ENOMEM if they do not fit, and
 * EK_EARG if they hold 2^30 cells or more); 0: what fits half of the free device memory.
 * The number of launches of a chunk does not depend on its frames.
 * ek_pockets_counts: counts_out [frames] = the pocket cells of each frame of the last run
 * (frames must be that run's).  ek_pockets_fetch: cells_out, labels_out [sum of counts] =
 * the flat index and the label of every pocket cell, frame after frame, within a frame in
 * ascending flat index.  ek_pockets_last_timing: ms_out[4] = the last run's uploads, touch
 * kernels, line-extent and rank kernels, label and compaction kernels, summed over its
 * chunks, between HIP events.
 * One dense grid (dims [3], 1 <= cells <= 2^26), each stage alone: ek_pockets_touches:
 * xyz [atoms][3], cutoff [atoms], origin [3] -> touches_out [cells] bytes 0 / 1;
 * ek_pockets_ranks: touches [cells] (any non-zero byte touches) -> ranks_out [cells];
 * ek_pockets_labels: mask [cells] (non-zero = pocket cell) -> labels_out [cells], -1
 * outside the mask. */
typedef struct ek_pockets ek_pockets;
int ek_pockets_open(int device, int32_t atoms, const double *cutoff, double spacing,
                    int32_t min_rank, ek_pockets **out);
int ek_pockets_run(ek_pockets *h, const float *xyz, int64_t frames, const float *origin,
                   const int32_t *dims, int64_t chunk_frames);
int ek_pockets_counts(ek_pockets *h, int64_t frames, int64_t *counts_out);
int ek_pockets_fetch(ek_pockets *h, int32_t *cells_out, int32_t *labels_out);
int ek_pockets_last_timing(ek_pockets *h, double *ms_out);
int ek_pockets_close(ek_pockets *h);
int ek_pockets_touches(int device, const float *xyz, int32_t atoms, const double *cutoff,
                       double spacing, const float *origin, const int32_t *dims,
                       uint8_t *touches_out);
int ek_pockets_ranks(int device, const uint8_t *touches, const int32_t *dims,
                     uint8_t *ranks_out);
int ek_pockets_labels(int device, const uint8_t *mask, const int32_t *dims,
                      int32_t *labels_out);

/* ---- smFRET dye labelling ---------------------------------------------------------------
 * Replaces dye_distance_distribution of enspara/geometry/dyes_from_expt_dist.py and what it
 * calls (csrc/ek_dyes.hip; the contract is DESIGN.md 4l).  All arrays are host memory.
 * A handle holds, on the device, cutoff [atoms] float64 = radius + probe in nm (> 0 and
 * finite), the two point clouds dye1 [n1][3], dye2 [n2][3] float32 in nm (finite, 1 <= n <=
 * 2^20) and bin_width (> 0, finite).
 * ek_dyes_run: xyz [frames][atoms][3] float32 in nm, finite; Mt [frames][2][12] float32 =
 * per frame and labelled residue the rotation M (row-major, 9) and the translation t (3),
 * finite: the caller makes them on the host.  Placement 0 = dye1 on residue 0, 1 = dye1 on
 * residue 1, 2 = dye2 on residue 0, 3 = dye2 on residue 1; pair 0 = placements (0, 3), pair
 * 1 = placements (1, 2).
 * Alignment, float32, nothing fused: p_j = ((x*M[0][j] + y*M[1][j]) + z*M[2][j]) + t[j].
 * Touch test, float64: a point is kept iff for every atom sqrt((dx*dx + dy*dy) + dz*dz) >
 * cutoff, d = double(atom) - double(point), the square root correctly rounded.  The kernel
 * compares the squared distance with the smallest double whose correctly rounded square
 * root exceeds the cutoff (made on the host): the same set, no square root.  Kept points
 * keep their order.
 * Histogram of all distances between two clouds (n1 points, n2 points), float64 distances
 * by the same formula: if n1 * n2 <= 5e7 the pairs are one chunk; otherwise the larger
 * cloud (the second on a tie) is cut into chunks of 2048 consecutive points.  Per chunk c:
 * dmax_c = its largest distance, nbins_c = int(dmax_c / bin_width) + 2, step_c = (nbins_c *
 * bin_width) / nbins_c, edge k = double(k) * step_c, and a distance counts in bin k iff
 * edge_k <= d < edge_{k+1}.  The chunks' counts are added bin by bin (int64); nbins = the
 * largest nbins_c.  The kernels take no square root: dmax_c / bin_width >= m and d >= edge_k
 * are decided on the squared distance against thresholds that are the exact images of those
 * conditions under a correctly rounded square root and division (host tables).  Counts are
 * taken with integer atomics only: every run gives the same bits.
 * Bound: nbins_c <= 4096.  The diagonal of the box that holds both clouds (times 1 + 2^-16)
 * must be below 4093 bin widths; in a run the box holds, per residue and axis j, t_j +- (rho
 * |column j of M| + (|t_j| + rho |column j of M|) 2^-20) (1 + 2^-16), rho the largest norm
 * of a point of either cloud.  Coordinates are at most 2^20 nm in magnitude and bin_width
 * lies in [2^-40, 2^40] (EK_EARG).
 * chunk_frames > 0: frames of one upload (at most 4096; EK_ENOMEM if they do not fit); 0:
 * what fits half of the free device memory.  Per chunk of frames: one upload of xyz and Mt,
 * the kernels, one download of kept counts, nbins and counts.
 * ek_dyes_counts: kept_out [frames][4] = the kept points of every placement, nbins_out
 * [frames][2] = nbins of every pair (0 where a placement of the pair kept nothing) of the
 * last run (frames must be that run's).  ek_dyes_fetch: counts_out [sum of nbins] int64,
 * frame after frame, pair 0 then pair 1.  ek_dyes_last_timing: ms_out[4] = the last run's
 * uploads, touch and compaction kernels, histogram kernels, downloads, summed over its
 * chunks, between HIP events.
 * Each stage alone: ek_dyes_touches: xyz [atoms][3], cutoff [atoms], coords [n][3] float32
 * (as they are: no alignment) -> keep_out [n] bytes 0 / 1.  ek_dyes_pair_hist: coords1
 * [n1][3], coords2 [n2][3] float32 -> *nbins_out and counts_out [4096] int64, zero from
 * nbins on. */
typedef struct ek_dyes ek_dyes;
int ek_dyes_open(int device, int32_t atoms, const double *cutoff, int32_t n1,
                 const float *dye1, int32_t n2, const float *dye2, double bin_width,
                 ek_dyes **out);
int ek_dyes_run(ek_dyes *h, const float *xyz, int64_t frames, const float *Mt,
                int64_t chunk_frames);
int ek_dyes_counts(ek_dyes *h, int64_t frames, int32_t *kept_out, int32_t *nbins_out);
int ek_dyes_fetch(ek_dyes *h, int64_t *counts_out);
int ek_dyes_last_timing(ek_dyes *h, double *ms_out);
int ek_dyes_close(ek_dyes *h);
int ek_dyes_touches(int device, const float *xyz, int32_t atoms, const double *cutoff,
                    const float *coords, int32_t n, uint8_t *keep_out);
int ek_dyes_pair_hist(int device, const float *coords1, int32_t n1, const float *coords2,
                      int32_t n2, double bin_width, int32_t *nbins_out, int64_t *counts_out);

/* ---- explicit dyes placed on a residue ---------------------------------------------------
 * Replaces map_dye_on_protein of enspara/geometry/explicit_r0_calc.py and what it calls
 * (align_full_dye_to_res, remove_touches_protein_dye_traj, assemble_dye_r_mu;
 * csrc/ek_dye_map.hip; the contract is DESIGN.md 4q).  All arrays are host memory.
 * A handle holds, on the device, cutoff [atoms] float64 = radius + probe in nm (in (0, 2^20]),
 * the n_excl atoms `excl` the touch test skips, the dye library dye_xyz [D][A][3] float32 in
 * nm (finite, at most 2^20 in magnitude, D * A < 2^31 - 256), the selections prot_sel and
 * dye_sel of 3 <= n_sel <= 16 atoms each (in [0, atoms) and [0, A)), and the atoms r_atom,
 * mu0, mu1 in [0, A) of the emission centre and the dipole.  prot_sel null: the dye
 * coordinates are taken as they are (no fit; dye_sel and n_sel are ignored).
 * ek_dye_map_run: xyz [centres][atoms][3] float32 in nm, finite and at most 2^20 in
 * magnitude (the caller's to check, as for ek_rmsf_run), 1 <= centres <= 32768 (what
 * ek_dye_map_max_centres answers fits half of the free device memory).  Per (centre p,
 * conformation d):
 *   fit    as ek_rmsf_run with the sums taken sequentially in selection order: the
 *          centroids of the two selections as float64 sums, the centred coordinates
 *          rounded to float32, S, Gx, Gy as float64 sums of the exact products, S rounded to
 *          float32, lambda by the iteration of the RMSD kernels, R from the adjugate of K -
 *          lambda I; flag 1 (and the identity) where the rotation is not determined (gap of
 *          the two largest eigenvalues <= 2e-5 (Gx + Gy));
 *   apply  aligned = float32(fma(R_i2, z, fma(R_i1, y, R_i0 * x)) + c_ref_i), (x, y, z) =
 *          double(coordinate) - centroid of the conformation's selection;
 *   touch  float64: a dye atom is free iff for every atom a that is not excluded (dx*dx +
 *          dy*dy) + dz*dz >= thr_a, d = double(atom) - double(aligned), thr_a the smallest
 *          double whose correctly rounded square root exceeds cutoff_a (made on the host):
 *          free iff every distance > cutoff.  counts [p][d] = the free atoms, exactly.
 *          Atoms farther from c_ref than reach + cutoff_a + margin_p are dropped before the
 *          test, which changes no count (reach = the largest distance of a dye atom from
 *          its conformation's selection centroid; margin_p = 2^-22 (max|c_ref| + reach) +
 *          2^-40 reach; without a fit the centre is the mean of all dye atoms and the
 *          margin 0);
 *   r, mu  coords [p][d][9] = double of the aligned float32 coordinates of r_atom, of mu0,
 *          and of their float32 difference mu0 - mu1.
 * Counts are taken with integer atomics only: every run gives the same bits, whatever the
 * number of centres of a run.  want_aligned != 0 keeps aligned [p][d][A][3] for the fetch.
 * ek_dye_map_fetch: the last run's counts_out [centres][D] int32, coords_out [centres][D][9],
 * flags_out [centres][D] bytes, aligned_out [centres][D][A][3] or null (centres must be that
 * run's: EK_ESTATE).  ek_dye_map_stats: list_len_out [centres] = the atoms that passed the
 * cull, *reach_out (may be null) = reach.  ek_dye_map_last_timing: ms_out[5] = the last run's
 * upload, fit, cull and touch kernels and the last fetch's download, between HIP events. */
typedef struct ek_dye_map ek_dye_map;
int ek_dye_map_open(int device, int32_t atoms, const double *cutoff, int32_t n_excl,
                    const int32_t *excl, int32_t D, int32_t A, const float *dye_xyz,
                    int32_t n_sel, const int32_t *prot_sel, const int32_t *dye_sel,
                    int32_t r_atom, int32_t mu0, int32_t mu1, ek_dye_map **out);
int ek_dye_map_max_centres(ek_dye_map *h, int32_t want_aligned, int64_t *out);
int ek_dye_map_run(ek_dye_map *h, const float *xyz, int64_t centres, int32_t want_aligned);
int ek_dye_map_fetch(ek_dye_map *h, int64_t centres, int32_t *counts_out, double *coords_out,
                     uint8_t *flags_out, float *aligned_out);
int ek_dye_map_stats(ek_dye_map *h, int64_t centres, int32_t *list_len_out, double *reach_out);
int ek_dye_map_last_timing(ek_dye_map *h, double *ms_out);
int ek_dye_map_close(ek_dye_map *h);

/* ---- joint probabilities and mutual information of weighted frames --------------------
 * Replaces the arithmetic of weighted_mi (enspara/info_theory/mutual_info.py:78-178;
 * csrc/ek_wmi.hip).  codes [frames][F] state codes as bytes (the caller validates them:
 * a code >= S counts nowhere), weights [frames] float64 (finite and not negative: the
 * caller's to check), 1 <= frames < 2^31 - 64, F and S
 * within ek_mi_open's limits; host memory.  P_out (may be null) [F][F][S][S] float64,
 * P[i][j][u][v] = the sum over frames of w_t [f_ti == u] [f_tj == v], taken on the
 * float64 matrix cores per chunk of frames and over the chunks in ascending order: no
 * atomics, the same bits every run.  mi_out (may be null; not both) [F][F] float64 =
 * per pair the sum over u (outer) and v (inner) of P * log(P / (P_x[i][u] * P_x[j][v]))
 * with P_x[i][u] = P[i][i][u][u], terms with P = 0 or P_x * P_x = 0 skipped; not
 * normalised, not clipped.  EK_ENOMEM if the chunk partials do not fit the device.
 * ek_wmi_last_timing: ms_out[4] = the last run's upload and pack, product kernel,
 * reduction, information kernel, between HIP events. */
int ek_wmi_run(int device, const uint8_t *codes, const double *weights, int64_t frames,
               int32_t F, int32_t S, double *P_out, double *mi_out);
int ek_wmi_last_timing(double *ms_out);

/* ---- relative entropy, Shannon entropy, state counts ---------------------------------
 * Replaces the arithmetic of enspara/info_theory/entropy.py and of compute_rotamer_counts
 * in enspara/apps/compute-shannon-entropy.py (csrc/ek_entropy.hip).  All arrays are host
 * memory, all arithmetic is float64, nothing is fused; rows, cols >= 1.
 * ek_ent_kl_rows: P, Q [rows][cols] -> out[r] = the sum over j of t = P * log(P / Q), in
 * nats.  A t that is NaN counts as 0 (P = 0 whatever Q is); P > 0 with Q = 0 gives +inf.
 * flags_out: one word, bit 0 set if some element of P is negative, bit 1 for Q (the
 * sums are then meaningless; the caller raises).  The terms of a row are added in an
 * order that its width and the parity of its first flat index fix (csrc/ek_entropy.hip
 * spells it out): the same bits on every run, no float atomics, not numpy's pairwise
 * order.  Rows up to 8 wide take one lane each, up to 128 wide 8 lanes, wider a wave.
 * ek_ent_js_rows: the same walk with m = 0.5 * (P + Q) formed in registers; out_p[r] =
 * the sum of P * log(P / m), out_q[r] = the sum of Q * log(Q / m).
 * ek_ent_shannon_rows: out[r] = -(the sum over j of x * log(x)), elements x <= 0 (and NaN)
 * contribute 0; normalize != 0: x = p / (the row's sum), the sum taken first in the
 * same order.
 * ek_ent_kl_counts: Q is built on the device and never leaves it: the n x n matrix of
 * (double)count + prior from the nnz sparse counts (ci, cj in [0, n), cv >= 0, prior >= 0;
 * EK_EARG otherwise; every cell at most once, which the caller guarantees and the call
 * does not check: of a cell given twice one entry is kept, which one is not defined), each row divided as
 * ek_msm_row_normalize divides it (the row sum added in column order, inv = 1 / sum, 0
 * for an empty row, Q = inv * Q), then ek_ent_kl_rows' kernel on P [n][n] and Q ->
 * out [n].
 * ek_ent_last_timing: ms_out[3] = the last of these calls' upload, building of Q (0
 * unless ek_ent_kl_counts), row kernel, between HIP events.
 * EK_ENOMEM if the inputs do not fit the device. */
int ek_ent_kl_rows(int device, int64_t rows, int64_t cols, const double *P, const double *Q,
                   double *out, uint32_t *flags_out);
int ek_ent_js_rows(int device, int64_t rows, int64_t cols, const double *P, const double *Q,
                   double *out_p, double *out_q, uint32_t *flags_out);
int ek_ent_shannon_rows(int device, int64_t rows, int64_t cols, const double *p,
                        int32_t normalize, double *out);
int ek_ent_kl_counts(int device, int32_t n, const double *P, int64_t nnz, const int32_t *ci,
                     const int32_t *cj, const int64_t *cv, double prior, double *out,
                     uint32_t *flags_out);
int ek_ent_last_timing(double *ms_out);
/* A handle owns counts [f][n_states] uint64 on the device, zero when opened; f and
 * n_states within ek_mi_open's limits.  ek_ent_state_counts_add: codes [frames][f] state
 * codes as bytes (ek_mi_add's layout), 0 <= frames < 2^31 - 64; counts[j][u] += the
 * number of frames with codes[t][j] == u.  A code >= n_states counts nowhere; the caller
 * validates.  Lanes run along the feature axis; n_states <= 4 are counted in registers,
 * more in the LDS; integer atomics only, so the counts do not depend on how the frames are
 * split.  ek_ent_state_counts_read downloads them.  ek_ent_state_counts_last_timing:
 * ms_out[2] = the last add's upload, its kernel. */
typedef struct ek_ent_state_counts ek_ent_state_counts;
int ek_ent_state_counts_open(int device, int32_t f, int32_t n_states,
                             ek_ent_state_counts **out);
int ek_ent_state_counts_add(ek_ent_state_counts *h, const uint8_t *codes, int64_t frames);
int ek_ent_state_counts_read(ek_ent_state_counts *h, uint64_t *counts_out);
int ek_ent_state_counts_last_timing(ek_ent_state_counts *h, double *ms_out);
int ek_ent_state_counts_close(ek_ent_state_counts *h);

/* ---- kinetic Monte Carlo on a transition matrix, smFRET bursts, ensembles ------------
 * Replaces enspara/msm/synthetic_data.py and the burst sampling of
 * enspara/geometry/dyes_from_expt_dist.py (csrc/ek_kmc.hip).  All arrays
 * are host memory.
 * Uniforms: Philox4x32-10, key = seed (low word first), counter = {i lo, i hi, chain lo,
 * stream << 28 | chain hi} with i = index >> 1; the call's words a, b, c, d give the
 * doubles ((a >> 5) * 2^26 + (b >> 6)) * 2^-53 (index even) and the same of c, d (index
 * odd).  Streams: 0 transition (index = the step left), 1 initial state (index 0), 2
 * distance bin, 3 in-bin jitter, 4 photon coin (index = the photon within its burst).
 * chain < 2^60.  What a chain draws depends on (seed, chain, index) alone.
 * ek_kmc_create: the rows of T compressed to their nonzeros: indptr [n_states + 1], cols
 * [nnz] ascending within a row, cdf [nnz] = cumsum(nonzeros of the row) / its last (so
 * every row's last cdf is 1.0).  A row may be empty.  EK_EARG if indptr does not
 * ascend from 0 or a column is no state.
 * ek_kmc_next: next_out[i] = the column of the first cdf entry of row states[i] that is
 * > u[i] (0 <= u < 1 and states in range: the caller checks; the kernel clamps).
 * bad_out: -1, or the smallest state with an empty row that had to step.
 * ek_kmc_trajectories: out [n_chains][n_steps]; out[c][0] = start_states[c], out[c][t + 1]
 * = one step from out[c][t] with the transition double of (chain first_chain + c, index
 * t).  form: 0 the library chooses, 1 a lane per chain (binary search), 2 a wave per
 * chain (64 pivots and a ballot per round); the states do not depend on it, nor on
 * step_cap (> 0: steps per launch; 0: the default), nor on how the chains are split
 * into calls.  bad_out as above; the chain stays where it is.
 * ek_kmc_ensemble: p <- p T repeated n_steps - 1 times, p0 [n] first.  T [n][n] dense
 * row-major (colptr null), or column-compressed colptr [n + 1], rows, vals (T null).
 * observable null: out [n_steps][n] = every p; else out [n_steps] = p . observable.
 * p_out [n] = the last p.  Fixed summation order (csrc/ek_kmc.hip), no float atomics.
 * ek_kmc_fret_probs: E_out[k] = r06 / (r06 + d^6) with d = the centre of the bin picked
 * by inverse CDF (dist_cdf, per state dist_off [n_states + 1]) with the bin double of
 * (chain, k) + jitter double * bin_width - bin_width / 2, d^6 = (d d)(d d)(d d).
 * ek_kmc_fret_bursts: burst b (chain first_burst + b) has the photons frame_off[b] ..
 * frame_off[b + 1] at the frames `frames` (>= 0, not decreasing, at least one).  Its
 * chain starts at the inverse CDF pop_cdf [n_states] of the initial double and runs to
 * its last frame; photons_out[k] = 1 iff the coin double <= E of photon k.  traj_out
 * null, or the chains' states, burst after burst (last frame + 1 each), flat.
 * ek_kmc_last_timing: ms_out[3] = upload, kernels, download of the last call. */
typedef struct ek_kmc ek_kmc;
int ek_kmc_create(int device, int32_t n_states, const int64_t *indptr, const int32_t *cols,
                  const double *cdf, ek_kmc **out);
int ek_kmc_destroy(ek_kmc *h);
int ek_kmc_next(ek_kmc *h, int64_t n, const int32_t *states, const double *u,
                int32_t *next_out, int64_t *bad_out);
int ek_kmc_trajectories(ek_kmc *h, uint64_t seed, int64_t first_chain, int64_t n_chains,
                        const int32_t *start_states, int64_t n_steps, int32_t form,
                        int64_t step_cap, int32_t *out, int64_t *bad_out);
int ek_kmc_ensemble(int device, int32_t n, const double *T, const int64_t *colptr,
                    const int32_t *rows, const double *vals, const double *p0,
                    int64_t n_steps, const double *observable, double *p_out, double *out);
int ek_kmc_fret_probs(int device, uint64_t seed, int64_t chain, int64_t n,
                      const int32_t *states, int32_t n_states, const int64_t *dist_off,
                      const double *centres, const double *dist_cdf, double bin_width,
                      double r06, double *E_out);
int ek_kmc_fret_bursts(ek_kmc *h, uint64_t seed, int64_t first_burst, int64_t n_bursts,
                       const int64_t *frame_off, const int64_t *frames,
                       const double *pop_cdf, const int64_t *dist_off, const double *centres,
                       const double *dist_cdf, double bin_width, double r06,
                       int64_t step_cap, uint8_t *photons_out, int32_t *traj_out,
                       int64_t *bad_out);
int ek_kmc_last_timing(double *ms_out);

/* ---- donor-excitation Monte Carlo on a pair of dye MSMs -------------------------------
 * Replaces enspara/geometry/dye_lifetimes.py (resolve_excitation, explicit_static_dyes,
 * fully_averaged_explict_dyes) and the pair arithmetic of explicit_r0_calc.py
 * (csrc/ek_dye_pair.hip).  All arrays are host memory.
 * A handle holds n_problems problems side by side.  Per side (d_: donors, a_: acceptors):
 * off [n_problems + 1] = the first state of every problem in the side's one numbering, a
 * state at least per problem; indptr [n + 1], cols [nnz], cdf [nnz] = the rows of all
 * problems compressed as for ek_kmc_create, cols in the side's numbering and within the
 * row's problem (EK_EARG otherwise); init [n] = per problem cumsum(eq probs) / its last;
 * xyz [n][9] = emission centre, dipole origin, dipole vector.  consts [n_problems][6] =
 * p_rad, p_nonrad, dt, c6, 1 / Td, 0 with R0^6 = c6 k2.
 * Uniforms as for ek_kmc; streams 5 decay (index = the step), 6 donor and 7 acceptor
 * (index 0: the initial state, t + 1: the hop of step t), 8 the FRET coin (index 0).
 * Sample j of problem p is chain first_chain + p 2^32 + j; 1 <= n_samples < 2^32,
 * n_problems * n_samples < 2^31, first_chain < 2^59.
 * ek_dye_pair_table: k2, r, FE [nd][na] and the decay cdf [nd][na][3] of one problem.
 * ek_dye_pair_resolve, dtraj_out null: steps [n_problems][n_samples] (out) and
 * outcomes_out (0 radiative, 1 non-radiative, 2 energy transfer; 3: still excited after
 * max_steps) of every sample.  step_cap: steps per launch, max_steps: steps per
 * excitation (0: the defaults; max_steps < 2^24); neither changes a result.  over_out: -1,
 * or the first sample still excited after max_steps.  bad_out [2]: -1, or the smallest
 * donor / acceptor state (the side's numbering) with an empty row that had to hop.
 * dtraj_out, atraj_out not null: steps is input (what the first form returned); the
 * states of sample after sample, steps + 1 each, in the problem's own numbering;
 * traj_cells = sum(steps + 1) (EK_EARG otherwise).
 * ek_dye_pair_static: acceptor_out[i] = 1 iff the coin of sample i <= FE of its chain's
 * initial states (dstate_out, astate_out), or <= fe_fixed[problem] where fe_fixed is given.
 * ek_dye_pair_last_timing: ms_out[3] = upload, kernels, download of the last call. */
typedef struct ek_dye_pair ek_dye_pair;
int ek_dye_pair_create(int device, int32_t n_problems, const int64_t *d_off,
                       const int64_t *d_indptr, const int32_t *d_cols, const double *d_cdf,
                       const double *d_init, const double *d_xyz, const int64_t *a_off,
                       const int64_t *a_indptr, const int32_t *a_cols, const double *a_cdf,
                       const double *a_init, const double *a_xyz, const double *consts,
                       ek_dye_pair **out);
int ek_dye_pair_destroy(ek_dye_pair *h);
int ek_dye_pair_table(ek_dye_pair *h, int32_t problem, double *k2_out, double *r_out,
                      double *fe_out, double *cdf_out);
int ek_dye_pair_resolve(ek_dye_pair *h, uint64_t seed, int64_t first_chain, int64_t n_samples,
                        int64_t step_cap, int64_t max_steps, int32_t *steps,
                        int8_t *outcomes_out, int32_t *dtraj_out, int32_t *atraj_out,
                        int64_t traj_cells, int64_t *bad_out, int64_t *over_out);
int ek_dye_pair_static(ek_dye_pair *h, uint64_t seed, int64_t first_chain, int64_t n_samples,
                       const double *fe_fixed, int8_t *acceptor_out, int32_t *dstate_out,
                       int32_t *astate_out);
int ek_dye_pair_last_timing(double *ms_out);

/* ---- smFRET bursts with explicit dyes: lifetime and kappa-squared photons --------------
 * Replaces the burst-level functions of enspara/geometry/dye_lifetimes.py
 * (sample_lifetimes_guarenteed_photon, run_mc) and explicit_r0_calc.py (sample_dye_coords,
 * simulate_burst_k2) (csrc/ek_dye_bursts.hip).  All arrays are host memory.
 * The bursts, their frames, pop_cdf, step_cap, traj_out and the chain of burst b are those of
 * ek_kmc_fret_bursts: the same seed gives the same states under either rule.  Photon k of
 * burst b draws from (seed, chain first_burst + b, index k) on streams 9 the photon event,
 * 10 the donor's conformation, 11 the acceptor's; the coin of the second rule is stream 4.
 * pick(u, m) = min(m - 1, (int64)(u * (double)m)); every list has fewer than 2^31 entries.
 * ek_dye_bursts_lifetimes: per state s the photon events ev_off[s] .. ev_off[s + 1] with
 * lifetimes ev_life and flags ev_flag (0 donor, 1 acceptor).  Photon k takes the entry
 * ev_off[s] + pick(u, m_s) of the state s its chain is in: flags_out[k], life_out[k];
 * states_out[k] = s.  bad_row_out as bad_out of ek_kmc_fret_bursts; bad_state_out: -1, or the
 * smallest state without an entry that had to serve a photon (its outputs are 0).
 * ek_dye_bursts_k2: per state the donor's conformations d_off[s] .. d_off[s + 1] (rows of 9
 * doubles in d_xyz: emission centre, dipole origin, dipole vector) and the acceptor's.
 * Photon k takes donor row i = pick(u_10, nd_s), acceptor row j = pick(u_11, na_s); k2_out,
 * r_out as ek_dye_pair_table computes them, FE = c6 k2 / (c6 k2 + r^6) with r^6 = (r r)^3 of
 * the unrooted r^2, flags_out[k] = 1 iff the coin <= FE; drow_out, arow_out: null, or i and j
 * (both or neither).  bad_state_out: a state one of whose dyes has no conformation.
 * ek_dye_photons_lifetimes, ek_dye_photons_k2: the same rules on a list of states: entry k
 * draws what photon k of burst `chain` draws.
 * ek_dye_pick_events: index_out[k] = pick(u[k], m of states[k]) with the caller's doubles
 * (0 <= u < 1, EK_EARG otherwise), -1 where the state has no entry.
 * ek_dye_bursts_last_timing: ms_out[3] = upload, kernels, download of the last call. */
int ek_dye_bursts_lifetimes(ek_kmc *h, uint64_t seed, int64_t first_burst, int64_t n_bursts,
                            const int64_t *frame_off, const int64_t *frames,
                            const double *pop_cdf, const int64_t *ev_off, const double *ev_life,
                            const uint8_t *ev_flag, int64_t step_cap, uint8_t *flags_out,
                            double *life_out, int32_t *states_out, int32_t *traj_out,
                            int64_t *bad_row_out, int64_t *bad_state_out);
int ek_dye_bursts_k2(ek_kmc *h, uint64_t seed, int64_t first_burst, int64_t n_bursts,
                     const int64_t *frame_off, const int64_t *frames, const double *pop_cdf,
                     const int64_t *d_off, const double *d_xyz, const int64_t *a_off,
                     const double *a_xyz, double c6, int64_t step_cap, uint8_t *flags_out,
                     double *k2_out, double *r_out, int32_t *states_out, int32_t *drow_out,
                     int32_t *arow_out, int32_t *traj_out, int64_t *bad_row_out,
                     int64_t *bad_state_out);
int ek_dye_photons_lifetimes(int device, uint64_t seed, int64_t chain, int64_t n,
                             const int32_t *states, int32_t n_states, const int64_t *ev_off,
                             const double *ev_life, const uint8_t *ev_flag, uint8_t *flags_out,
                             double *life_out, int64_t *bad_state_out);
int ek_dye_photons_k2(int device, uint64_t seed, int64_t chain, int64_t n, const int32_t *states,
                      int32_t n_states, const int64_t *d_off, const double *d_xyz,
                      const int64_t *a_off, const double *a_xyz, double c6, uint8_t *flags_out,
                      double *k2_out, double *r_out, int32_t *drow_out, int32_t *arow_out,
                      int64_t *bad_state_out);
int ek_dye_pick_events(int device, int64_t n, const int32_t *states, const double *u,
                       int32_t n_states, const int64_t *ev_off, int64_t *index_out,
                       int64_t *bad_state_out);
int ek_dye_bursts_last_timing(double *ms_out);

/* ---- dihedral angles and buffered rotamer states ------------------------------------
 * Replaces enspara/geometry/rotamer.py (csrc/ek_rotamer.hip).  All arrays are host
 * memory.  A dihedral is of one of n_kinds kinds (kind [n] bytes); kind k has
 * n_basins[k] <= 8 basins with the boundaries hb[k][0 .. n_basins[k]] (hb [n_kinds][9]
 * float64, from 0 to 360, increasing) and the shift shift[k]; width is the buffer on
 * either side of a boundary, in [0, 360 / n_basins) (EK_EARG otherwise).
 * ek_rotamer_states: angles [frames][n] float32, degrees in [0, 360) (the caller
 * validates) -> states_out [frames][n] uint8.  a = angle - shift in float32, + 360 where
 * negative; frame 0 takes the basin a lies in (hb[i] <= a < hb[i + 1]; an a that rounds
 * to 360 counts as the last basin); a later frame keeps the current basin s unless a has
 * left its gates (lower = hb[s], 0 read as 360, minus width; upper = hb[s + 1], 360 read
 * as 0, plus width; upper < lower: upper <= a <= lower leaves; upper > lower: anything
 * outside lower <= a <= upper leaves; equal: never), then takes the basin a lies in.
 * Compared in float64.
 * ek_dihedral_angles: xyz [frames][atoms][3] float32, quads [n][4] atom indices (EK_EARG
 * out of range) -> angles_out [frames][n] float32: atan2((b1 . c1) |b2|, c1 . c2) with b1
 * = x1 - x0, b2 = x2 - x1, b3 = x3 - x2, c1 = b2 x b3, c2 = b1 x b2 in float32, in
 * degrees, + 360 where negative, 359.5 where above it.
 * ek_dihedral_rotamers: both in one pass over the coordinates, the states equal to
 * ek_rotamer_states of ek_dihedral_angles bit for bit; angles_out may be null.
 * ms_out (may be null) [2]: the dihedral kernel alone, the state scan, between HIP
 * events.  At most 2^27 frames a call (EK_EARG); EK_ENOMEM if the arrays do not fit the
 * device. */
int ek_rotamer_states(int device, const float *angles, int64_t frames, int32_t n,
                      const uint8_t *kind, int32_t n_kinds, const int32_t *n_basins,
                      const double *hb, const float *shift, double width,
                      uint8_t *states_out, double *ms_out);
int ek_dihedral_angles(int device, const float *xyz, int64_t frames, int32_t atoms,
                       const int32_t *quads, int32_t n, float *angles_out, double *ms_out);
int ek_dihedral_rotamers(int device, const float *xyz, int64_t frames, int32_t atoms,
                         const int32_t *quads, int32_t n, const uint8_t *kind,
                         int32_t n_kinds, const int32_t *n_basins, const double *hb,
                         const float *shift, double width, uint8_t *states_out,
                         float *angles_out, double *ms_out);

/* ---- leading eigenpairs of a sparse transition matrix ---------------------------
 * Device primitives of an Arnoldi / Krylov-Schur solver replacing the ARPACK /
 * LAPACK calls of eigenspectrum (enspara/msm/transition_matrices.py:173-233).
 * The operator A is given in CSR (host arrays, copied to the device); the
 * basis V[0..m_max] lives on the device.  The host keeps the projected
 * (m x m) problem only.
 *   ek_krylov_step(j, apply, h_col): w = A V[j] (apply != 0) or w = V[j+1]
 *     (apply == 0); orthogonalise w against V[0..j] (classical Gram-Schmidt,
 *     twice); h_col[0..j] = coefficients, h_col[j+1] = ||w||, V[j+1] = w/||w||.
 *   ek_krylov_rotate(m, kk, Q, move_last): V[0..kk) = V[0..m) Q, Q column-major
 *     m x kk; move_last != 0 also moves V[m] to V[kk] (restart). */
typedef struct ek_krylov ek_krylov;
int ek_krylov_create(int device, int64_t n, const int64_t *indptr,
                     const int32_t *indices, const double *data, int32_t m_max,
                     ek_krylov **out);
int ek_krylov_destroy(ek_krylov *k);
int ek_krylov_set_vector(ek_krylov *k, int32_t j, const double *vec);
int ek_krylov_get_vector(ek_krylov *k, int32_t j, double *vec);
int ek_krylov_step(ek_krylov *k, int32_t j, int32_t apply, double *h_col);
int ek_krylov_rotate(ek_krylov *k, int32_t m, int32_t kk, const double *Q,
                     int32_t move_last);
/* Arnoldi steps j0 .. m-1 enqueued back to back (one synchronisation at the
 * end).  H_out: column-major, leading dimension ldh >= m + 1; column j gets
 * h[0..j+1].  The caller checks the sub-diagonal for breakdowns. */
int ek_krylov_expand(ek_krylov *k, int32_t j0, int32_t m, double *H_out,
                     int32_t ldh);
/* The operator of ek_krylov_step / _expand from here on: A itself (degree 0) or
 * T_degree((A - c) / e), the Chebyshev polynomial on [a, b] = [c - e, c + e] (degree
 * >= 2: `degree` sparse products per step by the three-term recurrence).  What
 * eigenspectrum's restarted iteration uses once it has seen where the wanted
 * eigenvalues end (reference transition_matrices.py:173-233 leaves this to ARPACK):
 * eigenvalues above b are amplified and pulled apart, the rest stay within [-1, 1],
 * so the restarts -- and with them the orthogonalisations, most of the launches --
 * drop by an order of magnitude where the leading eigenvalues cluster at 1.  The
 * eigenpairs returned are A's: Rayleigh-Ritz on the converged subspace (host). */
int ek_krylov_set_filter(ek_krylov *k, int32_t degree, double a, double b);
/* out_host[c][0..n) = V[0..m) Q[:, c], c < kk <= m_max + 1; basis unchanged */
int ek_krylov_combine(ek_krylov *k, int32_t m, int32_t kk, const double *Q,
                      double *out_host);

/* ---- feature-space metrics --------------------------------------------------------
 * Replace the reference's native distance kernels, enspara/geometry/libdist.pyx
 * (_euclidean :122-145, _manhattan :100-117, _hamming :77-95; bound as metrics
 * 'euclidean' / 'manhattan' at enspara/cluster/util.py:292-295).
 * Samples: row-major [n_samples][n_features] host array of elem_kind
 * 0 = float32, 1 = float64, 2 = int64 (hamming only).  ek_feat_distance
 * computes metric 0 = euclidean, 1 = manhattan, 2 = hamming between every
 * sample and the point y (n_features elements of the same kind) into
 * float64 out_host[n_samples]; float32 samples use float32 differences and
 * squares and a float64 running sum in feature order, exactly as the
 * reference's generated C does. */
typedef struct ek_feat ek_feat;
int ek_feat_create(int device, int64_t n_samples, int32_t n_features,
                   int32_t elem_kind, ek_feat **out);
int ek_feat_destroy(ek_feat *k);
int ek_feat_load(ek_feat *k, const void *X, int64_t first, int64_t count);
int ek_feat_distance(ek_feat *k, int32_t metric, const void *y,
                     double *out_host);
/* The k-centers loop itself (kcenters.py:217-231 with the iteration of
 * :243-311) for a feature metric, resident on the device: per center one
 * launch computes metric(X, X[argmax]) with the arithmetic of
 * ek_feat_distance, applies the strict-< update to float64 distances / labels
 * kept in HBM and leaves arg-max partials; a single-workgroup launch reduces
 * them (first index of the maximum), applies the stop rule
 * `distances.max() > dist_cutoff` and fetches the next center's features.
 * dist_io / assign_io: the state on entry (float64 [n], int32 [n]; a fresh run
 * passes +inf / -1) and on return; labels first_label, first_label + 1, ..;
 * at most max_new centers; centers_out[0..*n_added) = the samples chosen;
 * *final_max = distances.max() after the last update. */
int ek_feat_kcenters(ek_feat *k, int32_t metric, int32_t first_label,
                     int32_t max_new, double dist_cutoff, double *dist_io,
                     int32_t *assign_io, int64_t *centers_out, int32_t *n_added,
                     double *final_max);
/* ---- the same loop over several shards (one ek_feat handle each) ----------------
 * The reference's MPI iteration (kcenters.py:314-378) for a feature metric:
 * every shard owns a contiguous block of the samples, `global_offset` is the
 * global index of its first one.  Per center every shard contributes ONE
 * candidate record, ek_feat_record_bytes(n_features, elem_kind) long (a multiple
 * of 16):
 *   { double max_dist; int64_t global_index; T row[n_features] }
 * max_dist = the maximum of the shard's float64 distances, global_index =
 * global_offset + the first local index of that maximum, row = that sample's
 * features in the samples' own element kind; a shard without samples writes
 * max_dist = -inf.  The caller exchanges the records (one all-gather);
 * ek_feat_kcenters_step is ONE launch: every workgroup picks the winner among
 * the n_recs records at all_recs_dev (largest max_dist, lowest record index
 * among equal ones -- with the shards in rank order np.argmax's first index over
 * the concatenated data), applies the stop rule `!(max > dist_cutoff)` to it (so
 * that every shard stops at the same label; later steps return at once),
 * computes metric(X_local, row) with the arithmetic of ek_feat_distance, applies
 * the strict-< update with `label`, and the workgroup that arrives last writes
 * the shard's next record to own_rec_dev (which may be the shard's slot of
 * all_recs_dev only where n_recs == 1) and appends (winner's global index, its
 * max_dist) to the history.  All pointers named *_dev are device memory; the
 * launches go to the handle's stream: `stream` of ek_feat_create_sharded (a
 * hipStream_t the caller keeps alive; NULL: a stream of the handle's own), so
 * that a caller's collectives on that stream are ordered with them.
 * ek_feat_state_reset: distances +inf, labels -1, history empty;
 * ek_feat_state_upload / _download: float64 [n_samples], int32 [n_samples];
 * ek_feat_local_candidate: the record of the state as it stands (once before the
 * loop, after a reset or an upload); ek_feat_history_download: entries
 * [first, first + count) (index -1 where none) and *n_done = last label + 1. */
size_t ek_feat_record_bytes(int32_t n_features, int32_t elem_kind);
int ek_feat_create_sharded(int device, int64_t n_samples, int32_t n_features,
                           int32_t elem_kind, int64_t global_offset, void *stream,
                           ek_feat **out);
int ek_feat_state_reset(ek_feat *k);
int ek_feat_state_upload(ek_feat *k, const double *dist_host,
                         const int32_t *assign_host);
int ek_feat_state_download(ek_feat *k, double *dist_host, int32_t *assign_host);
int ek_feat_local_candidate(ek_feat *k, void *rec_dev);
int ek_feat_kcenters_step(ek_feat *k, int32_t metric, const void *all_recs_dev,
                          int32_t n_recs, int32_t label, double dist_cutoff,
                          void *own_rec_dev);
int ek_feat_history_download(ek_feat *k, int32_t first, int32_t count,
                             int64_t *center_index_out, double *center_dist_out,
                             int32_t *n_done);
int ek_feat_history_reset(ek_feat *k);
/* Every sample against a table of centers (reference util.py:186-203 around a
 * libdist metric): centers_host is row-major [n_centers][n_features] in the
 * handle's element kind.  One launch: label 0 and distance +inf to begin with,
 * the centers visited in ascending order, updated on strict < (NaN is never
 * taken, the lowest index wins ties); every (sample, center) distance is one
 * thread's sum over the features in order, the arithmetic of ek_feat_distance,
 * so labels and float64 distances are what n_centers calls of it and the host
 * scan give, bit for bit.  The result replaces the handle's resident state
 * (float64 distances, int32 labels: ek_feat_state_download, ek_feat_kcenters_step
 * continue from it); n_centers == 0 leaves label 0 / +inf.  Works on handles of
 * ek_feat_create and ek_feat_create_sharded (on the caller's stream there);
 * returns after the work has completed. */
int ek_feat_assign_nearest(ek_feat *k, int32_t metric, const void *centers_host,
                           int32_t n_centers);
/* One PAM sweep (reference kmedoids.py:575-699, serial branch) over clusters
 * *cid .. n_medoids - 1 for metric 0 (euclidean) / 1 (manhattan), with the
 * float64 distances, the labels and the medoids' features resident on the device:
 * per proposal the member count, the draw, the distance of every sample to the
 * proposal, the three masks (:644-658), the ambiguous members against all
 * medoids (strict <, ascending medoid index: util.py:199-203), and both costs
 * mean(d**2) in float64 with numpy's pairwise summation (:478-479); the host
 * compares them (:683).  dist_io (float64) / assign_io (int32) are the state:
 * uploaded when *cid == 0, written back when the sweep is through.  proposals ==
 * NULL: proposals are drawn like RandomState.choice(state_inds) from `raw`, the
 * next 32-bit outputs of the caller's RandomState (*pos: outputs consumed).
 * medoids[c] is replaced and accept[c] = 1 where proposal c was accepted.
 * *status: 0 done; 1 `raw` ran out at cluster *cid (call again with more; the
 * state stays on the device); 2 cluster *cid has no member (choice raises).
 * Round 5: for samples beyond 64 MB the proposals go in windows of up to 32 --
 * drawn when the window opens, every sample's distance to each of them in ONE
 * pass; a drawn proposal's window ends where an accepted earlier one moved a
 * sample into or out of its cluster (:611-614 draws from the member list of the
 * moment).  Environment EK_FEAT_PAM_WINDOWS=1 / 0 forces / forbids the form,
 * EK_FEAT_PAM_SYNC=1 is round 3's loop with two waits per proposal; same
 * results in all of them. */
int ek_feat_pam_sweep(ek_feat *k, int32_t metric, int32_t n_medoids, int64_t *medoids,
                      const int64_t *proposals, const uint32_t *raw, int64_t n_raw,
                      int64_t *pos, double *dist_io, int32_t *assign_io,
                      int32_t *accept, int32_t *cid, int32_t *status);
/* frees what ek_feat_pam_sweep keeps between calls (ek_feat_destroy does it too) */
void ek_feat_pam_release(ek_feat *k);
/* ---- the same sweep over several shards (one ek_feat handle each) --------------
 * The reference's MPI branch of the sweep (kmedoids.py:575-699 with the draw of
 * :482-517) for a feature metric, on handles made by ek_feat_create_sharded that
 * hold a state (a k-centers run, ek_feat_state_reset / _upload).  The float64
 * distances, the labels and the features of ALL medoids stay on every shard; the
 * caller keeps the random stream and the decision.  Protocol, per sweep:
 *   1. every shard gathers the rows of the medoids it owns into a table
 *      [n_medoids][n_features] in the samples' element kind, zero elsewhere
 *      (ek_feat_pam_gather_rows: samples_host are LOCAL indices, rows_host the
 *      table rows they go to -- the library does not know the table's height:
 *      the caller guarantees rows_host[i] < its rows); the caller adds the shards' tables up (each row has
 *      one owner) and hands the sum to ek_feat_pam_begin, which keeps its own copy;
 *   2. per window of clusters (at most 32 per call, the limit of this interface;
 *      the driver in enspara_amd/sharded.py uses windows of 8):
 *      ek_feat_pam_count_batch -> the local member
 *      counts of clusters cid0 .. cid0 + count - 1 (the caller gathers them and
 *      draws choice(m) over the global count, members in global order);
 *      ek_feat_pam_select_batch(js) -> the js[j]-th LOCAL member of cluster
 *      cid0 + j in local order (-1 where js[j] < 0), from the scans the count of
 *      the same cid0 left; the owners gather the proposals' rows as in 1.;
 *   3. per proposal ek_feat_pam_propose(cid, row_dev, win_lo, win_count, out_dev):
 *      ONE read of the shard's samples -- metric(X_local, row) with the arithmetic
 *      of ek_feat_distance, the three masks of kmedoids.py:644-658 into a trial
 *      state, the ambiguous members against all medoids with the row in place of
 *      medoid cid (strict <, ascending medoid index) -- then the record at out_dev
 *        { double sum_old, sum_new; int64_t n; uint32_t n_amb, moved }   (32 bytes)
 *      sum_old / sum_new = np.sum(d ** 2) of the shard's distances as they stand /
 *      as the proposal would leave them, each in numpy's pairwise order over the
 *      shard's own float64 array; n = the shard's samples; n_amb = its ambiguous
 *      members; moved bit i = cluster win_lo + i (i < win_count <= 32) would lose
 *      or gain a sample on this shard.  A shard without samples writes zeros.
 *      The caller exchanges the records (one all-gather), adds the sums in shard
 *      order, divides by the global sample count and accepts iff new < old (:683);
 *   4. ek_feat_pam_commit(accept) on every shard: the trial state becomes the
 *      state, or the medoid table gets its column back.  One proposal at a time.
 * Nothing per sample crosses to the host.  All launches go to the handle's stream;
 * count / select / gather wait for it, begin / propose / commit do not.  With one
 * shard holding every sample the state after a sweep is ek_feat_pam_sweep's, bit
 * for bit. */
int ek_feat_pam_count_batch(ek_feat *k, int32_t cid0, int32_t count,
                            int64_t *counts_host);
int ek_feat_pam_select_batch(ek_feat *k, int32_t cid0, int32_t count,
                             const int64_t *js_host, int64_t *members_host);
int ek_feat_pam_gather_rows(ek_feat *k, int32_t count, const int64_t *samples_host,
                            const int64_t *rows_host, void *table_dev);
int ek_feat_pam_begin(ek_feat *k, int32_t metric, const void *table_dev,
                      int32_t n_medoids);
int ek_feat_pam_propose(ek_feat *k, int32_t cid, const void *row_dev, int32_t win_lo,
                        int32_t win_count, void *out_dev);
int ek_feat_pam_commit(ek_feat *k, int32_t accept);

/* ---- tuning knobs (benchmarks only) -------------------------------------- */
/* frames per lane of the distance kernel: 1, 2 or 4; 0 = choose from the
 * shard size */
int ek_set_frames_per_lane(ek_ctx *ctx, int fpl);
/* Options of a context: ek_set_option(ctx, key, value) / ek_get_option.  Every
 * option leaves centers, labels and distances unchanged (each form is tested
 * against the oracle); the ones marked MEASUREMENT exist so that two forms can
 * be timed against each other in one process and are not meant for callers. */
enum ek_option {
    /* non-temporal loads of the frame stream: 0 / 1; -1 = automatic (on when
     * the shard is larger than the Infinity Cache).  MEASUREMENT */
    EK_OPT_NONTEMPORAL = 1,
    /* nearest-center kernel (ek_assign_nearest): 0 automatic, 1 vector FMA, 2
     * MFMA 32x32x2, 3 MFMA 16x16x4 on the quad copy of the frames.
     * MEASUREMENT */
    EK_OPT_ASSIGN_KERNEL = 2,
    /* candidate centers per round of ek_kcenters_run / ek_ms_* / ek_spec_*: -1
     * automatic (up to 16, see EK_OPT_ADAPTIVE), 1 = one-center passes, 4, 8,
     * 16, 32 (32 only on request -- measured, its second sixteen guesses are
     * accepted too rarely --: the frames streamed twice per round, candidates
     * 0..15 and 16..31; the one-launch-per-step forms -- ek_spec_*,
     * EK_OPT_CHAINED = 0, EK_OPT_FUSED_ROUNDS = 0 -- stop at 16).  Every rank
     * of a group must hold the same value (sharded._agree_on_form) */
    EK_OPT_CANDIDATES = 4,
    /* cheap steps of a round in ek_kcenters_run: 1 chained (default), 0 one
     * launch pair per accepted center.  MEASUREMENT */
    EK_OPT_CHAINED = 5,
    /* PAM proposals search the ambiguous members' new medoid only among the
     * medoids within their reach (triangle inequality): 1 (default) / 0.  Used
     * only while the state is known to hold, for every frame, the distance to
     * the medoid its label names: true after ek_state_reset + k-centers, false
     * after ek_state_upload / ek_assign_nearest */
    EK_OPT_PAM_PRUNE = 6,
    /* assert (1) or withdraw (0) that property, e.g. after ek_assign_nearest
     * with the medoid frames themselves as centers */
    EK_OPT_STATE_EXACT = 7,
    /* with EK_OPT_CANDIDATES = -1, let ek_kcenters_run move between 1, 8 and 16
     * candidates per round by measured centers per millisecond: 1 (default) /
     * 0 (always the widest form) */
    EK_OPT_ADAPTIVE = 8,
    /* retired (round 1's pass kernel with the candidates staged in LDS); only
     * the value 1 is accepted */
    EK_OPT_PASS_FORM = 9,
    /* ek_kcenters_run's rounds in three launches (the single-workgroup steps
     * ride at the end of the launch that produces their input): 1 (default) /
     * 0 (one launch per step).  MEASUREMENT */
    EK_OPT_FUSED_ROUNDS = 10,
    /* the reference's `use_triangle_inequality` (kcenters.py:287-296 /
     * :351-364), 0 default / 1: per round the distances of the existing
     * centers to the candidates mark, per tile of 256 frames, the candidates
     * none of whose frames can move (own center at least twice the frame's
     * distance away, with a margin); such (tile, candidate) pairs are not
     * computed and a tile without any is not read.  From a fresh state
     * (ek_state_reset) and for >= 3 atoms.  Also in the sharded one-center
     * iteration (ek_kcenters_step with gathered records): every shard keeps a
     * table of the accepted centers filled from the winning records */
    EK_OPT_TRIANGLE = 11,
    /* ek_pam_window_run works through a window whose prefetch was restricted
     * to a list of frames in ONE workgroup, no launch between two proposals
     * (1, default) or with three launches per proposal (0).  MEASUREMENT */
    EK_OPT_PAM_ONE_WORKGROUP = 12,
    /* the (ambiguous member, medoid within reach) pairs such a workgroup
     * searches itself (default 16384); a proposal with more ends the window
     * and goes through the launches.  0 makes every proposal whose members
     * have another medoid within reach do so (tests) */
    EK_OPT_PAM_MAX_PAIRS = 13,
    /* such a workgroup takes both cost sums (numpy's order) for every proposal
     * (1) or only where the sum of the changes, new^2 - old^2 over the frames
     * the proposal moves, does not decide kmedoids.py:683's comparison by four
     * orders of magnitude more than the rounding of the sums can amount to (0,
     * default).  MEASUREMENT */
    EK_OPT_PAM_BOTH_SUMS = 14,
    /* the next round's candidates are chosen among the farthest frames per 64
     * frames of the state the whole chain leaves (1, default) or per 256 (0).
     * MEASUREMENT */
    EK_OPT_FINE_PICK = 15,
    /* ek_pam_sweep's windows of drawn proposals take the proposal-to-medoid
     * distance table as the lower bounds the medoid-to-medoid table and the
     * proposals' own distances give (triangle inequality; half the pairs of a
     * window's tables): 1 (default) / 0 exact distances.  MEASUREMENT */
    EK_OPT_PAM_BOUNDS = 16,
    /* how many of a label's farthest frames the candidate pick of a round may
     * list (the list of 64 the guesses are chosen from): 0 (default) = 4 or 16
     * by the share of its guesses the run sees accepted (4 suits frames in
     * clouds around templates, 16 a continuous landscape), 1 .. 16 fixed */
    EK_OPT_PICK_CAP = 17,
    /* ek_ms_run's ladder moves from rounds of 8 to 16 once they accept 4.5 (1)
     * or 6.5 (0, default) centers: 1 suits shards of up to ~300 000 frames;
     * every rank of a group must set the same value (sharded.kcenters_sharded
     * does, from the gathered shard sizes) */
    EK_OPT_SMALL_SHARDS = 18,
    /* a PAM window's slots evaluated at once ahead of their turn: 1 (default)
     * / 0 (each in its turn; ek_pam_ahead_stats).  MEASUREMENT */
    EK_OPT_PAM_AHEAD = 19,
    /* a PAM window's record, the next window's member counts and the drawn
     * frames written into mapped host memory by the kernels that make them (1,
     * default) or copied back behind them (0).  MEASUREMENT */
    EK_OPT_PAM_ZERO_COPY = 20,
    /* the distance kernels of a PAM window (tables, listed frames) on the
     * matrix cores, 16 rows x 16 columns per wave (1, default) or LDS-staged
     * 64 x 8 per workgroup (0); process-wide.  MEASUREMENT */
    EK_OPT_PAM_PAIRS_MFMA = 21,
    /* rounds of 16 candidates of ek_kcenters_run: the states every prefix of the
     * round's chain would leave are reduced to their per-tile arg-max by the pass
     * itself, from registers (the chain kernel is then one workgroup that decides
     * and picks, and the presumed order is the order the plan's greedy choice took
     * the candidates in) or by a sweep over the kept distance vectors in the chain
     * kernel (rounds 3-5): 1 (default) the former on shards of up to 524 288 frames
     * -- where it pays: 10 % of a fit at 125 000 frames, nothing at 10^6 --, 2
     * always, 0 never.  MEASUREMENT */
    EK_OPT_PASS_SWEEP = 22,
    /* ek_ms_run (peer mailboxes): an exchange in two steps inside the chain kernel --
     * every shard's per-prefix maxima first; every shard then walks the chain itself and
     * offers the far frames of the state the chain REALLY left -- (1, default) or in one,
     * the offers speculating that the whole chain holds and a chain that broke offered
     * again in an exchange of its own (0: rounds 3-5; what ek_ms_local / ek_ms_global,
     * whose exchange is the caller's collective, always do).  Every rank of a group must
     * hold the same value.  MEASUREMENT */
    EK_OPT_MS_TWO_PHASE = 23,
    /* ek_kcenters_run, single shard, fused rounds: stream only the frames a round can
     * still change.  A frame at distance d <= theta from its center cannot be changed
     * by a center accepted at 2 theta or more (triangle inequality, with the margin
     * of EK_OPT_TRIANGLE), so between two batches of rounds the frames above theta
     * are compacted -- ascending, bit copies -- into a second frame store, the rounds
     * run on it with a stop rule that refuses every center at or below the guard
     * 2 theta, and their results are scattered back.  Centers, labels and distances
     * are unchanged.  0 never, 1 (default) when the view would stream at most 0.8 x
     * the frames streamed now, 2 forced: rebuilt every other round whenever a frame is
     * settled (tests), 3 as 2 with the view's buffers filled with 0xFF bytes before
     * every rebuild (tests: a slot a rebuild fails to write is a NaN, not a lucky
     * zero).  Off with EK_OPT_TRIANGLE, an uploaded state, fewer than 3
     * atoms, or no memory for the second store. */
    EK_OPT_ACTIVE_VIEW = 24,
    /* the active view's policy, in per mille, 500 .. 950 each.  EK_OPT_VIEW_RHO
     * (default 750): a view's guard sits at this share of the maximum it was built
     * at; every value is sound (the guard is derived from theta).  EK_OPT_VIEW_RATIO
     * (default 800): a view is built when it would stream at most this share of the
     * frames streamed now. */
    EK_OPT_VIEW_RHO = 25,
    EK_OPT_VIEW_RATIO = 26
};
int ek_set_option(ek_ctx *ctx, int32_t key, int32_t value);
/* the value an option holds (what ek_set_option stored, or its default) */
int ek_get_option(ek_ctx *ctx, int32_t key, int32_t *value);
/* time of the last ek_kcenters_run loop measured with HIP events on the
 * context's stream, milliseconds, and the number of distance-kernel launches
 * it covered */
int ek_last_run_timing(ek_ctx *ctx, float *ms, int32_t *launches);

/* Sampled timing of the distance kernel alone: after ek_timing_begin, every
 * `sample_every`-th ek_kcenters_step brackets its distance-kernel launch with
 * a HIP event pair on the context's stream (at most max_samples pairs).
 * ek_timing_end synchronises and returns the mean elapsed time per sampled
 * launch in milliseconds -- of the launches with the number of candidates per
 * pass that was sampled most, which ek_timing_form then reports (a run moves
 * between 1, 8 and 16 candidates per pass). */
int ek_timing_begin(ek_ctx *ctx, int32_t sample_every, int32_t max_samples);
int ek_timing_end(ek_ctx *ctx, float *avg_ms, int32_t *n_samples);
int ek_timing_form(ek_ctx *ctx, int32_t *candidates);
/* gbytes_per_s[0]: read + write rate (GB/s) of a 16-byte-per-lane non-temporal
 * copy of `bytes` bytes on this GPU; [1]: the rate of only reading them (what the
 * distance kernels do); best of four each: the measured ceilings bench.py quotes
 * beside the nominal HBM peak */
int ek_hbm_copy_rate(int device, size_t bytes, double *gbytes_per_s);
/* Test entry: the QCP arithmetic of csrc/ek_qcp.h evaluated by a KERNEL on m
 * inner-product matrices handed over by the caller (host arrays: S [m][9] f32,
 * Gx / Gy [m] f64 traces, cur [m] f32 the distance each solve may stop above) --
 * full[i] = ek_rmsd_from_S, below[i] = ek_rmsd_from_S_below(.., cur[i]),
 * cert[i] = ek_far_certified_f32(S, (float)(Gx + Gy), n_atoms, cur[i]) in bit 0 and
 * ek_far_certified2_f32 (the second level) in bit 1 -- so that
 * the soundness tests of the early-stopped solve and of the float32 certificate
 * run through the instructions that ship (v_rcp_f32 / v_sqrt_f32 / v_rsq_f32:
 * 1 ulp, where the host build of the header rounds correctly).  Stands where
 * mdtraj.rmsd's own per-pair solve would (cluster/util.py:289-291); not used by
 * the product path. */
int ek_qcp_probe(int device, const float *S, const double *Gx, const double *Gy,
                 int32_t n_atoms, const float *cur, int64_t m, float *full,
                 float *below, unsigned char *cert);
/* Test entry: the distance kernels of a large shard's PAM window (csrc/ek_pam.hip:
 * ek_pam_pairs_kernel / ek_pam_pairs16_kernel, modes 0 and 1) on host arrays, through
 * the launchers the sweep itself calls.  rows [n_rows][3 n_atoms] f32 are centred
 * structures and rows_G [n_rows] f64 their traces, cols [n_col][3 n_atoms] / cols_G
 * likewise (n_col <= 32); the columns are made into records here.  form: 1 the
 * matrix-core kernels, 0 the LDS-staged ones, for this call only (ek_set_option key 21
 * is what it was afterwards).
 *   list == NULL, the tables of a window: rows are the medoid table, n_rows == K + 1,
 *     row K the medoid that row `held` stands for (held == -1: none).
 *     T [n_col][K] = rmsd(medoid c, column j); O [n_old][K] = rmsd(medoid c, medoid
 *     old_lo + i), old_lo + n_old <= K, n_old <= 32; dmin [ceil(n_col / 8)][K] = the
 *     minimum of T over each group of 8 columns.  dprop [n_col] given (n_old == n_col
 *     then): only O is computed, T[j][c] = max(O[j][c] - dprop[j], 0) and dmin from it.
 *   list [n_list] given (every entry < n_rows), the listed rows against the columns:
 *     vecs[j * n_pad + list[i]] = rmsd(row list[i], column j), n_pad >= n_rows.
 * T, O, dmin and vecs are copied to the device before the launch and back after it:
 * an entry no kernel wrote still holds what the caller put there.  Not used by the
 * product path. */
int ek_pam_pairs_probe(int device, int32_t form, int32_t n_atoms, const float *rows,
                       const double *rows_G, int64_t n_rows, const float *cols,
                       const double *cols_G, int32_t n_col, int32_t K, int32_t held,
                       int32_t old_lo, int32_t n_old, const float *dprop, float *T,
                       float *O, float *dmin, const uint32_t *list, int64_t n_list,
                       int64_t n_pad, float *vecs);

/* DEBUG (tools/fuzz_*.py).  With EK_POISON=1 in the environment when the library starts,
 * every working buffer of a context starts as 0x5a bytes (EK_POISON_BYTE) and is followed by a guard page;
 * this returns the number of buffers something wrote past the end of (their names go to
 * stderr), 0 without EK_POISON. */
int ek_debug_guards(ek_ctx *ctx);

/* ---- what the library holds on the device ------------------------------------
 * Every device allocation, pinned host allocation, stream and event of the library
 * goes through one counted front (csrc/ek_track.h).  out[7], all counted inside the
 * library (other processes on the card do not move them):
 *   [0] live device allocations        [1] their bytes (as asked for)
 *   [2] live pinned host allocations   [3] their bytes
 *   [4] live streams                   [5] live events
 *   [6] device allocations that succeeded since the library was loaded (monotonic)
 * Works without a device (all zeros there).  Always returns EK_OK for out != NULL. */
int ek_live_resources(int64_t *out);
/* TEST AID.  Arms one failure: the k-th device allocation from now (0-based, all
 * threads, whatever the device) returns hipErrorOutOfMemory from the counted front
 * without calling HIP or touching the device; the arm is then clear again.  k < 0
 * disarms.  Returns the arm that was pending (-1: none). */
int64_t ek_fail_alloc_at(int64_t k);

#ifdef __cplusplus
}
#endif
#endif /* ENSPARA_HIP_H */
