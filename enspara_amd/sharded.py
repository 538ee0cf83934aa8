"""Frame-sharded k-centers over the GPUs of one node.

One process per GPU (``torch.distributed``, backend "nccl" = RCCL over xGMI);
rank r owns the contiguous frame block [offset_r, offset_r + n_r) of the
concatenated data set.  Per iteration each rank contributes ONE candidate
record -- (local max distance, global index, trace, centred coordinates of
that frame; ``ek_record_bytes`` long, 3.6 KB at 300 atoms) -- to a single
all-gather; every rank then picks the same winner on the device (largest
distance, lowest rank on ties) inside the distance kernel's prologue.

This replaces the reference's MPI iteration, enspara/cluster/kcenters.py:
314-378: two pickled allgathers (:332-335) + owner arg-max (:337) + Bcast of
the frame (mpi/ops.py:169-212) + Barrier/allreduce(MAX) for the stop test
(mpi/ops.py:128-140).  Contiguous sharding + "lowest rank wins" reproduces
the single-process np.argmax first-index rule globally, so results are
identical to the 1-GPU run bit for bit, and center indices are plain global
frame numbers instead of the reference's (rank, local index) pairs.

The driver is written against a small shard protocol so that the same loop
runs on CPU with the "gloo" backend in tests (tests/test_sharded_gloo.py
plugs in a checker-backed shard); the product shard is :class:`DeviceShard`.

Feature metrics ('euclidean', 'manhattan', libdist.hamming on a 2-D array of
samples) shard the same way: :class:`FeatureShard` speaks the one-record part
of the protocol over an ``ek_feat`` handle -- record = (float64 local max
distance, global index, that sample's features), one launch per center and
rank (csrc/ek_feat_kcenters.hip ``feat_shard_step_kernel``) -- and
:func:`fit_features_sharded` is the estimators' ``mpi_mode`` for them: same
centers, labels and float64 distances as the single-process loop.  No rounds
of several candidates and no mailbox transport there; the PAM sweeps
(:func:`pam_sweep_sharded`) run over either kind of shard.
"""
import collections
import contextlib

import numpy as np


class _StoreShard:
    """What :class:`DeviceShard` and :class:`FeatureShard` share: the store's
    records and state in torch CUDA tensors that torch.distributed can move.
    The store must have been created on a non-default torch stream (``s =
    torch.cuda.Stream()``, handed over as ``stream=s.cuda_stream``) and the
    driver must run under ``with torch.cuda.stream(s)``: torch orders its
    collectives against the current stream, so kernels and the all-gather are
    then ordered on the device without host syncs.  (Handle 0, the legacy
    default stream, means "create your own" to ek_ctx_create.)"""

    def __init__(self, store):
        import torch
        self.torch = torch
        self.store = store
        self.device = torch.device("cuda", store.device)

    @property
    def record_bytes(self):
        return self.store.record_bytes

    @property
    def n_local(self):
        return self.store.n

    @property
    def offset(self):
        return self.store.global_offset

    def new_buffer(self, nbytes):
        return self.torch.empty(nbytes, dtype=self.torch.uint8,
                                device=self.device)

    def local_candidate(self, rec):
        self.store.local_candidate(rec.data_ptr())

    def progress(self):
        """-> number of centers so far; synchronises"""
        _, _, n_done = self.store.history(0, 0)
        return n_done

    def history(self, first, count):
        return self.store.history(first, count)

    def reset_history(self):
        self.store.reset_history()

    def state(self):
        """-> (distances [n_local], labels int32 [n_local]) on the host"""
        return self.store.download_state()

    def set_state(self, distances, assignments):
        """the caller's per-frame state (a warm start, kmedoids.py:133-146)"""
        self.store.upload_state(distances, assignments)

    def host_to_buffer(self, arr):
        """int64 numpy array -> tensor a collective can move"""
        return self.torch.from_numpy(np.ascontiguousarray(
            arr, dtype=np.int64)).to(self.device)

    def to_host(self, t):
        """Small device tensor -> numpy, waiting by polling an event: a
        blocking synchronize can cost far more than the proposal it guards
        when the host thread is put to sleep."""
        torch = self.torch
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        while not ev.query():
            pass
        return h.numpy()

    def pam_count_batch(self, cid0, count):
        return self.store.pam_count_members_batch(cid0, count)

    def pam_select_batch(self, cid0, js):
        return self.store.pam_select_members_batch(cid0, js)

    def pam_commit(self, accept):
        self.store.pam_commit(accept)


class DeviceShard(_StoreShard):
    """Shard protocol on top of a :class:`enspara_amd.device.FrameStore`
    (float32 distances; stream rules: :class:`_StoreShard`)."""

    def step(self, all_recs, n_recs, label, cutoff, own_rec):
        self.store.kcenters_step(all_recs.data_ptr(), n_recs, label, cutoff,
                                 own_rec.data_ptr())

    def set_triangle_inequality(self, on):
        self.store.set_option("triangle", 1 if on else 0)

    def quad_copy_ready(self):
        return self.store.quad_copy_ready()

    def pin_candidates(self, T):
        self.store.set_option("candidates", int(T))

    def reserve_centers(self, n_centers):
        self.store.reserve_centers(n_centers)

    def candidates_option(self):
        """what the option holds (-1: automatic), to put it back afterwards"""
        return self.store.get_option("candidates")

    def set_small_shards(self, on):
        self.store.set_option("small_shards", 1 if on else 0)

    def assign_nearest(self, centers_xyz):
        """every local frame against the given centers (float32 [K, A, 3]):
        the state becomes (nearest center, distance), util.py:199-203"""
        self.store.assign_nearest(centers_xyz)

    def set_exact(self, on):
        """every frame's distance IS the one to the medoid its label names
        (option key 7: lets the PAM search use the triangle inequality)"""
        self.store.set_option("state_exact", 1 if on else 0)

    # multi-candidate rounds
    @property
    def candidates(self):
        return self.store.candidates

    def spec_begin(self, first_label, limit, recs):
        self.store.spec_begin(first_label, limit, recs.data_ptr())

    def spec_round(self, recs_all, n_recs, cutoff):
        self.store.spec_round(recs_all.data_ptr(), n_recs, cutoff)

    def spec_localmax(self, hdr):
        self.store.spec_localmax(hdr.data_ptr())

    def spec_apply(self, hdrs_all, n_hdrs, cutoff):
        self.store.spec_apply(hdrs_all.data_ptr(), n_hdrs, cutoff)

    # chained cheap steps (csrc/ek_chain.hip)
    def spec_chain_bytes(self):
        return self.store.spec_chain_bytes()

    def spec_chain_rows(self, rows):
        self.store.spec_chain_rows(rows.data_ptr())

    def spec_chain_max(self, rows_all, n_shards, hdrs):
        self.store.spec_chain_max(rows_all.data_ptr(), n_shards,
                                  hdrs.data_ptr())

    def spec_chain_apply(self, hdrs_all, n_shards, cutoff):
        self.store.spec_chain_apply(hdrs_all.data_ptr(), n_shards, cutoff)

    def spec_round_end(self, recs):
        self.store.spec_round_end(recs.data_ptr())

    def spec_progress(self):
        return self.store.spec_progress()

    # rounds with one exchange each (csrc/ek_mshard.hip)
    def ms_setup(self, world, rank):
        return self.store.ms_setup(world, rank)

    def ms_begin(self, first_label, limit):
        self.store.ms_begin(first_label, limit)

    def ms_local(self, cutoff, msg):
        self.store.ms_local(cutoff, msg.data_ptr())

    def ms_global(self, cutoff, msgs_all):
        self.store.ms_global(cutoff, msgs_all.data_ptr())

    def ms_end(self):
        self.store.ms_end()

    ms_connected = 0        # shards whose mailboxes are connected (connect_mailboxes)

    def ms_run(self, first_label, max_new, cutoff):
        idx, cd, _ = self.store.ms_run(first_label, max_new, cutoff)
        return idx, cd

    # PAM across shards: centers travel as centred coordinates + trace
    @property
    def n_atoms(self):
        return self.store.A

    def new_table(self, rows):
        """-> (coords float32 [rows, 3A], meta int64 [2 * rows]), zeroed;
        meta[:rows] holds the traces' float64 bit patterns, meta[rows:] is
        free for the caller (global frame indices)."""
        t = self.torch
        return (t.zeros((rows, 3 * self.n_atoms), dtype=t.float32,
                        device=self.device),
                t.zeros(2 * rows, dtype=t.int64, device=self.device))

    def fill_rows(self, local_frames, rows, coords, meta):
        if len(local_frames):
            self.store.centered_frames(local_frames, rows, coords.data_ptr(),
                                       meta.data_ptr())

    def pam_begin_table(self, coords, meta, n_medoids):
        self.store.pam_begin_table(coords.data_ptr(), meta.data_ptr(),
                                   n_medoids)

    def pam_count(self, cid):
        return self.store.pam_count_members(cid)

    def pam_select(self, cid, j):
        return self.store.pam_select_member(cid, j)

    def pam_prefetch_centers(self, coords, meta, count, win_lo=0, win_count=0):
        self.store.pam_prefetch_centers(coords.data_ptr(), meta.data_ptr(),
                                        count, win_lo, win_count)

    def pam_propose_center(self, cid, slot, coords, meta, row, n_members_local,
                           win_lo, win_count, out):
        self.store.pam_propose_center(
            cid, slot, coords.data_ptr() + 12 * self.n_atoms * row,
            meta.data_ptr() + 8 * row, n_members_local, win_lo, win_count,
            out.data_ptr())


class FeatureShard(_StoreShard):
    """The one-record shard protocol (``record_bytes``, ``new_buffer``,
    ``local_candidate``, ``step``, ``progress``, ``history``,
    ``reset_history``) on top of a
    :class:`enspara_amd.geometry.libdist.FeatureStore` for ``metric`` 0
    euclidean / 1 manhattan / 2 hamming (float64 distances; stream rules:
    :class:`_StoreShard`).  No ``candidates``: one center per exchange."""

    def __init__(self, store, metric):
        super().__init__(store)
        self.metric = int(metric)

    def step(self, all_recs, n_recs, label, cutoff, own_rec):
        self.store.kcenters_step(self.metric, all_recs.data_ptr(), n_recs,
                                 label, cutoff, own_rec.data_ptr())

    def distance(self, y):
        """metric(X_local, y) -> float64 [n_local] on the host (warm start)"""
        out = np.zeros(self.store.n, dtype=np.float64)
        self.store.distance(self.metric, y, out)
        return out

    def assign_nearest(self, centers):
        """the nearest of ``centers`` ([K, n_features] rows) for every local
        sample, one launch; the result is the state on the device
        -> (distances float64 [n_local], labels int32 [n_local]) on the host"""
        return self.store.assign_nearest(self.metric, centers)

    def reset_state(self):
        """distances +inf, labels -1"""
        self.store.reset_state()

    # PAM across shards, the methods pam_sweep_sharded drives (DeviceShard's):
    # rows travel as [rows, n_features] tables in the samples' element kind,
    # the int64 `meta` vector only carries the proposals' global indices
    def new_table(self, rows):
        t = self.torch
        dt = {"float32": t.float32, "float64": t.float64,
              "int64": t.int64}[np.dtype(self.store.dtype).name]
        return (t.zeros((rows, self.store.F), dtype=dt, device=self.device),
                t.zeros(2 * rows, dtype=t.int64, device=self.device))

    def fill_rows(self, local_samples, rows, table, meta):
        if len(local_samples):
            self.store.pam_gather_rows(local_samples, rows, table.data_ptr())

    def pam_begin_table(self, table, meta, n_medoids):
        self.store.pam_begin(self.metric, table.data_ptr(), n_medoids)

    def pam_count(self, cid):
        return self.store.pam_count_members_batch(cid, 1)[0]

    def pam_select(self, cid, j):
        return self.store.pam_select_members_batch(cid, [j])[0]

    def pam_prefetch_centers(self, table, meta, count, win_lo=0, win_count=0):
        """(nothing to prepare: a proposal reads its row from the table)"""

    def pam_propose_center(self, cid, slot, table, meta, row, n_members_local,
                           win_lo, win_count, out):
        self.store.pam_propose(
            cid, table.data_ptr() + row * table.stride(0) * table.element_size(),
            win_lo, win_count, out.data_ptr())


def _to_host(shard, t):
    f = getattr(shard, "to_host", None)
    return f(t) if f is not None else t.cpu().numpy()


def _world(group):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


def _everyone(mine, group=None):
    """Every rank's (picklable) ``mine`` in rank order; ``[mine]`` where there
    is nobody else to ask: one rank, or no process group at all."""
    import torch.distributed as dist
    world, _ = _world(group)
    if world == 1:
        return [mine]
    said = [None] * world
    dist.all_gather_object(said, mine, group=group)
    return said


def kcenters_sharded(shard, first_label, max_new, dist_cutoff=0.0, group=None,
                     check_every=16, fresh=True, use_triangle_inequality=False):
    """Run up to ``max_new`` k-centers iterations over all ranks' shards.

    Every rank calls this with its own shard.  Returns
    (global center indices int64 [k], their pre-update distances float32 [k]);
    identical on every rank.  The per-frame state stays on each shard.
    ``fresh=False`` continues a previous call (keeps the accepted-center
    history and the candidate record already held by the shard).
    ``use_triangle_inequality`` (reference kcenters.py:351-364): one center per
    pass, every shard keeps the accepted centers and does not read the tiles of
    256 frames none of which can come closer to the new center than to its own
    (csrc/ek_kcenters.hip ek_ti_center_tab_kernel); same results, fewer bytes
    on time-ordered data.
    """
    import torch.distributed as dist
    world, _ = _world(group)
    collective = dist.is_available() and dist.is_initialized()
    T = getattr(shard, "candidates", 1)
    if hasattr(shard, "set_triangle_inequality"):
        shard.set_triangle_inequality(bool(use_triangle_inequality))
    if use_triangle_inequality:
        T = 1               # (the test is per center: one-center passes)
    if T > 8 and hasattr(shard, "quad_copy_ready"):
        # (a group that has to narrow its rounds does so for THIS run only: the
        # caller's own setting of the option comes back afterwards)
        before = (shard.candidates_option()
                  if hasattr(shard, "candidates_option") else None)
        T0, T = T, _agree_on_form(shard, T, group, world, collective)
        if T != T0 and before is not None:
            try:
                return _kcenters_sharded_ms(shard, first_label, max_new,
                                            dist_cutoff, group, fresh, world,
                                            T, collective)
            finally:
                shard.pin_candidates(before)
    if T > 1 and world <= MAX_ROUND_RECORDS and hasattr(shard, "ms_local"):
        return _kcenters_sharded_ms(shard, first_label, max_new, dist_cutoff,
                                    group, fresh, world, T, collective)
    if T > 1 and world <= MAX_ROUND_RECORDS:
        return _kcenters_sharded_rounds(shard, first_label, max_new,
                                        dist_cutoff, group, fresh, world, T,
                                        collective)
    if T > 1:
        import logging
        logging.getLogger(__name__).warning(
            "%d ranks: more than the %d candidate records a round can choose "
            "from; falling back to one exchange per center", world,
            MAX_ROUND_RECORDS)
    rb = shard.record_bytes
    mine = shard.new_buffer(rb)
    everyone = shard.new_buffer(rb * world) if collective else mine
    if fresh:
        shard.reset_history()
    shard.local_candidate(mine)
    open_loop = not (dist_cutoff > 0)
    issued = 0
    while issued < max_new:
        todo = (max_new - issued) if open_loop else min(check_every,
                                                        max_new - issued)
        for i in range(todo):
            if collective:
                dist.all_gather_into_tensor(everyone, mine, group=group)
            shard.step(everyone, world, first_label + issued + i,
                       float(dist_cutoff), mine)
        issued += todo
        if not open_loop:
            n_done = shard.progress()
            if n_done < first_label + issued:     # a step hit the stop rule
                break
    idx, cd, n_done = shard.history(first_label, max_new)
    k = max(0, n_done - first_label)
    return np.array(idx[:k], dtype=np.int64), np.array(cd[:k],
                                                      dtype=np.float32)


# records a round's plan can choose its candidates from (the device keeps a
# 64 x 64 table of their pairwise distances, csrc/ek_spec.hip)
MAX_ROUND_RECORDS = 64


def _agree_on_form(shard, T, group, world, collective):
    """Every shard of a group has to run rounds of the same width: they plan
    the same candidates from the same messages.  Rounds of 16 / 32 need a third
    copy of the frames on the device; a rank without room for it would, on its
    own, run rounds of 8 beside peers running 16 -- diverging plans, a mailbox
    time-out.  So the ranks ask first (the copy is made here if it can be) and
    if ANY has no room, ALL pin their rounds to 8 candidates (option key 4)."""
    try:
        ok = 1 if shard.quad_copy_ready() else 0
    except Exception:           # reported by the run itself; here: narrow rounds
        ok = 0
    everyone = _gather_i64(shard, [ok, shard.n_local], group, world, collective)
    # (the ladder of the rounds across shards: earlier to 16 candidates where the
    # shards are small -- the same answer on every rank, from the same numbers)
    if hasattr(shard, "set_small_shards"):
        shard.set_small_shards(int(everyone[:, 1].max()) < 300000)
    if int(everyone[:, 0].min()) == 1:
        return T
    import logging
    logging.getLogger(__name__).warning(
        "rank(s) %s have no memory for the quad copy of their frames: every "
        "rank runs rounds of 8 candidates",
        [int(r) for r in np.flatnonzero(everyone[:, 0] == 0)])
    shard.pin_candidates(8)
    return 8


def _kcenters_sharded_ms(shard, first_label, max_new, dist_cutoff, group, fresh,
                         world, T, collective):
    """Rounds of up to T candidates with ONE exchange each (csrc/
    ek_mshard.hip): per round every rank all-gathers one message -- its (max
    distance, global index) in the state every prefix of the round's chain
    would leave, and its farthest frames of the state the whole chain would
    leave -- where the reference moves two allgathers, a frame broadcast and
    an allreduce per CENTER (kcenters.py:332-348).  Every rank takes the same
    decisions from the same messages.  If the shards are connected by peer
    mailboxes (`shard.ms_connected`), the exchange happens on the device and
    the whole loop inside the library (`ms_run`): nothing here per round."""
    import torch.distributed as dist
    rank = dist.get_rank(group) if collective else 0
    if fresh:
        shard.reset_history()
    if getattr(shard, "ms_connected", 0) == world:
        # (nothing is allocated inside the run: a hipMalloc / hipFree waits for the
        # whole device, and the peers may be polling for this shard's message by then)
        if hasattr(shard, "reserve_centers"):
            shard.reserve_centers(first_label + max_new)
        if collective:      # (the shards wait for one another on the device from here on)
            dist.barrier(group=group)
        idx, cd = shard.ms_run(first_label, max_new, float(dist_cutoff))
        return (np.array(idx, dtype=np.int64), np.array(cd, dtype=np.float32))
    key = (world, rank)
    if getattr(shard, "_ms_key", None) != key:
        shard._ms_bytes = shard.ms_setup(world, rank)
        shard._ms_key = key
    mb = shard._ms_bytes
    mine = shard.new_buffer(mb)
    everyone = shard.new_buffer(mb * world) if collective else mine
    limit = first_label + max_new
    shard.ms_begin(first_label, limit)
    n_done = first_label
    per_round = 0.6 * T
    while max_new > 0:
        # (the same count on every rank: n_done is)
        rounds = max(2, min(256, int((limit - n_done) / per_round) + 2))
        before = n_done
        for _ in range(rounds):
            shard.ms_local(float(dist_cutoff), mine)
            if collective:
                dist.all_gather_into_tensor(everyone, mine, group=group)
            shard.ms_global(float(dist_cutoff), everyone)
        n_done, stopped = shard.spec_progress()
        if stopped or n_done >= limit:
            break
        per_round = max(1.0, (n_done - before) / rounds)
    shard.ms_end()
    idx, cd, n_done = shard.history(first_label, max_new)
    k = max(0, min(max_new, n_done - first_label))
    return np.array(idx[:k], dtype=np.int64), np.array(cd[:k],
                                                      dtype=np.float32)


def connect_mailboxes(shard, group=None):
    """Peer mailboxes for the shards of a torch.distributed group of processes
    on one node (one GPU each): every rank publishes the hipIpc handles of its
    mailbox, opens the others', and from then on `kcenters_sharded` runs its
    rounds with the exchange on the device (DeviceShard.ms_run).  Collective:
    every rank calls it, and every rank makes the SAME sequence of collectives
    whatever fails where (a rank that cannot export or open a handle -- no
    peer access to one GPU -- still takes part in both gathers).  Returns True
    with ``shard.ms_connected = world`` only if every rank connected every
    peer; otherwise every rank closes what it opened, ``ms_connected`` is 0,
    ``shard.ms_connect_error`` holds this rank's exception (if it had one) and
    the caller stays on the all-gather transport."""
    import torch.distributed as dist
    world, rank = _world(group)
    st = shard.store
    why, mine = None, None
    try:
        st.ms_setup(world, rank)
        mine = st.ms_mailbox(ipc=True) if world > 1 else None
    except Exception as e:          # reported below, after the collectives
        why = e
    handles = [None] * world
    if world > 1:
        dist.all_gather_object(handles, mine, group=group)
    if why is None:
        try:
            for p in range(world):
                if p == rank:
                    st.ms_connect(p)
                elif handles[p] is None:
                    raise RuntimeError("rank %d published no mailbox" % p)
                else:
                    st.ms_connect(p, ipc=handles[p])
        except Exception as e:
            why = e
    # one more gather: the verdict, and the point no rank passes before every
    # rank has mapped every mailbox
    verdicts = [why is None]
    if world > 1:
        verdicts = [None] * world
        dist.all_gather_object(verdicts, why is None, group=group)
    shard.ms_connect_error = why
    if not all(verdicts):
        try:                        # closes the mappings, ms_peers = 0
            st.ms_setup(world, rank)
        except Exception:
            pass
        shard.ms_connected = 0
        return False
    shard.ms_connected = world
    return True


def _kcenters_sharded_rounds(shard, first_label, max_new, dist_cutoff, group,
                             fresh, world, T, collective):
    """Multi-candidate rounds (csrc/ek_spec.hip) across ranks.  Messages per
    round: one all-gather of T candidate records per rank, then -- chained
    cheap steps, csrc/ek_chain.hip -- one all-gather of each rank's view of
    the candidate frames it owns (320 B) and one of its per-prefix (max
    distance, global index) headers (128 B): three exchanges per round of
    ~6 centers, against the reference's two allgathers + Bcast + allreduce per
    center (kcenters.py:332-348).  A shard without the chained entry points
    falls back to one 16-byte header all-gather per accepted center."""
    import torch.distributed as dist
    rb = shard.record_bytes
    # every rank offers its first `offer` records (they are ordered: record 0 is
    # its farthest point): all T while world * T fits the plan's table, fewer
    # per rank in larger groups -- the round still runs T candidates
    offer = min(T, max(1, MAX_ROUND_RECORDS // world))
    recs_mine = shard.new_buffer(rb * T)
    recs_all = shard.new_buffer(rb * offer * world) if collective else recs_mine
    hdr_mine = shard.new_buffer(16)
    hdr_all = shard.new_buffer(16 * world) if collective else hdr_mine
    limit = first_label + max_new
    chained = hasattr(shard, "spec_chain_rows")
    if chained:
        rows_b, hdrs_b = shard.spec_chain_bytes()
        rows_mine = shard.new_buffer(rows_b)
        rows_all = shard.new_buffer(rows_b * world) if collective else rows_mine
        chdr_mine = shard.new_buffer(hdrs_b)
        chdr_all = shard.new_buffer(hdrs_b * world) if collective else chdr_mine
    if fresh:
        shard.reset_history()
    shard.spec_begin(first_label, limit, recs_mine)
    n_done = first_label
    per_round = 0.6 * T
    while max_new > 0:
        rounds = max(2, min(256, int((limit - n_done) / per_round) + 1))
        before = n_done
        for _ in range(rounds):
            if collective:
                dist.all_gather_into_tensor(recs_all, recs_mine[:rb * offer],
                                            group=group)
            shard.spec_round(recs_all, world * offer if collective else T,
                             float(dist_cutoff))
            if chained:
                shard.spec_chain_rows(rows_mine)
                if collective:
                    dist.all_gather_into_tensor(rows_all, rows_mine,
                                                group=group)
                shard.spec_chain_max(rows_all, world, chdr_mine)
                if collective:
                    dist.all_gather_into_tensor(chdr_all, chdr_mine,
                                                group=group)
                shard.spec_chain_apply(chdr_all, world, float(dist_cutoff))
            else:
                for _j in range(1, T):
                    shard.spec_localmax(hdr_mine)
                    if collective:
                        dist.all_gather_into_tensor(hdr_all, hdr_mine,
                                                    group=group)
                    shard.spec_apply(hdr_all, world, float(dist_cutoff))
            shard.spec_round_end(recs_mine)
        n_done, stopped = shard.spec_progress()
        if stopped or n_done >= limit:
            break
        per_round = max(1.0, (n_done - before) / rounds)
    idx, cd, n_done = shard.history(first_label, max_new)
    k = max(0, n_done - first_label)
    return np.array(idx[:k], dtype=np.int64), np.array(cd[:k],
                                                      dtype=np.float32)


def warm_start_sharded(shard, init_centers, group=None):
    """The warm start of the reference's k-centers (kcenters.py:200-206) over
    all ranks' shards: every frame goes to its nearest initial center
    (util.assign_to_nearest_center: strict <, the lower index wins ties) and
    every OCCUPIED label is represented by its member closest to that center
    (util.find_cluster_centers: the first such member) -- first in the GLOBAL
    order, rank r's frames following rank r-1's, so that the result is the
    single-process one.  (The reference's MPI mode runs find_cluster_centers on
    each rank's local arrays, kcenters.py:205: indices that mean different
    frames on different ranks.  Not reproduced.)

    Every rank passes the same ``init_centers``.  Returns the list of global
    frame indices, one per occupied label in label order: the k-centers loop
    continues from ``first_label = len(result)`` (kcenters.py:306)."""
    from .cluster.util import _stack_centers
    centers = _stack_centers([c for c in init_centers])
    K0 = int(centers.shape[0])
    shard.assign_nearest(centers)
    d, a = shard.state()
    return _closest_members(d, a, shard.offset, K0, group)


def _closest_members(d, a, offset, K0, group=None):
    """Per occupied label of 0..K0-1 the member closest to its center, the
    first such member in the GLOBAL order, from every rank's local (distances,
    labels): -> global indices in label order (see ``warm_start_sharded``)."""
    d = np.asarray(d, dtype=np.float64)
    a = np.asarray(a, dtype=np.int64)
    best_d = np.full(K0, np.inf, dtype=np.float64)
    best_g = np.full(K0, -1, dtype=np.int64)
    if len(a):
        # per label: smallest distance, then smallest index
        order = np.lexsort((np.arange(len(a)), d, a))
        lab = a[order]
        first = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
        best_d[lab[first]] = d[order[first]]
        best_g[lab[first]] = offset + order[first]
    tables = _everyone((best_d, best_g), group)
    ctr = []
    for lab in range(K0):
        win_d, win_g = np.inf, -1
        for bd, bg in tables:               # rank order = global frame order
            if bg[lab] >= 0 and (win_g < 0 or bd[lab] < win_d):
                win_d, win_g = bd[lab], int(bg[lab])
        if win_g >= 0:
            ctr.append(win_g)
    return ctr


def shard_bounds(n_total, world, rank, align=256):
    """Contiguous, tile-aligned split of n_total frames over ``world`` ranks.
    -> (offset, count)"""
    tiles = (n_total + align - 1) // align
    base, extra = divmod(tiles, world)
    t0 = rank * base + min(rank, extra)
    t1 = t0 + base + (1 if rank < extra else 0)
    lo = min(n_total, t0 * align)
    hi = min(n_total, t1 * align)
    return lo, hi - lo


# ---------------------------------------------------------------------------
# PAM (k-medoids) sweeps over sharded frames
# ---------------------------------------------------------------------------
PAM_OUT = np.dtype([("sum_old", "<f8"), ("sum_new", "<f8"),
                    ("n_frames", "<i8"), ("n_amb", "<u4"), ("moved", "<u4")])
assert PAM_OUT.itemsize == 32


def _gather_i64(shard, values, group, world, collective):
    """Every rank's small int64 vector -> ndarray [world, len(values)]."""
    import torch
    import torch.distributed as dist
    values = np.ascontiguousarray(values, dtype=np.int64)
    if not collective:
        return values[None, :].copy()
    mine = shard.host_to_buffer(values)
    everyone = torch.empty(world * len(values), dtype=torch.int64,
                           device=mine.device)
    dist.all_gather_into_tensor(everyone, mine, group=group)
    return _to_host(shard, everyone).reshape(world, len(values)).copy()


def _share_rows(coords, meta, group, collective):
    """Each row was filled by exactly one rank and is zero elsewhere: an
    integer sum over ranks of the raw bit patterns reproduces it exactly on
    every rank (x + 0 + ... + 0 in two's complement), for the float32
    coordinates, the float64 traces and the int64 indices alike."""
    if not collective:
        return
    import torch
    import torch.distributed as dist
    dist.all_reduce(coords.view(torch.int32), op=dist.ReduceOp.SUM,
                    group=group)
    dist.all_reduce(meta, op=dist.ReduceOp.SUM, group=group)


class _ShardWindow:
    __slots__ = ("lo", "hi", "m", "m_local", "before", "j", "gidx", "stale")


def pam_sweep_sharded(shard, medoids, proposals=None, random_state=None,
                      group=None, prefetch=8):
    """One PAM sweep (reference kmedoids.py:575-699, MPI branch) over all
    ranks' shards.  ``medoids``: global frame index of every cluster's medoid,
    the same list on every rank; ``random_state`` must also be the same on
    every rank (an int seed or identically seeded RandomState).  Returns the
    updated list -- identical on every rank and identical to what the
    single-GPU sweep returns for the concatenated frames; the per-frame state
    stays on the shards.

    Messages: per window of ``prefetch`` clusters one all-gather of member
    counts and one exchange of the proposed frames' coordinates (3.6 KB each
    at 300 atoms); per proposal one all-gather of a 32-byte record per rank
    (cost sums, moved-cluster mask) -- against the reference's pickled
    allgather + Bcast of the frame + two allreduces per proposal
    (kmedoids.py:482-517, mpi/ops.py:143-212)."""
    import torch.distributed as dist
    from .cluster.kcenters import check_random_state
    world, rank = _world(group)
    collective = dist.is_available() and dist.is_initialized()
    if collective and world > 1 and random_state is None and proposals is None:
        raise ValueError("pam_sweep_sharded needs a random_state shared by "
                         "all ranks")
    rs = check_random_state(random_state)
    medoids = [int(g) for g in medoids]
    K = len(medoids)
    if proposals is not None and len(proposals) != K:
        raise ValueError("Length of 'proposals' didn't match length of "
                         "'medoids' (%d != %d)." % (len(proposals), K))
    width = max(1, min(int(prefetch), 8))
    lay = _gather_i64(shard, [shard.offset, shard.n_local], group, world,
                      collective)
    n_total = int(lay[:, 1].sum())
    lo_mine, hi_mine = shard.offset, shard.offset + shard.n_local

    def owned(g):
        return lo_mine <= g < hi_mine

    # medoid table, assembled from the owners' rows
    coords, meta = shard.new_table(K)
    rows = [r for r, g in enumerate(medoids) if owned(g)]
    shard.fill_rows([medoids[r] - lo_mine for r in rows], rows, coords, meta)
    _share_rows(coords, meta, group, collective)
    shard.pam_begin_table(coords, meta, K)

    pc, pm = shard.new_table(width)            # window proposals
    oc, om = shard.new_table(1)                # a proposal outside the window
    out_mine = shard.new_buffer(PAM_OUT.itemsize)
    out_all = (shard.new_buffer(PAM_OUT.itemsize * world) if collective
               else out_mine)
    win = None
    acceptances = 0
    for cid in range(K):
        if win is None or cid >= win.hi:
            win = _ShardWindow()
            win.lo, win.hi, win.stale = cid, min(K, cid + width), 0
            cnt = win.hi - win.lo
            mine = shard.pam_count_batch(win.lo, cnt)
            allc = _gather_i64(shard, mine, group, world, collective)
            win.m = [int(x) for x in allc.sum(axis=0)]
            win.m_local = [int(x) for x in mine]
            win.before = [int(x) for x in allc[:rank].sum(axis=0)]
            pc.zero_()
            pm.zero_()
            if proposals is None:
                ahead = np.random.RandomState()
                ahead.set_state(rs.get_state())
                win.j = []
                for m in win.m:
                    if m <= 0:
                        break
                    win.j.append(int(ahead.choice(m)))
                jl = [j - b for j, b in zip(win.j, win.before)]
                jl = [x if 0 <= x < ml else -1
                      for x, ml in zip(jl, win.m_local)]
                slots = [s for s, x in enumerate(jl) if x >= 0]
                if slots:
                    fl = shard.pam_select_batch(win.lo, jl)
                    shard.fill_rows([int(fl[s]) for s in slots], slots, pc, pm)
                    idx = np.zeros(width, dtype=np.int64)
                    for s in slots:
                        idx[s] = lo_mine + int(fl[s])
                    pm[width:] = shard.host_to_buffer(idx)
                n_guess = len(win.j)
            else:
                win.j = None
                want = [int(g) for g in proposals[win.lo:win.hi]]
                slots = [s for s, g in enumerate(want) if owned(g)]
                shard.fill_rows([want[s] - lo_mine for s in slots], slots, pc,
                                pm)
                idx = np.zeros(width, dtype=np.int64)
                for s in slots:
                    idx[s] = want[s]
                pm[width:] = shard.host_to_buffer(idx)
                n_guess = cnt
            _share_rows(pc, pm, group, collective)
            win.gidx = [int(g) for g in
                        _to_host(shard, pm[width:width + n_guess])]
            shard.pam_prefetch_centers(pc, pm, n_guess, win.lo,
                                       win.hi - win.lo)
        slot = cid - win.lo
        exact = not ((win.stale >> slot) & 1)
        if exact:
            m, m_local, before = win.m[slot], win.m_local[slot], win.before[slot]
            counted = False
        else:
            m_local = int(shard.pam_count(cid))
            allc = _gather_i64(shard, [m_local], group, world, collective)
            m, before = int(allc.sum()), int(allc[:rank].sum())
            counted = True
        use_slot = -1
        if proposals is None:
            j = int(rs.choice(m))                            # kmedoids.py:514
            if exact and slot < len(win.j) and j == win.j[slot]:
                use_slot, g = slot, win.gidx[slot]
        else:
            use_slot, g = slot, win.gidx[slot]
        if use_slot < 0:
            oc.zero_()
            om.zero_()
            jl = j - before
            if 0 <= jl < m_local:
                if not counted:
                    shard.pam_count(cid)         # leaves the scan for select
                f = int(shard.pam_select(cid, jl))
                shard.fill_rows([f], [0], oc, om)
                om[1:] = shard.host_to_buffer([lo_mine + f])
            _share_rows(oc, om, group, collective)
            g = int(_to_host(shard, om[1:])[0])
            shard.pam_propose_center(cid, -1, oc, om, 0, m_local, win.lo,
                                     win.hi - win.lo, out_mine)
        else:
            shard.pam_propose_center(cid, use_slot, pc, pm, use_slot, m_local,
                                     win.lo, win.hi - win.lo, out_mine)
        if collective:
            dist.all_gather_into_tensor(out_all, out_mine, group=group)
        recs = _to_host(shard, out_all).view(PAM_OUT)
        if int(recs[rank]["n_amb"]) > m_local:
            raise RuntimeError("PAM proposal for cluster %d: %d ambiguous "
                               "members on this shard, %d declared"
                               % (cid, int(recs[rank]["n_amb"]), m_local))
        s_old = s_new = 0.0
        moved = 0
        for r in range(len(recs)):               # fixed order: deterministic
            s_old += float(recs[r]["sum_old"])
            s_new += float(recs[r]["sum_new"])
            moved |= int(recs[r]["moved"])
        accept = (s_new / n_total) < (s_old / n_total)       # kmedoids.py:683
        shard.pam_commit(accept)
        if accept:
            medoids[cid] = g
            acceptances += 1
            win.stale |= moved
    return medoids


# ---------------------------------------------------------------------------
# what the estimator-level entries below share: who holds what, agreement
# before anything can hang, the centers' rows from the ranks that hold them
# ---------------------------------------------------------------------------
def _split_indices(starts, indices):
    """Flat indices into blocks laid end to end (``starts`` [n_blocks + 1]) ->
    (block, index within it) pairs.  An index on a boundary belongs to the
    block that holds it, never to an empty block before it."""
    out = []
    for g in indices:
        b = int(np.searchsorted(starts, g, side="right") - 1)
        out.append((b, int(g) - int(starts[b])))
    return out


class _Layout:
    """Where every rank's frames / samples lie in the global order (rank r's
    follow rank r-1's), from every rank's count: ``world``, ``rank``,
    ``starts`` int64 [world + 1], ``n_total`` and this rank's [``lo``, ``hi``).
    Without a process group: one rank that holds everything."""

    def __init__(self, counts, group=None):
        self.group = group
        self.world, self.rank = _world(group)
        self.starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.n_total = int(self.starts[-1])
        self.lo = int(self.starts[self.rank])
        self.hi = int(self.starts[self.rank + 1])

    @classmethod
    def gather(cls, n_local, group=None):
        """collective: every rank says how many it holds"""
        return cls(_everyone(int(n_local), group), group)

    def pairs(self, global_indices):
        """-> (rank, local index) pairs, the reference's form of a center
        index in MPI mode (kcenters.py:375-376)"""
        return _split_indices(self.starts, global_indices)


def _rows_from_owners(which, local, lay):
    """``local[g - lay.lo]`` for every global index g of ``which``, from the
    rank that holds it: -> the rows in the order of ``which`` (copies, in the
    dtype of ``local``), the same list on every rank.  Collective."""
    mine = {k: local[g - lay.lo].copy() for k, g in enumerate(which)
            if lay.lo <= g < lay.hi}
    rows = {}
    for part in _everyone(mine, lay.group):
        rows.update(part)
    return [rows[k] for k in range(len(which))]


def _need_group(what="mpi_mode"):
    import torch.distributed as dist
    from .exception import ImproperlyConfigured
    if not (dist.is_available() and dist.is_initialized()):
        raise ImproperlyConfigured(
            "%s needs an initialised torch.distributed process group "
            "(one process per GPU, e.g. under torchrun)" % what)


def _agree_on_seed(random_state, group=None):
    """The sweeps draw member ranks from ONE stream that every rank replays
    (the reference agrees on each draw, mpi/ops.py randind): ranks that pass
    different seeds or differently positioned RandomStates would propose
    different samples and wait for each other forever, so they compare first
    and raise ImproperlyConfigured together.  None everywhere (also the global
    numpy RandomState, what the estimators make of None): rank 0's draw for
    all.  Without a process group there is nobody to agree with.
    -> RandomState; for an int seed or identically seeded RandomStates exactly
    ``check_random_state(random_state)``"""
    import hashlib
    import torch.distributed as dist
    from .cluster.kcenters import check_random_state
    from .exception import ImproperlyConfigured
    if not (dist.is_available() and dist.is_initialized()):
        return check_random_state(random_state)
    if random_state is None or random_state is np.random.mtrand._rand:
        mark = None
    elif isinstance(random_state, (int, np.integer)):
        mark = ("seed", int(random_state))
    elif isinstance(random_state, np.random.RandomState):
        st = random_state.get_state()
        mark = ("state", hashlib.sha1(np.asarray(st[1]).tobytes()).hexdigest(),
                int(st[2]))
    else:
        mark = ("other", repr(random_state))
    draw = int(np.random.SeedSequence().entropy % (2 ** 31 - 1))
    everyone = _everyone((mark, draw), group)
    if len(set(m for m, _ in everyone)) != 1:
        raise ImproperlyConfigured(
            "the ranks disagree on random_state (%s): the sharded PAM sweep "
            "needs the same seed, or identically seeded RandomStates, on "
            "every rank" % ", ".join(
                "rank %d: %s" % (r, "None" if m is None else m[0] + " " +
                                 str(m[1])[:12]) for r, (m, _) in
                enumerate(everyone)))
    if mark is None:
        return check_random_state(everyone[0][1])
    return check_random_state(random_state)


def _raise_together(err, agree, what, group=None):
    """A rank raising alone would leave the others waiting in the next
    collective, so every check of a rank's own arguments ends here: ``err`` is
    None or this rank's (exception class, message), ``agree`` what all ranks
    must have in common (``what`` names its fields).  If any rank has an error
    EVERY rank raises the first one's class with all the messages; if they
    disagree every rank raises ImproperlyConfigured.  Without a process group
    the exception is the local one, as it is."""
    from .exception import ImproperlyConfigured
    world, _ = _world(group)
    said = _everyone((err, agree), group)
    bad = [(r, e) for r, (e, _) in enumerate(said) if e is not None]
    if bad and world == 1:
        raise err[0](err[1])
    if bad:
        raise bad[0][1][0]("; ".join(
            m if m.startswith("rank ") else "rank %d: %s" % (r, m)
            for r, (_, m) in bad))
    if len(set(a for _, a in said)) != 1:
        raise ImproperlyConfigured(
            "the ranks disagree on %s: %s" % (what, ", ".join(
                "rank %d: %s" % (r, a) for r, (_, a) in enumerate(said))))


def _cluster_result(shard, pairs, centers):
    """the ClusterResult of the reference's MPI mode: ``center_indices`` as
    (rank, local index) pairs, this rank's labels (int64) and distances
    (float64) from the shard, the centers' rows, the same on every rank"""
    from .cluster import util
    d, a = shard.state()
    return util.ClusterResult(
        center_indices=pairs, assignments=np.asarray(a).astype(np.int64),
        distances=np.asarray(d, dtype=np.float64), centers=centers)


def _kcenters_then_pam(shard, med, max_new, dist_cutoff, n_iters, rs, group,
                       use_triangle_inequality=False):
    """Up to ``max_new`` k-centers iterations after the centers ``med`` already
    there (a warm start's, or none), then ``n_iters`` PAM sweeps drawing from
    the RandomState ``rs``, over all ranks' shards (reference hybrid.py:112-162
    in MPI mode).  -> (the medoids' global indices, how many k-centers added);
    labels and distances stay on the shards."""
    idx, _ = kcenters_sharded(shard, len(med), max_new,
                              float(dist_cutoff or 0.0), group=group,
                              use_triangle_inequality=use_triangle_inequality)
    med = list(med) + [int(g) for g in idx]
    for _ in range(int(n_iters)):
        med = pam_sweep_sharded(shard, med, random_state=rs, group=group)
    return med, len(idx)


def _fit_on_shard(shard, local, lay, med, max_new, dist_cutoff, n_iters, rs,
                  init_centers=(), use_triangle_inequality=False):
    """:func:`_kcenters_then_pam` and its :func:`_cluster_result`: ``centers``
    = the rows of ``local`` the centers are, from the ranks that hold them.
    k-centers alone (no sweep) returns ``init_centers``, the warm start's
    centers as the caller gave them, followed by the new ones."""
    med, n_new = _kcenters_then_pam(shard, med, max_new, dist_cutoff, n_iters,
                                    rs, lay.group, use_triangle_inequality)
    if int(n_iters) > 0:                # every center is a medoid of the data
        init_centers, n_new = (), len(med)
    return _cluster_result(
        shard, lay.pairs(med), list(init_centers) +
        _rows_from_owners(med[len(med) - n_new:], local, lay))


def khybrid_sharded(shard, n_clusters, dist_cutoff=0.0, n_iters=5,
                    random_state=None, group=None):
    """k-centers then ``n_iters`` PAM sweeps over all ranks' ready shards
    (:func:`_kcenters_then_pam`).  ``random_state`` is wrapped once, so an int
    seed gives one stream across the sweeps -- what the KHybrid estimator does
    (hybrid.py:78,103) -- and has to be the same on every rank
    (:func:`_agree_on_seed`).  Returns the medoids' global frame indices;
    labels and distances stay on the shards."""
    rs = _agree_on_seed(random_state, group)
    if n_clusters is None or np.isinf(n_clusters):
        # cut-off only: same cap as the single-GPU path (cluster/kcenters.py)
        n_clusters = 2 * _Layout.gather(shard.n_local, group).n_total + 16
    return _kcenters_then_pam(shard, [], int(n_clusters), dist_cutoff, n_iters,
                              rs, group)[0]


# ---------------------------------------------------------------------------
# k-medoids across shards with a warm start (reference kmedoids.py, MPI mode)
# ---------------------------------------------------------------------------
def ctr_ids_mpi(cluster_center_inds, lengths, world):
    """The reference's ``ctr_ids_mpi`` (kmedoids.py:365-407): cluster centers
    given with respect to ALL data -- flat frame indices into the
    concatenation of all trajectories, or (global trajectory, frame) pairs --
    -> (rank, index into that rank's concatenated frames) pairs, for the
    reference's distribution of trajectories over ranks: trajectory t lives on
    rank ``t % world`` (mpi/io.py:126, load_trajectory_as_striped), a rank's
    frames are its trajectories t = rank, rank + world, .. one after the
    other.  A pure function of ``world`` (the reference reads mpi.size())."""
    lengths = [int(v) for v in lengths]
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if len(cluster_center_inds) == 0:
        return []
    pairs = cluster_center_inds
    if not hasattr(cluster_center_inds[0], "__len__"):
        # [global frame index, ...] -> [[global trajectory, frame], ...]
        for c in cluster_center_inds:
            if int(c) < 0 or int(c) >= starts[-1]:
                raise IndexError("cluster center index %d outside the %d frames "
                                 "X_lengths describes" % (c, int(starts[-1])))
        pairs = _split_indices(starts, [int(c) for c in cluster_center_inds])
    out = []
    for t, f in pairs:
        t, f = int(t), int(f)
        if t < 0 or t >= len(lengths) or f < 0 or f >= lengths[t]:
            raise IndexError("cluster center (%d, %d) outside X_lengths" % (t, f))
        r = t % world
        owned = lengths[r::world]
        out.append((r, int(sum(owned[:t // world])) + f))
    return out


def _frames_to_medoids(shard, rows):
    shard.assign_nearest(np.array(rows, dtype=np.float32))
    # the centers were the medoid frames themselves: every frame's distance is
    # the distance to the medoid its label names
    if hasattr(shard, "set_exact"):
        shard.set_exact(True)


def _samples_to_medoids(shard, rows):
    _assign_shard_to_centers(shard, rows, shard.n_local)


# What the k-medoids start has to know about the data it runs on: what the
# messages call it; whether a warm start needs X_lengths (the reference's rule
# for frames, kmedoids.py:264-283; samples may also come as flat indices in rank
# order); the cold start's assignment, (shard, the medoids' rows) -> every row
# of the shard to its nearest (strict <, the lowest label on ties).
_Kind = collections.namedtuple("_Kind", "what lengths_required to_medoids")
_FRAMES = _Kind("frames", True, _frames_to_medoids)
_SAMPLES = _Kind("samples", False, _samples_to_medoids)


def _kmedoids_on_shard(shard, local, lay, kind, n_clusters=None, n_iters=5,
                       assignments=None, distances=None,
                       cluster_center_inds=None, X_lengths=None, proposals=None,
                       random_state=None):
    """k-medoids over all ranks' shards, the reference's MPI mode
    (kmedoids.py:133-146 dispatch, :225-283 ``_kmedoids_inputs_tree_mpi``,
    :365-407 ``ctr_ids_mpi``, sweeps :410-476 / :575-699), for frames and
    feature samples alike (``kind``); ``local`` holds this rank's rows.

    Warm start: this rank's ``assignments`` / ``distances`` and the same
    ``cluster_center_inds`` on every rank.  With ``X_lengths`` (the lengths of
    ALL trajectories, striped over the ranks t % world) they are flat indices
    into the concatenation of all trajectories or (trajectory, frame) pairs
    (:func:`ctr_ids_mpi`); without it, where the kind allows that, flat
    indices in the ranks' order (rank r's after rank r-1's).  Supplying only
    some of the three raises the reference's ImproperlyConfigured.  Cold start
    (none of the three; the reference's own branch, :247-262, cannot run --
    ``np.arange(X)``, ``.append`` on None): ``n_clusters`` distinct indices
    drawn over ALL ranks' data from a seeded ``np.random.default_rng`` like the
    single-process path (kmedoids.py:345-352), then everything to its nearest.

    ``proposals``: (rank, local index) pairs, one per cluster (:581-623).
    Every check that can fail on one rank alone is exchanged first, so that all
    ranks raise together (:func:`_raise_together`), and the ranks agree on one
    random stream for the cold start's draw and the sweeps' draws
    (:func:`_agree_on_seed`).  -> ClusterResult, ``centers`` = the medoids'
    rows of ``local`` on every rank.  Collective: every rank calls it."""
    from .exception import DataInvalid, ImproperlyConfigured
    n_local = lay.hi - lay.lo
    given = [assignments is not None, distances is not None,
             cluster_center_inds is not None]
    warm = all(given)
    err = None                  # (exception class, message)
    med, d0, a0 = None, None, None
    if any(given) and not warm:
        err = (ImproperlyConfigured,
               "For KMedoids, MPI mode can start from scratch without "
               "assignments, distances, or cluster_center_inds. "
               "Or, it requires that all are supplied.")
    elif not warm and n_clusters is None:
        err = (ImproperlyConfigured,
               "Must provide n_clusters or cluster_center_inds, assignments,"
               "and distances for KMedoids in MPI mode.")
    elif warm:
        try:
            if X_lengths is None and kind.lengths_required:
                raise ImproperlyConfigured(
                    "If cluster_center_inds is given with respect to all data "
                    "then X_lengths (the lengths of ALL trajectories) also "
                    "needs to be supplied")
            if X_lengths is not None:
                mine_len = sum(int(v) for v in X_lengths[lay.rank::lay.world])
                if mine_len != n_local:
                    raise DataInvalid(
                        "rank %d holds %d %s, but the trajectories X_lengths "
                        "gives it (t %% %d == %d) have %d"
                        % (lay.rank, n_local, kind.what, lay.world, lay.rank,
                           mine_len))
                med = [int(lay.starts[r]) + i for r, i in
                       ctr_ids_mpi(cluster_center_inds, X_lengths, lay.world)]
            elif hasattr(cluster_center_inds[0], "__len__"):
                raise ImproperlyConfigured(
                    "If cluster_center_inds is given as [[global_traj_id, "
                    "frame_id],...] then X_lengths also needs to be supplied")
            else:
                med = [int(g) for g in cluster_center_inds]
                if min(med) < 0 or max(med) >= lay.n_total:
                    raise IndexError("cluster center index outside the %d %s "
                                     "of all ranks" % (lay.n_total, kind.what))
            d0 = np.asarray(distances, dtype=np.float64)
            a0 = np.asarray(assignments)
            if len(d0) != n_local or len(a0) != n_local:
                raise DataInvalid(
                    "%d assignments / %d distances for %d %s"
                    % (len(a0), len(d0), n_local, kind.what))
            mine = [g - lay.lo for g in med if lay.lo <= g < lay.hi]
            # the medoids must sit at (numerically) zero distance
            # (kmedoids.py:185-187)
            if not np.all(d0[mine] < 0.001):
                raise DataInvalid(
                    "cluster_center_inds name %s that are not at distance 0 "
                    "from their cluster's center (max %g)"
                    % (kind.what, float(np.max(d0[mine]))))
        except (DataInvalid, ImproperlyConfigured, IndexError) as e:
            err = (type(e), str(e))
    K = (len(med) if med is not None else
         (int(n_clusters) if n_clusters is not None else 0))
    if err is None and proposals is not None:
        if len(proposals) != K:
            err = (DataInvalid,
                   "Length of 'proposals' didn't match length of 'medoid_inds' "
                   "({} != {}).".format(len(proposals), K))
        elif not hasattr(proposals[0], "__len__"):
            err = (DataInvalid,
                   "Depth of 'proposals' didn't match 'medoid_inds' "
                   "(proposals[0] == {}, whereas medoid_inds[0] == {})".format(
                       proposals[0], (0, 0)))
    _raise_together(err, (warm, K, proposals is not None, int(n_iters)),
                    "the start (warm, clusters, proposals given, n_iters)",
                    lay.group)
    # one random_state for all: the cold start's draw of the medoids and the
    # sweeps' draws of members both have to be the same on every rank
    rs = _agree_on_seed(random_state, lay.group)
    if warm:
        shard.set_state(d0, a0.astype(np.int32))
    else:
        seed = random_state
        if not isinstance(seed, (int, np.integer)):
            seed = rs.randint(0, 2 ** 31 - 1)       # (the agreed stream's)
        rng = np.random.default_rng(seed=int(seed))
        med = np.array([])
        while len(np.unique(med)) < int(n_clusters):
            med = rng.integers(0, lay.n_total, int(n_clusters))
        med = [int(g) for g in med]
        kind.to_medoids(shard, _rows_from_owners(med, local, lay))
    prop = None
    if proposals is not None:
        prop = [int(lay.starts[int(r)]) + int(i) for r, i in proposals]
    for _ in range(int(n_iters)):
        med = pam_sweep_sharded(shard, med, proposals=prop, random_state=rs,
                                group=lay.group)
    return _cluster_result(shard, lay.pairs(med),
                           _rows_from_owners(med, local, lay))


def kmedoids_sharded(shard, xyz_local, n_iters=5, assignments=None,
                     distances=None, cluster_center_inds=None, X_lengths=None,
                     proposals=None, random_state=None, n_clusters=None,
                     group=None):
    """k-medoids with metric RMSD over all ranks' ready shards, see
    :func:`_kmedoids_on_shard`: every rank passes the ``assignments`` /
    ``distances`` of ITS frames ``xyz_local``; a warm start needs ``X_lengths``.
    Returns (medoids as (rank, local index) pairs, centers float32 [K, A, 3]);
    labels and distances stay on the shard.  Works without a process group."""
    A = shard.n_atoms
    xyz_local = np.asarray(xyz_local, dtype=np.float32).reshape(-1, A, 3)
    res = _kmedoids_on_shard(
        shard, xyz_local, _Layout.gather(shard.n_local, group), _FRAMES,
        n_clusters=n_clusters, n_iters=n_iters, assignments=assignments,
        distances=distances, cluster_center_inds=cluster_center_inds,
        X_lengths=X_lengths, proposals=proposals, random_state=random_state)
    return res.center_indices, np.array(res.centers, dtype=np.float32).reshape(
        len(res.centers), A, 3)


# ---------------------------------------------------------------------------
# estimator-level entry: the reference's mpi_mode
# ---------------------------------------------------------------------------
@contextlib.contextmanager
def _device_frame_shard(xyz, offset):
    """The product's shard for RMSD: a FrameStore holding ``xyz`` on a torch
    stream of its own on the current CUDA device, state reset, the driver
    running under that stream."""
    import torch
    from .device import FrameStore
    device = torch.cuda.current_device()
    tstream = torch.cuda.Stream(device=device)
    with FrameStore(int(xyz.shape[0]), int(xyz.shape[1]), device=device,
                    global_offset=int(offset),
                    stream=tstream.cuda_stream) as store:
        store.load(xyz)
        store.reset_state()
        with torch.cuda.stream(tstream):
            yield DeviceShard(store)


def kmedoids_fit_sharded(traj, n_clusters=None, n_iters=5, assignments=None,
                         distances=None, cluster_center_inds=None,
                         X_lengths=None, proposals=None, random_state=None,
                         group=None, make_shard=None):
    """``kmedoids()`` / ``KMedoids.fit`` when the process group has more than one
    rank (the reference decides by ``mpi.size() > 1``, kmedoids.py:172): every
    rank passes ITS OWN frames (the trajectories t % world == rank, one after
    the other), see :func:`_kmedoids_on_shard`.  One process per GPU; the
    current CUDA device holds the shard (``make_shard(xyz, offset)`` -> a
    context manager yielding another one: tests plug in a host shard).
    Returns a ClusterResult like the reference's MPI mode: ``center_indices``
    as (rank, local frame index) pairs, this rank's ``assignments`` /
    ``distances``, the medoids' coordinates on every rank."""
    from .device import as_xyz
    _need_group()
    xyz = as_xyz(traj)
    lay = _Layout.gather(len(xyz), group)
    with (make_shard or _device_frame_shard)(xyz, lay.lo) as shard:
        return _kmedoids_on_shard(
            shard, xyz, lay, _FRAMES, n_clusters=n_clusters, n_iters=n_iters,
            assignments=assignments, distances=distances,
            cluster_center_inds=cluster_center_inds, X_lengths=X_lengths,
            proposals=proposals, random_state=random_state)


def fit_sharded(traj, n_clusters=None, dist_cutoff=0.0, n_iters=0,
                random_state=None, group=None, use_triangle_inequality=False,
                init_centers=None, make_shard=None):
    """k-centers (+ ``n_iters`` PAM sweeps) where every rank of the initialised
    ``torch.distributed`` group passes ITS OWN frames -- what ``mpi_mode=True``
    means in the reference (kcenters.py:314-378, kmedoids.py MPI branch): rank
    r's frames follow rank r-1's in the global order, ties go to the lowest
    rank.  One process per GPU; the current CUDA device holds the shard
    (``make_shard``: as for :func:`kmedoids_fit_sharded`).

    Returns a ClusterResult like the reference's MPI mode: ``center_indices``
    as (rank, local frame index) pairs (kcenters.py:375-376), ``assignments`` /
    ``distances`` for this rank's frames, ``centers`` = the centers'
    coordinates (float32 [A, 3] each), the same list on every rank.
    ``random_state`` and ``init_centers`` (a warm start, kcenters.py:200-206:
    see ``warm_start_sharded``) must be the same on every rank; the sweeps'
    random stream is agreed on first (:func:`_agree_on_seed`)."""
    from .device import as_xyz
    from .exception import ImproperlyConfigured
    _need_group()
    xyz = as_xyz(traj)
    A = int(xyz.shape[1])
    lay = _Layout.gather(len(xyz), group)
    if lay.n_total == 0:
        raise ValueError("cannot cluster an empty trajectory")
    if n_clusters is None or np.isinf(n_clusters):
        if not dist_cutoff:
            raise ImproperlyConfigured("Either n_clusters or cluster_radius "
                                       "is required for KHybrid clustering")
        max_new = 2 * lay.n_total + 16
    else:
        max_new = int(n_clusters)
    rs = _agree_on_seed(random_state, group) if int(n_iters) > 0 else None
    kept = ()
    if init_centers is not None and int(n_iters) == 0:
        # k-centers alone returns the caller's initial centers followed by the
        # new ones (kcenters.py:200-240: `centers` starts as init_centers, and
        # the labels and distances of a warm start are measured to THEM), as the
        # single-process path does; `center_indices` stays the occupied labels'
        # closest members + the new centers' frames (kcenters.py:205).  (An
        # initial center that attracts no frame leaves `center_indices` shorter
        # than `centers` and the new labels start at len(center_indices),
        # kcenters.py:306: the reference's own misalignment, reproduced like the
        # single-process path does)
        kept = [np.asarray(as_xyz(c_)[0] if np.ndim(c_) == 3 else c_,
                           dtype=np.float32).reshape(A, 3).copy()
                for c_ in init_centers]
    with (make_shard or _device_frame_shard)(xyz, lay.lo) as shard:
        med = []
        if init_centers is not None:
            med = warm_start_sharded(shard, init_centers, group=group)
            # (the shards' tables of accepted centers would lack these: the
            # tile skip is an optimisation only, results do not change)
            use_triangle_inequality = False
        return _fit_on_shard(shard, xyz, lay, med, max(0, max_new - len(med)),
                             dist_cutoff, n_iters, rs, kept,
                             use_triangle_inequality)


# ---------------------------------------------------------------------------
# feature metrics in mpi_mode (euclidean / manhattan / hamming on 2-D samples)
# ---------------------------------------------------------------------------
METRIC_NAMES = {0: "euclidean", 1: "manhattan", 2: "hamming"}


def _feature_data_problem(X, metric_id):
    """None if the k-centers loop can run on these samples on the device (what
    the single-process path's ``resident`` test accepts, cluster/kcenters.py:
    a 2-D ndarray of floating-point values other than float16 without NaN, or
    of integers; hamming: integers only), else what is wrong with them."""
    if not isinstance(X, np.ndarray) or X.ndim != 2:
        return "the samples must be a 2-D numpy array (got %s)" % (
            "shape %s" % (X.shape,) if isinstance(X, np.ndarray)
            else type(X).__name__)
    if X.shape[1] < 1:
        return "the samples have no features"
    integer = np.issubdtype(X.dtype, np.integer)
    if metric_id == 2:
        return None if integer else (
            "hamming distance needs integer samples, got %s" % X.dtype)
    if integer:
        return None
    if not np.issubdtype(X.dtype, np.floating) or X.dtype == np.float16:
        return "samples of dtype %s" % X.dtype
    if np.isnan(X).any():
        return "the samples contain NaN"
    return None


def _assign_shard_to_centers(shard, centers, n_local):
    """util.assign_to_nearest_center (util.py:199-203) of the shard's samples
    to ``centers`` as the shard's state: label 0 / +inf, then every center in
    order, strict <.  A device shard does the scan in one launch and keeps the
    result where the steps that follow read it; a shard object without
    ``assign_nearest`` gets the per-center loop around its ``distance``.
    -> (distances float64, labels int32) on the host"""
    if hasattr(shard, "assign_nearest"):
        return shard.assign_nearest(centers)
    d = np.full(n_local, np.inf, dtype=np.float64)
    a = np.zeros(n_local, dtype=np.int32)
    for i, c in enumerate(centers):
        dc = shard.distance(np.asarray(c))
        closer = dc < d
        d[closer] = dc[closer]
        a[closer] = i
    shard.set_state(d, a)
    return d, a


@contextlib.contextmanager
def _device_feature_shard(Xw, metric_id, offset):
    """The product's shard: a FeatureStore on a torch stream of its own on the
    current CUDA device, the driver running under that stream."""
    import torch
    from .geometry.libdist import FeatureStore
    device = torch.cuda.current_device()
    tstream = torch.cuda.Stream(device=device)
    with FeatureStore.from_array(Xw, metric_id, device=device,
                                 global_offset=offset,
                                 stream=tstream.cuda_stream) as store:
        with torch.cuda.stream(tstream):
            yield FeatureShard(store, metric_id)


_PAM_WHAT = "the sharded PAM sweep"


def _agree_on_samples(X, metric_id, group, what="mpi_mode"):
    """The pre-loop agreement of the feature drivers: the ranks compare
    (n_features, dtype, metric, data usable) and raise TOGETHER, see
    :func:`fit_features_sharded`.  -> the :class:`_Layout` of the samples"""
    from .exception import DataInvalid, ImproperlyConfigured
    _need_group(what)
    if metric_id not in METRIC_NAMES:
        raise ImproperlyConfigured("not a device feature metric: %r"
                                   % (metric_id,))
    problem = _feature_data_problem(X, metric_id)
    mine = (int(X.shape[0]) if problem is None else 0,
            int(X.shape[1]) if problem is None else -1,
            str(X.dtype) if problem is None else "", int(metric_id), problem)
    everyone = _everyone(mine, group)
    bad = [(r, e[4]) for r, e in enumerate(everyone) if e[4] is not None]
    if bad:
        raise DataInvalid(
            "mpi_mode with metric '%s' cannot run on these samples: %s"
            % (METRIC_NAMES[metric_id],
               "; ".join("rank %d: %s" % b for b in bad)))
    if len(set(e[1:4] for e in everyone)) != 1:
        raise ImproperlyConfigured(
            "the ranks disagree on (n_features, dtype, metric): %s"
            % ", ".join("rank %d: (%d, %s, %s)"
                        % (r, e[1], e[2], METRIC_NAMES.get(e[3], e[3]))
                        for r, e in enumerate(everyone)))
    lay = _Layout([e[0] for e in everyone], group)
    if lay.n_total == 0:
        raise ValueError("cannot cluster an empty set of samples")
    return lay


def fit_features_sharded(X, metric_id, n_clusters=None, dist_cutoff=0.0,
                         init_centers=None, group=None, make_shard=None,
                         n_iters=0, random_state=None):
    """k-centers with a feature metric (``metric_id`` 0 euclidean, 1 manhattan,
    2 hamming) where every rank of the initialised ``torch.distributed`` group
    passes ITS OWN samples, a 2-D array [n_local, n_features] (n_local may be
    0) -- ``mpi_mode=True`` of the reference (kcenters.py:314-378) for these
    metrics: rank r's samples follow rank r-1's in the global order, ties go to
    the lowest rank, the result is the single-process one.

    Returns a ClusterResult like :func:`fit_sharded`: ``center_indices`` as
    (rank, local index) pairs, this rank's ``assignments`` (int64) /
    ``distances`` (float64), ``centers`` = the centers' feature rows in X's
    dtype, the same list on every rank.  ``init_centers`` (the same rows on
    every rank) is the warm start of kcenters.py:200-206 by the rule of
    :func:`warm_start_sharded`; ``centers`` / ``center_indices`` then follow
    the single-process path (the initial centers, then the new rows; occupied
    labels' closest members, then the new samples).

    ``n_iters`` > 0: that many PAM sweeps follow (k-hybrid, hybrid.py:112-162
    in MPI mode; :func:`pam_sweep_sharded` over the shard's ``pam_*`` methods),
    one random stream across them from ``random_state`` -- the same int seed or
    identically seeded RandomState on every rank (:func:`_agree_on_seed`);
    ``centers`` are then the medoids' rows.  A cluster without members makes
    ``RandomState.choice`` raise on every rank in the same proposal.

    The ranks first compare (n_features, dtype, metric, data usable): on a
    disagreement EVERY rank raises ImproperlyConfigured, on unusable samples
    anywhere EVERY rank raises DataInvalid -- a rank raising alone would leave
    the others waiting in the next collective.  ``make_shard(X, metric_id,
    offset)`` -> a context manager yielding the shard (tests plug in a
    numpy-backed one); the default puts the samples on the current CUDA
    device."""
    lay = _agree_on_samples(X, metric_id, group,
                            _PAM_WHAT if n_iters else "mpi_mode")
    rs = _agree_on_seed(random_state, group) if int(n_iters) > 0 else None
    with (make_shard or _device_feature_shard)(X, metric_id, lay.lo) as shard:
        if init_centers is None:
            centers, med = [], []
            shard.reset_state()
        else:
            centers = [c for c in init_centers]
            d, a = _assign_shard_to_centers(shard, centers, lay.hi - lay.lo)
            med = _closest_members(d, a, lay.lo, len(centers), group)
        budget = (np.inf if n_clusters is None else n_clusters) - len(med)
        max_new = (0 if budget <= 0 else
                   (2 * lay.n_total + 16 if np.isinf(budget) else int(budget)))
        return _fit_on_shard(shard, X, lay, med, max_new, dist_cutoff, n_iters,
                             rs, centers)


def kmedoids_features_sharded(X, metric_id, n_clusters=None, n_iters=5,
                              assignments=None, distances=None,
                              cluster_center_inds=None, X_lengths=None,
                              proposals=None, random_state=None, group=None,
                              make_shard=None):
    """``kmedoids()`` / ``KMedoids.fit`` in mpi_mode for a feature metric
    (``metric_id`` 0 euclidean, 1 manhattan, 2 hamming): every rank passes ITS
    OWN samples [n_local, n_features], the counterpart of
    :func:`kmedoids_fit_sharded` for RMSD with the same two starts
    (:func:`_kmedoids_on_shard`); a warm start may also name its medoids
    without ``X_lengths``, as flat indices in the ranks' order.  Returns a
    ClusterResult shaped like :func:`fit_features_sharded`'s."""
    lay = _agree_on_samples(X, metric_id, group, _PAM_WHAT)
    with (make_shard or _device_feature_shard)(X, metric_id, lay.lo) as shard:
        return _kmedoids_on_shard(
            shard, X, lay, _SAMPLES, n_clusters=n_clusters, n_iters=n_iters,
            assignments=assignments, distances=distances,
            cluster_center_inds=cluster_center_inds, X_lengths=X_lengths,
            proposals=proposals, random_state=random_state)

