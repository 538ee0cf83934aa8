// ek_feat_kcenters.hip -- k-centers in feature space: the loop resident on one
// device, and the step of a run over several shards.
#include "ek_feat.h"

#include <algorithm>

// ===========================================================================
// k-centers in feature space, resident on the device
// ===========================================================================
// Reference: the loop of enspara/cluster/kcenters.py:217-231 with the serial
// iteration :243-311 for metrics 'euclidean' / 'manhattan' (libdist.pyx) --
//   new_index = argmax(distances); dist = metric(X, X[new_index]);
//   closer = dist < distances; distances[closer] = dist[closer]; assignments[closer] = k;
//   maxdist = distances.max()
// -- which costs a metric call plus six numpy passes over n and an arg-max on the
// host per center when only the metric runs on the device.  Here the float64
// distances and the labels stay in HBM: one launch computes the new center's
// distances (the arithmetic of feat_distance_kernel, bit for bit), applies the
// strict-< update and leaves per-workgroup (max, first index) partials; a
// single-workgroup launch reduces them, applies the stop rule, and copies the
// next center's features out of the tiles.  No host round trip per center.
// sample f's finished distance to the new center against the one it has: the
// strict-< update (kcenters.py:304), and what the sample hands to the arg-max
// (lanes past n: a pair that never wins)
template <int METRIC>
__device__ __forceinline__ void feat_kcenters_update(double acc, int F, int64_t f, int64_t n,
                                                     int32_t label, double *__restrict__ dist,
                                                     int32_t *__restrict__ assign, double &v,
                                                     int64_t &i)
{
    v = -__builtin_inf();
    i = 0x7fffffffffffffffLL;
    if (f < n) {
        acc = feat_finish<METRIC>(acc, F);
        double cur = dist[f];
        if (acc < cur) {
            cur = acc;
            dist[f] = acc;
            assign[f] = label;
        }
        v = cur;
        i = f;
    }
}

template <typename T, int METRIC>
__global__ void __launch_bounds__(EK_BLOCK)
feat_step_kernel(const T *__restrict__ tiles, const T *__restrict__ y, int64_t n,
                 int F, int32_t label, double *__restrict__ dist,
                 int32_t *__restrict__ assign, FeatBlockMax *__restrict__ bm,
                 FeatCtl *__restrict__ ctl, int64_t *__restrict__ hist)
{
    __shared__ T ys[FY_CHUNK];
    if (ctl->stopped)
        return;
    const int64_t f = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    const double acc = feat_one_vs_all<T, METRIC>(feat_tile_ptr(tiles, f, F), y, F, ys);
    double v;
    int64_t i;
    feat_kcenters_update<METRIC>(acc, F, f, n, label, dist, assign, v, i);
    feat_block_partial(v, i, bm);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        hist[label] = ctl->next;            // the sample this center is
        ctl->n_done = ctl->n_done + 1;
    }
}

// per-workgroup partials of the state as it stands (before the first step)
__global__ void __launch_bounds__(EK_BLOCK)
feat_blockmax_kernel(const double *__restrict__ dist, int64_t n,
                     FeatBlockMax *__restrict__ bm)
{
    const int64_t f = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    double v = -__builtin_inf();
    int64_t i = 0x7fffffffffffffffLL;
    if (f < n) {
        v = dist[f];
        i = f;
    }
    feat_block_partial(v, i, bm);
}

// np.argmax / distances.max() (kcenters.py:282, :226), the stop rule (:217) and
// the next center's features, contiguous in y
template <typename T>
__global__ void __launch_bounds__(1024)
feat_pick_kernel(const FeatBlockMax *__restrict__ bm, int nb,
                 const T *__restrict__ tiles, int F, double cutoff,
                 T *__restrict__ y, FeatCtl *__restrict__ ctl)
{
    __shared__ double rv[1024 / EK_WAVE];
    __shared__ int64_t ri[1024 / EK_WAVE];
    __shared__ int64_t win;
    if (ctl->stopped)
        return;
    const int tid = threadIdx.x;
    double v = -__builtin_inf();
    int64_t i = 0x7fffffffffffffffLL;
    for (int b = tid; b < nb; b += 1024) {
        const FeatBlockMax m = bm[b];
        if (feat_better(m.val, m.idx, v, i)) {
            v = m.val;
            i = m.idx;
        }
    }
    feat_wave_argmax(v, i);
    feat_slots_put(v, i, rv, ri);
    if (tid == 0) {
        feat_slots_best(v, i, rv, ri);
        ctl->last_max = v;
        if (!(v > cutoff))
            ctl->stopped = 1;
        ctl->next = i;
        win = (v > cutoff) ? i : -1;
    }
    __syncthreads();
    const int64_t c = win;
    if (c < 0)
        return;
    feat_copy_row(y, 1, feat_tile_ptr(tiles, c, F), F, 1024);
}

template <typename T> static void feat_enqueue_pick(ek_feat *k, int nb, double cutoff)
{
    hipLaunchKernelGGL((feat_pick_kernel<T>), dim3(1), dim3(1024), 0, k->s, k->bm, nb,
                       (const T *)k->tiles, k->F, cutoff, (T *)k->y, k->ctl);
}

// `count` centers with labels label0, label0 + 1, ..: two launches each
template <typename T, int M>
static void feat_enqueue_steps(ek_feat *k, int nb, int32_t label0, int32_t count, double cutoff)
{
    for (int32_t t = 0; t < count; ++t) {
        hipLaunchKernelGGL((feat_step_kernel<T, M>), dim3((unsigned)nb), dim3(EK_BLOCK), 0,
                           k->s, (const T *)k->tiles, (const T *)k->y, k->n, k->F, label0 + t,
                           k->kdist, k->kassign, k->bm, k->ctl, k->hist);
        feat_enqueue_pick<T>(k, nb, cutoff);
    }
}

int feat_state_alloc(ek_feat *k)
{
    // (each on its own: a call that failed part-way leaves the ones it got with the
    // handle, and the next call must not take the first for all four)
    const size_t n1 = (size_t)std::max<int64_t>(k->n, 1);
    const size_t nb = (n1 + EK_BLOCK - 1) / EK_BLOCK;
    if (!k->kdist)
        FE_HIP(ek_dev_malloc((void **)&k->kdist, n1 * sizeof(double)));
    if (!k->kassign)
        FE_HIP(ek_dev_malloc((void **)&k->kassign, n1 * sizeof(int32_t)));
    if (!k->bm)
        FE_HIP(ek_dev_malloc((void **)&k->bm, nb * sizeof(FeatBlockMax)));
    if (!k->ctl)
        FE_HIP(ek_dev_malloc((void **)&k->ctl, sizeof(FeatCtl)));
    return EK_OK;
}

// Runs up to max_new iterations from the state (dist_io, assign_io) the caller
// passes in (float64 distances, int32 labels; a fresh run passes +inf / -1) with
// labels first_label, first_label + 1, ..; writes the state back, the samples
// chosen as centers to centers_out[0..*n_added) and distances.max() after the
// last update to *final_max.
extern "C" int ek_feat_kcenters(ek_feat *k, int32_t metric, int32_t first_label,
                                int32_t max_new, double dist_cutoff,
                                double *dist_io, int32_t *assign_io,
                                int64_t *centers_out, int32_t *n_added,
                                double *final_max)
{
    if (!k || !dist_io || !assign_io || !n_added || metric < 0 || metric > 2 ||
        first_label < 0 || max_new < 0)
        return ek_set_error(EK_EARG, "ek_feat_kcenters: bad argument");
    if (!k->loaded)
        return ek_set_error(EK_ESTATE, "ek_feat_kcenters: no samples loaded");
    if (int rc = feat_metric_ok(k, metric, "ek_feat_kcenters"))
        return rc;
    *n_added = 0;
    if (k->n == 0)
        return EK_OK;
    FE_HIP(hipSetDevice(k->device));
    const int nb = (int)((k->n + EK_BLOCK - 1) / EK_BLOCK);
    if (int rc = feat_state_alloc(k))
        return rc;
    if (first_label + max_new + 1 > k->hist_cap) {
        FE_HIP(hipStreamSynchronize(k->s));
        (void)ek_dev_free(k->hist);
        k->hist = nullptr;
        k->hist_cap = 0;
        FE_HIP(ek_dev_malloc((void **)&k->hist,
                         (size_t)(first_label + max_new + 1) * sizeof(int64_t)));
        k->hist_cap = first_label + max_new + 1;
    }
    FeatCtl c0;
    c0.next = 0;
    c0.n_done = 0;
    c0.stopped = 0;
    c0.last_max = 0.0;
    FE_HIP(hipMemcpyAsync(k->ctl, &c0, sizeof(c0), hipMemcpyHostToDevice, k->s));
    FE_HIP(hipMemcpyAsync(k->kdist, dist_io, (size_t)k->n * sizeof(double),
                          hipMemcpyHostToDevice, k->s));
    FE_HIP(hipMemcpyAsync(k->kassign, assign_io, (size_t)k->n * sizeof(int32_t),
                          hipMemcpyHostToDevice, k->s));
    hipLaunchKernelGGL(feat_blockmax_kernel, dim3((unsigned)nb), dim3(EK_BLOCK), 0, k->s,
                       k->kdist, k->n, k->bm);
    feat_dispatch_type(k, [&](auto t) {
        feat_enqueue_pick<typename decltype(t)::type>(k, nb, dist_cutoff);
    });
    // with no cut-off the trip count is known: everything is enqueued at once;
    // with one, in batches, looking at the stop flag in between (steps enqueued
    // past the stopping point return at once)
    const bool open_loop = !(dist_cutoff > 0.0);
    const int32_t batch = open_loop ? max_new : 32;
    int32_t issued = 0;
    FeatCtl cr = c0;
    while (issued < max_new) {
        const int32_t todo = std::min(batch, max_new - issued);
        feat_dispatch(k, metric, [&](auto t, auto m) {
            feat_enqueue_steps<typename decltype(t)::type, decltype(m)::value>(
                k, nb, first_label + issued, todo, dist_cutoff);
        });
        FE_HIP(hipGetLastError());
        issued += todo;
        if (!open_loop) {
            FE_HIP(hipMemcpyAsync(&cr, k->ctl, sizeof(cr), hipMemcpyDeviceToHost,
                                  k->s));
            FE_HIP(hipStreamSynchronize(k->s));
            if (cr.stopped)
                break;
        }
    }
    FE_HIP(hipMemcpyAsync(&cr, k->ctl, sizeof(cr), hipMemcpyDeviceToHost, k->s));
    FE_HIP(hipMemcpyAsync(dist_io, k->kdist, (size_t)k->n * sizeof(double),
                          hipMemcpyDeviceToHost, k->s));
    FE_HIP(hipMemcpyAsync(assign_io, k->kassign, (size_t)k->n * sizeof(int32_t),
                          hipMemcpyDeviceToHost, k->s));
    FE_HIP(hipStreamSynchronize(k->s));
    *n_added = cr.n_done;
    if (final_max)
        *final_max = cr.last_max;
    if (centers_out && cr.n_done > 0) {
        FE_HIP(hipMemcpyAsync(centers_out, k->hist + first_label,
                              (size_t)cr.n_done * sizeof(int64_t),
                              hipMemcpyDeviceToHost, k->s));
        FE_HIP(hipStreamSynchronize(k->s));
    }
    return EK_OK;
}

// ===========================================================================
// k-centers in feature space over several shards (one ek_feat handle each)
// ===========================================================================
// Reference: the MPI iteration of enspara/cluster/kcenters.py:314-378 for any
// metric -- two allgathers (:332-335), the owner's arg-max (:337), a broadcast
// of the new center and the stop test (:217).  Here every shard keeps ONE
// candidate record
//   { double max_dist; int64 global_index; T row[F] }      (16-byte multiple)
// -- the maximum of its float64 distances, global_offset + the first local index
// of that maximum, that sample's features -- and the caller exchanges the records
// (one all-gather).  The step is one launch per center and shard: every
// workgroup picks the winner among the records (largest max_dist, lowest record
// index among equal ones: with contiguous shards in rank order np.argmax's first
// index over the concatenated data, :282 / :337), applies the stop rule
// `!(max > cutoff)` to it, computes metric(X_local, winner's row) with the
// arithmetic of feat_distance_kernel, applies the strict-< update and leaves its
// (max, first index) partial; the workgroup that arrives last (ek_arrive_last_tree:
// the partials cross workgroups as agent-scope relaxed atomics) reduces them and
// writes the shard's next record, row gathered from the tiles.  A shard without
// samples writes max_dist = -inf: it never wins.
extern "C" size_t ek_feat_record_bytes(int32_t n_features, int32_t elem_kind)
{
    if (n_features < 1 || elem_kind < 0 || elem_kind > 2)
        return 0;
    const size_t b = 16 + (size_t)n_features * (elem_kind == 0 ? 4 : 8);
    return (b + 15) / 16 * 16;
}

// Every workgroup hands in its (max, first local index) partial; the one that
// arrives last reduces all of them and writes the shard's record.  True in all
// threads of that workgroup.
template <typename T>
__device__ __forceinline__ bool feat_shard_finish(double v, int64_t i,
                                                  double (&rv)[EK_BLOCK / EK_WAVE],
                                                  int64_t (&ri)[EK_BLOCK / EK_WAVE],
                                                  const T *__restrict__ tiles,
                                                  int64_t n, int F, int64_t goff,
                                                  FeatBlockMax *bm, FeatShardCtl *ctl,
                                                  unsigned char *own_rec)
{
    feat_block_argmax_all(v, i, rv, ri);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&bm[blockIdx.x].val, v, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&bm[blockIdx.x].idx, i, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!ek_arrive_last_tree(&ctl->top, ctl->leaves))
        return false;
    v = -__builtin_inf();
    i = 0x7fffffffffffffffLL;
    for (unsigned int b = threadIdx.x; b < gridDim.x; b += EK_BLOCK) {
        const double ov = __hip_atomic_load(&bm[b].val, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        const int64_t oi = __hip_atomic_load(&bm[b].idx, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
        if (feat_better(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
    feat_block_argmax_all(v, i, rv, ri);
    const bool any = i < n;             // (no sample: v = -inf, no row)
    feat_copy_row((T *)(own_rec + 16), 1, feat_tile_ptr(tiles, any ? i : (int64_t)0, F), F,
                  EK_BLOCK, any);
    if (threadIdx.x == 0) {
        *(double *)own_rec = any ? v : -__builtin_inf();
        *(int64_t *)(own_rec + 8) = any ? goff + i : (int64_t)-1;
    }
    return true;
}

// the record of the state as it stands (before the first step, after a reset or
// a warm start)
template <typename T>
__global__ void __launch_bounds__(EK_BLOCK)
feat_shard_candidate_kernel(const T *__restrict__ tiles, int64_t n, int F, int64_t goff,
                            const double *__restrict__ dist, FeatBlockMax *bm,
                            FeatShardCtl *ctl, unsigned char *own_rec)
{
    __shared__ double rv[EK_BLOCK / EK_WAVE];
    __shared__ int64_t ri[EK_BLOCK / EK_WAVE];
    const int64_t f = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    double v = -__builtin_inf();
    int64_t i = 0x7fffffffffffffffLL;
    if (f < n) {
        v = dist[f];
        i = f;
    }
    feat_shard_finish<T>(v, i, rv, ri, tiles, n, F, goff, bm, ctl, own_rec);
}

// (recs and own_rec may be the same memory -- one shard, no exchange --: the last
// workgroup writes own_rec only after every workgroup has read what it needs)
template <typename T, int METRIC>
__global__ void __launch_bounds__(EK_BLOCK)
feat_shard_step_kernel(const T *__restrict__ tiles, int64_t n, int F, int64_t goff,
                       const unsigned char *recs, int n_recs, size_t rec_bytes,
                       int32_t label, double cutoff, double *__restrict__ dist,
                       int32_t *__restrict__ assign, FeatBlockMax *bm, FeatShardCtl *ctl,
                       int64_t *__restrict__ hist_idx, double *__restrict__ hist_d,
                       unsigned char *own_rec)
{
    __shared__ T ys[FY_CHUNK];
    __shared__ double rv[EK_BLOCK / EK_WAVE];
    __shared__ int64_t ri[EK_BLOCK / EK_WAVE];
    if (ctl->stopped)
        return;
    // the winner among the records: the same in every workgroup of every shard
    double wv = -__builtin_inf();
    int64_t wr = 0x7fffffffffffffffLL;
    for (int r = threadIdx.x; r < n_recs; r += EK_BLOCK) {
        const double v = *(const double *)(recs + (size_t)r * rec_bytes);
        if (feat_better(v, r, wv, wr)) {
            wv = v;
            wr = r;
        }
    }
    feat_block_argmax_all(wv, wr, rv, ri);
    if (!(wv > cutoff)) {               // kcenters.py:217 (also: no record holds a sample)
        if (blockIdx.x == 0 && threadIdx.x == 0)
            ctl->stopped = 1;
        return;
    }
    const unsigned char *win = recs + (size_t)wr * rec_bytes;
    const int64_t win_gidx = *(const int64_t *)(win + 8);
    const T *y = (const T *)(win + 16);
    const int64_t f = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    const double acc = feat_one_vs_all<T, METRIC>(feat_tile_ptr(tiles, f, F), y, F, ys);
    double v;
    int64_t i;
    feat_kcenters_update<METRIC>(acc, F, f, n, label, dist, assign, v, i);
    if (feat_shard_finish<T>(v, i, rv, ri, tiles, n, F, goff, bm, ctl, own_rec) &&
        threadIdx.x == 0) {
        hist_idx[label] = win_gidx;
        hist_d[label] = wv;
        ctl->n_done = label + 1;
    }
}

int feat_shard_alloc(ek_feat *k, int32_t label)
{
    if (int rc = feat_state_alloc(k))
        return rc;
    if (!k->sctl) {
        FE_HIP(ek_dev_malloc((void **)&k->sctl, sizeof(FeatShardCtl)));
        FE_HIP(hipMemsetAsync(k->sctl, 0, sizeof(FeatShardCtl), k->s));
    }
    if (label >= k->shist_cap) {
        int32_t cap = std::max(k->shist_cap, 1024);
        while (cap <= label)
            cap *= 2;
        int64_t *hi = nullptr;
        double *hd = nullptr;
        // (hi and hd belong to nobody until the handle takes them: every failure
        // from here on gives both back)
        hipError_t e = ek_dev_malloc((void **)&hi, (size_t)cap * sizeof(int64_t));
        if (e == hipSuccess)
            e = ek_dev_malloc((void **)&hd, (size_t)cap * sizeof(double));
        if (e == hipSuccess)
            e = hipMemsetAsync(hi, 0xff, (size_t)cap * sizeof(int64_t), k->s);
        if (e == hipSuccess)
            e = hipMemsetAsync(hd, 0, (size_t)cap * sizeof(double), k->s);
        if (e == hipSuccess && k->shist_cap)
            e = hipMemcpyAsync(hi, k->shist_idx, (size_t)k->shist_cap * sizeof(int64_t),
                               hipMemcpyDeviceToDevice, k->s);
        if (e == hipSuccess && k->shist_cap)
            e = hipMemcpyAsync(hd, k->shist_d, (size_t)k->shist_cap * sizeof(double),
                               hipMemcpyDeviceToDevice, k->s);
        if (e == hipSuccess)
            e = hipStreamSynchronize(k->s);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(k->s);
            (void)ek_dev_free(hi);
            (void)ek_dev_free(hd);
            FE_HIP(e);
        }
        (void)ek_dev_free(k->shist_idx);
        (void)ek_dev_free(k->shist_d);
        k->shist_idx = hi;
        k->shist_d = hd;
        k->shist_cap = cap;
    }
    return EK_OK;
}

__global__ void __launch_bounds__(EK_BLOCK)
feat_fill_state_kernel(double *__restrict__ dist, int32_t *__restrict__ assign, int64_t n)
{
    const int64_t f = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    if (f < n) {
        dist[f] = __builtin_inf();
        assign[f] = -1;
    }
}

extern "C" int ek_feat_history_reset(ek_feat *k)
{
    if (!k)
        return ek_set_error(EK_EARG, "ek_feat_history_reset: NULL handle");
    FE_HIP(hipSetDevice(k->device));
    int rc = feat_shard_alloc(k, 0);
    if (rc)
        return rc;
    FE_HIP(hipMemsetAsync(k->shist_idx, 0xff, (size_t)k->shist_cap * sizeof(int64_t), k->s));
    FE_HIP(hipMemsetAsync(k->shist_d, 0, (size_t)k->shist_cap * sizeof(double), k->s));
    FE_HIP(hipMemsetAsync(k->sctl, 0, sizeof(FeatShardCtl), k->s));
    return EK_OK;
}

extern "C" int ek_feat_state_reset(ek_feat *k)
{
    if (!k)
        return ek_set_error(EK_EARG, "ek_feat_state_reset: NULL handle");
    FE_HIP(hipSetDevice(k->device));
    int rc = feat_shard_alloc(k, 0);
    if (rc)
        return rc;
    if (k->n > 0) {
        hipLaunchKernelGGL(feat_fill_state_kernel,
                           dim3((unsigned)((k->n + EK_BLOCK - 1) / EK_BLOCK)), dim3(EK_BLOCK),
                           0, k->s, k->kdist, k->kassign, k->n);
        FE_HIP(hipGetLastError());
    }
    return ek_feat_history_reset(k);
}

extern "C" int ek_feat_state_upload(ek_feat *k, const double *dist_host,
                                    const int32_t *assign_host)
{
    if (!k || ((!dist_host || !assign_host) && k->n > 0))
        return ek_set_error(EK_EARG, "ek_feat_state_upload: NULL argument");
    FE_HIP(hipSetDevice(k->device));
    int rc = feat_shard_alloc(k, 0);
    if (rc)
        return rc;
    if (k->n > 0) {
        FE_HIP(hipMemcpyAsync(k->kdist, dist_host, (size_t)k->n * sizeof(double),
                              hipMemcpyHostToDevice, k->s));
        FE_HIP(hipMemcpyAsync(k->kassign, assign_host, (size_t)k->n * sizeof(int32_t),
                              hipMemcpyHostToDevice, k->s));
    }
    FE_HIP(hipStreamSynchronize(k->s));
    return EK_OK;
}

extern "C" int ek_feat_state_download(ek_feat *k, double *dist_host, int32_t *assign_host)
{
    if (!k)
        return ek_set_error(EK_EARG, "ek_feat_state_download: NULL handle");
    if (!k->kdist)
        return ek_set_error(EK_ESTATE, "ek_feat_state_download: no state on the device");
    FE_HIP(hipSetDevice(k->device));
    if (dist_host && k->n > 0)
        FE_HIP(hipMemcpyAsync(dist_host, k->kdist, (size_t)k->n * sizeof(double),
                              hipMemcpyDeviceToHost, k->s));
    if (assign_host && k->n > 0)
        FE_HIP(hipMemcpyAsync(assign_host, k->kassign, (size_t)k->n * sizeof(int32_t),
                              hipMemcpyDeviceToHost, k->s));
    FE_HIP(hipStreamSynchronize(k->s));
    return EK_OK;
}

extern "C" int ek_feat_local_candidate(ek_feat *k, void *rec_dev)
{
    if (!k || !rec_dev)
        return ek_set_error(EK_EARG, "ek_feat_local_candidate: NULL argument");
    if (!k->loaded || !k->kdist)
        return ek_set_error(EK_ESTATE, "ek_feat_local_candidate: samples and a state "
                                       "(ek_feat_state_reset / _upload) first");
    FE_HIP(hipSetDevice(k->device));
    int rc = feat_shard_alloc(k, 0);
    if (rc)
        return rc;
    const unsigned blocks = (unsigned)std::max<int64_t>((k->n + EK_BLOCK - 1) / EK_BLOCK, 1);
    feat_dispatch_size(k, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(feat_shard_candidate_kernel<T>, dim3(blocks), dim3(EK_BLOCK), 0, k->s,
                           (const T *)k->tiles, k->n, k->F, k->goff, k->kdist, k->bm, k->sctl,
                           (unsigned char *)rec_dev);
    });
    FE_HIP(hipGetLastError());
    return EK_OK;
}

extern "C" int ek_feat_kcenters_step(ek_feat *k, int32_t metric, const void *all_recs_dev,
                                     int32_t n_recs, int32_t label, double dist_cutoff,
                                     void *own_rec_dev)
{
    if (!k || !all_recs_dev || !own_rec_dev || metric < 0 || metric > 2 || n_recs < 1 ||
        label < 0)
        return ek_set_error(EK_EARG, "ek_feat_kcenters_step: bad argument");
    if (!k->loaded || !k->kdist)
        return ek_set_error(EK_ESTATE, "ek_feat_kcenters_step: samples and a state "
                                       "(ek_feat_state_reset / _upload) first");
    if (int rc = feat_metric_ok(k, metric, "ek_feat_kcenters_step"))
        return rc;
    FE_HIP(hipSetDevice(k->device));
    int rc = feat_shard_alloc(k, label);
    if (rc)
        return rc;
    const unsigned blocks = (unsigned)std::max<int64_t>((k->n + EK_BLOCK - 1) / EK_BLOCK, 1);
    const size_t rb = ek_feat_record_bytes(k->F, k->kind);
    feat_dispatch(k, metric, [&](auto t, auto m) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((feat_shard_step_kernel<T, decltype(m)::value>), dim3(blocks),
                           dim3(EK_BLOCK), 0, k->s, (const T *)k->tiles, k->n, k->F, k->goff,
                           (const unsigned char *)all_recs_dev, (int)n_recs, rb, label,
                           dist_cutoff, k->kdist, k->kassign, k->bm, k->sctl, k->shist_idx,
                           k->shist_d, (unsigned char *)own_rec_dev);
    });
    FE_HIP(hipGetLastError());
    return EK_OK;
}

extern "C" int ek_feat_history_download(ek_feat *k, int32_t first, int32_t count,
                                        int64_t *center_index_out, double *center_dist_out,
                                        int32_t *n_done)
{
    if (!k || first < 0 || count < 0)
        return ek_set_error(EK_EARG, "ek_feat_history_download: bad argument");
    FE_HIP(hipSetDevice(k->device));
    int rc = feat_shard_alloc(k, 0);
    if (rc)
        return rc;
    FeatShardCtl ctl;
    FE_HIP(hipMemcpyAsync(&ctl, k->sctl, sizeof(ctl), hipMemcpyDeviceToHost, k->s));
    const int32_t avail = std::max(0, std::min(count, k->shist_cap - first));
    if (avail > 0 && center_index_out)
        FE_HIP(hipMemcpyAsync(center_index_out, k->shist_idx + first,
                              (size_t)avail * sizeof(int64_t), hipMemcpyDeviceToHost, k->s));
    if (avail > 0 && center_dist_out)
        FE_HIP(hipMemcpyAsync(center_dist_out, k->shist_d + first,
                              (size_t)avail * sizeof(double), hipMemcpyDeviceToHost, k->s));
    FE_HIP(hipStreamSynchronize(k->s));
    for (int32_t i = avail; i < count; ++i) {
        if (center_index_out)
            center_index_out[i] = -1;
        if (center_dist_out)
            center_dist_out[i] = 0.0;
    }
    if (n_done)
        *n_done = ctl.n_done;
    return EK_OK;
}
