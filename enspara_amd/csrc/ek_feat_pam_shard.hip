// ek_feat_pam_shard.hip -- one shard of a PAM sweep in feature space over several handles.
#include "ek_feat.h"

#include <string.h>
#include <algorithm>
#include <new>

// ===========================================================================
// PAM (k-medoids) sweep in feature space over several shards (one ek_feat handle each)
// ===========================================================================
// Reference: the MPI branch of enspara/cluster/kmedoids.py:575-699 (the draw over the
// gathered member counts :482-517, mpi/ops.py:143-212) for the libdist metrics.  Every
// shard keeps its float64 distances, its labels and the medoids' features (all K of
// them: an ambiguous member may go to any) in HBM; per proposal the caller hands every
// shard the proposed sample's features and gets ONE 32-byte record back,
//   { double sum_old, sum_new; int64 n; uint32 n_amb, moved }
// -- np.sum(d**2) of the shard's float64 distances as they stand and as the proposal
// would leave them, each in numpy's pairwise order over the shard's own array (the
// tree of feat_pw_leaf_kernel), and the clusters of the caller's window whose member
// lists the proposal would change.  The caller adds the records' sums in shard order,
// decides (kmedoids.py:683), and tells every shard.  The arithmetic is the single
// sweep's: FeatAcc's chain per (sample, row) pair, the three masks of :644-658, the
// ambiguous members against all medoids with strict < in ascending medoid index
// (feat_pam_nearest_tiled_kernel as it is), so one shard holding everything computes
// what ek_feat_pam_sweep computes, bit for bit.
#define FS_GATHER 64    // rows per gather launch

struct FeatPamOut {
    double sum_old, sum_new;
    int64_t n;
    uint32_t n_amb, moved;
};

// (member counts of a window's clusters with their scans, and the js[j]-th member from
// those scans: ek_launch_count_members_multi / ek_launch_select_member_multi, ek_pam.hip)

__device__ __forceinline__ uint32_t feat_win_bit(int32_t label, int win_lo, int win_count)
{
    const int i = label - win_lo;
    return (i >= 0 && i < win_count) ? (1u << i) : 0u;
}

// table[rows[b]][:] = the features of local sample idx[b]; rows that are not this
// shard's stay as they are (zero: the caller adds the shards' tables up)
template <typename T>
__global__ void __launch_bounds__(EK_BLOCK)
feat_shard_gather_kernel(const T *__restrict__ tiles, int64_t n, int F,
                         const int64_t *__restrict__ idx_rows, int count,
                         T *__restrict__ table)
{
    const int64_t f = idx_rows[blockIdx.x];
    const int64_t row = idx_rows[count + blockIdx.x];
    if (f < 0 || f >= n || row < 0)
        return;
    feat_copy_row(table + (size_t)row * F, 1, feat_tile_ptr(tiles, f, F), F, EK_BLOCK);
}

// MT[j][c] = table[c][j]: the medoids' rows [K][F] as the caller assembled them into
// the feature-major form the ambiguous members' search reads (thread = medoid)
template <typename T>
__global__ void __launch_bounds__(EK_BLOCK)
feat_shard_table_kernel(const T *__restrict__ table, int F, int Kcap, T *__restrict__ MT)
{
    const int c = blockIdx.x;
    for (int j = threadIdx.x; j < F; j += EK_BLOCK)
        MT[(size_t)j * Kcap + c] = table[(size_t)c * F + j];
}

// The proposal's pass over the shard's samples: distance of every sample to the row
// y (feat_distance_kernel's chain: non-temporal tile loads, the row in LDS in FY_CHUNK
// pieces), the three masks of kmedoids.py:644-658 into the trial state, the ambiguous
// members into `amb`, the window's clusters that lose or gain a sample into
// counters[1].  Workgroup 0 also puts the row into column cid of the medoid table,
// the column it displaces into `col` (nothing reads the table before the search that
// follows on the stream).
template <typename T, int METRIC>
__global__ void __launch_bounds__(EK_BLOCK)
feat_shard_propose_kernel(const T *__restrict__ tiles, const T *__restrict__ y, int64_t n,
                          int F, const double *__restrict__ dist,
                          const int32_t *__restrict__ assign, int32_t cid, int win_lo,
                          int win_count, double *__restrict__ ndist,
                          int32_t *__restrict__ nassign, uint32_t *__restrict__ amb,
                          unsigned int *__restrict__ counters, int Kcap, T *__restrict__ MT,
                          T *__restrict__ col)
{
    __shared__ T ys[FY_CHUNK];
    __shared__ uint32_t s_m;
    if (threadIdx.x == 0)
        s_m = 0;
    const int64_t f = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    // (workgroup 0: the piece of the row in LDS goes into the table as well)
    const double acc = feat_one_vs_all<T, METRIC>(
        feat_tile_ptr(tiles, f, F), y, F, ys, [&](int j0, int w) {
            if (blockIdx.x == 0)
                for (int j = threadIdx.x; j < w; j += EK_BLOCK) {
                    col[j0 + j] = MT[(size_t)(j0 + j) * Kcap + cid];
                    MT[(size_t)(j0 + j) * Kcap + cid] = ys[j];
                }
        });
    uint32_t m = 0;
    if (f < n) {
        const int32_t a = assign[f];
        if (feat_pam_classify(dist[f], a, feat_finish<METRIC>(acc, F), cid, f, ndist, nassign,
                              amb, counters))
            m = feat_win_bit(a, win_lo, win_count) | feat_win_bit(cid, win_lo, win_count);
    }
    if (m)
        atomicOr(&s_m, m);
    __syncthreads();
    if (threadIdx.x == 0 && s_m)
        atomicOr(&counters[1], s_m);
}

// one workgroup: the chunk sums of both columns added left to right
// (feat_total_decide_kernel's order), the ambiguous members that leave cluster cid,
// and the shard's record
__global__ void __launch_bounds__(EK_BLOCK)
feat_shard_record_kernel(const double *__restrict__ chunksum, int n_chunks, int64_t n,
                         const uint32_t *__restrict__ amb,
                         const unsigned int *__restrict__ counters,
                         const int32_t *__restrict__ nassign, int32_t cid, int win_lo,
                         int win_count, FeatPamOut *__restrict__ out)
{
    __shared__ double sums[2];
    __shared__ double cs[2 * EK_BLOCK];
    __shared__ uint32_t s_m;
    if (threadIdx.x == 0)
        s_m = 0;
    double run = 0.0;
    for (int c0 = 0; c0 < n_chunks; c0 += EK_BLOCK) {
        const int w = (n_chunks - c0 < EK_BLOCK) ? (n_chunks - c0) : EK_BLOCK;
        __syncthreads();
        for (int e = threadIdx.x; e < 2 * w; e += EK_BLOCK)
            cs[e] = chunksum[2 * (size_t)c0 + e];
        __syncthreads();
        if (threadIdx.x < 2)
            for (int c = 0; c < w; ++c)
                run = run + cs[2 * c + threadIdx.x];
    }
    if (threadIdx.x < 2)
        sums[threadIdx.x] = run;
    const unsigned int n_amb = counters[0];
    uint32_t m = 0;
    for (unsigned int i = threadIdx.x; i < n_amb; i += EK_BLOCK) {
        const int32_t na = nassign[amb[i]];
        if (na != cid)
            m |= feat_win_bit(na, win_lo, win_count) | feat_win_bit(cid, win_lo, win_count);
    }
    __syncthreads();
    if (m)
        atomicOr(&s_m, m);
    __syncthreads();
    if (threadIdx.x == 0) {
        out->sum_old = sums[0];
        out->sum_new = sums[1];
        out->n = n;
        out->n_amb = n_amb;
        out->moved = counters[1] | s_m;
    }
}

static int feat_shard_pam_state(ek_feat *k, const char *who, bool begun)
{
    if (!k)
        return ek_set_error(EK_EARG, "%s: NULL handle", who);
    if (!k->loaded || !k->kdist)
        return ek_set_error(EK_ESTATE, "%s: samples and a state (ek_feat_state_reset / "
                                       "_upload, or a k-centers run) first", who);
    if (k->n > 0xffffffffLL)
        return ek_set_error(EK_EARG, "%s: %lld samples on one shard", who, (long long)k->n);
    if (begun && (!k->pam || k->pam->sh_metric < 0))
        return ek_set_error(EK_ESTATE, "%s: ek_feat_pam_begin first", who);
    return EK_OK;
}

static int feat_shard_pam_alloc(ek_feat *k)
{
    if (!k->pam) {
        k->pam = new (std::nothrow) FeatPam();
        if (!k->pam)
            return ek_set_error(EK_ENOMEM, "ek_feat_pam: out of host memory");
    }
    FeatPam &p = *k->pam;
    // (each on its own: a call that failed part-way must not leave the next one a
    // group it takes for whole)
    const size_t nb = (size_t)std::max<int64_t>((k->n + EK_BLOCK - 1) / EK_BLOCK, 1);
    if (!p.sh_blockcnt)
        FE_HIP(ek_dev_malloc((void **)&p.sh_blockcnt, EK_PAM_WIN * nb * sizeof(int32_t)));
    if (!p.sh_scan)
        FE_HIP(ek_dev_malloc((void **)&p.sh_scan, EK_PAM_WIN * nb * sizeof(int64_t)));
    if (!p.sh_io)
        FE_HIP(ek_dev_malloc((void **)&p.sh_io, 3 * EK_PAM_WIN * sizeof(int64_t)));
    if (!p.sh_rows)
        FE_HIP(ek_dev_malloc((void **)&p.sh_rows, 2 * FS_GATHER * sizeof(int64_t)));
    return EK_OK;
}

extern "C" int ek_feat_pam_count_batch(ek_feat *k, int32_t cid0, int32_t count,
                                       int64_t *counts_host)
{
    int rc = feat_shard_pam_state(k, "ek_feat_pam_count_batch", false);
    if (rc)
        return rc;
    if (!counts_host || cid0 < 0 || count < 1 || count > EK_PAM_WIN)
        return ek_set_error(EK_EARG, "ek_feat_pam_count_batch: bad argument (1..%d clusters)",
                            EK_PAM_WIN);
    if (k->n == 0) {
        memset(counts_host, 0, (size_t)count * sizeof(int64_t));
        return EK_OK;
    }
    FE_HIP(hipSetDevice(k->device));
    if ((rc = feat_shard_pam_alloc(k)))
        return rc;
    FeatPam &p = *k->pam;
    ek_launch_count_members_multi(k->kassign, k->n, cid0, count, p.sh_blockcnt, p.sh_scan,
                                  p.sh_io, k->s);
    FE_HIP(hipGetLastError());
    FE_HIP(hipMemcpyAsync(counts_host, p.sh_io, (size_t)count * sizeof(int64_t),
                          hipMemcpyDeviceToHost, k->s));
    FE_HIP(hipStreamSynchronize(k->s));
    return EK_OK;
}

extern "C" int ek_feat_pam_select_batch(ek_feat *k, int32_t cid0, int32_t count,
                                        const int64_t *js_host, int64_t *members_host)
{
    int rc = feat_shard_pam_state(k, "ek_feat_pam_select_batch", false);
    if (rc)
        return rc;
    if (!js_host || !members_host || cid0 < 0 || count < 1 || count > EK_PAM_WIN)
        return ek_set_error(EK_EARG, "ek_feat_pam_select_batch: bad argument (1..%d "
                                     "clusters)", EK_PAM_WIN);
    if (k->n == 0 || !k->pam || !k->pam->sh_io) {
        for (int32_t j = 0; j < count; ++j)
            members_host[j] = -1;
        if (k->n == 0)
            return EK_OK;
        return ek_set_error(EK_ESTATE, "ek_feat_pam_select_batch: ek_feat_pam_count_batch "
                                       "of the same clusters first");
    }
    FE_HIP(hipSetDevice(k->device));
    FeatPam &p = *k->pam;
    FE_HIP(hipMemcpyAsync(p.sh_io + EK_PAM_WIN, js_host, (size_t)count * sizeof(int64_t),
                          hipMemcpyHostToDevice, k->s));
    ek_launch_select_member_multi(k->kassign, k->n, cid0, count, p.sh_scan,
                                  p.sh_io + EK_PAM_WIN, p.sh_io + 2 * EK_PAM_WIN, k->s);
    FE_HIP(hipGetLastError());
    FE_HIP(hipMemcpyAsync(members_host, p.sh_io + 2 * EK_PAM_WIN,
                          (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, k->s));
    FE_HIP(hipStreamSynchronize(k->s));
    return EK_OK;
}

extern "C" int ek_feat_pam_gather_rows(ek_feat *k, int32_t count, const int64_t *samples_host,
                                       const int64_t *rows_host, void *table_dev)
{
    if (!k || count < 0 || (count > 0 && (!samples_host || !rows_host || !table_dev)))
        return ek_set_error(EK_EARG, "ek_feat_pam_gather_rows: bad argument");
    if (!k->loaded)
        return ek_set_error(EK_ESTATE, "ek_feat_pam_gather_rows: no samples loaded");
    for (int32_t i = 0; i < count; ++i)
        if (samples_host[i] < 0 || samples_host[i] >= k->n || rows_host[i] < 0)
            return ek_set_error(EK_EARG, "ek_feat_pam_gather_rows: sample %lld (row %lld) "
                                         "is not one of this shard's %lld",
                                (long long)samples_host[i], (long long)rows_host[i],
                                (long long)k->n);
    if (count == 0)
        return EK_OK;
    FE_HIP(hipSetDevice(k->device));
    int rc = feat_shard_pam_alloc(k);
    if (rc)
        return rc;
    FeatPam &p = *k->pam;
    for (int32_t done = 0; done < count; done += FS_GATHER) {
        const int32_t cnt = std::min<int32_t>(FS_GATHER, count - done);
        FE_HIP(hipMemcpyAsync(p.sh_rows, samples_host + done, (size_t)cnt * sizeof(int64_t),
                              hipMemcpyHostToDevice, k->s));
        FE_HIP(hipMemcpyAsync(p.sh_rows + cnt, rows_host + done, (size_t)cnt * sizeof(int64_t),
                              hipMemcpyHostToDevice, k->s));
        feat_dispatch_size(k, [&](auto t) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL(feat_shard_gather_kernel<T>, dim3(cnt), dim3(EK_BLOCK), 0, k->s,
                               (const T *)k->tiles, k->n, k->F, p.sh_rows, cnt, (T *)table_dev);
        });
        FE_HIP(hipGetLastError());
        // (sh_rows is written again by the next piece, and by the next call)
        FE_HIP(hipStreamSynchronize(k->s));
    }
    return EK_OK;
}

extern "C" int ek_feat_pam_begin(ek_feat *k, int32_t metric, const void *table_dev,
                                 int32_t n_medoids)
{
    int rc = feat_shard_pam_state(k, "ek_feat_pam_begin", false);
    if (rc)
        return rc;
    if (!table_dev || n_medoids < 1 || metric < 0 || metric > 2)
        return ek_set_error(EK_EARG, "ek_feat_pam_begin: bad argument (metrics: euclidean 0, "
                                     "manhattan 1, hamming 2)");
    if ((rc = feat_metric_ok(k, metric, "ek_feat_pam_begin")))
        return rc;
    FE_HIP(hipSetDevice(k->device));
    if ((rc = feat_shard_pam_alloc(k)))
        return rc;
    FeatPam &p = *k->pam;
    p.sh_cid = -1;
    p.sh_metric = metric;
    p.K = n_medoids;
    if (k->n == 0)
        return EK_OK;           // (nothing of this shard is ever looked at)
    if ((rc = feat_pam_alloc(k, p, n_medoids))) {
        // (a group of the scratch may be half made: all of it goes, ek_feat_pam_sweep)
        (void)hipStreamSynchronize(k->s);
        ek_feat_pam_release(k);
        return rc;
    }
    feat_dispatch_size(k, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(feat_shard_table_kernel<T>, dim3(n_medoids), dim3(EK_BLOCK), 0, k->s,
                           (const T *)table_dev, k->F, p.Kcap, (T *)p.MT);
    });
    FE_HIP(hipGetLastError());
    return EK_OK;
}

// a proposal's five launches: [distances + classification + the row into the table], the
// ambiguous members' search, leaf sums, chunk sums, the record
template <typename T, int M>
static void feat_shard_enqueue_propose(ek_feat *k, FeatPam &p, int32_t cid, const void *row_dev,
                                       int32_t win_lo, int32_t win_count, void *out_dev)
{
    const unsigned blocks = (unsigned)((k->n + EK_BLOCK - 1) / EK_BLOCK);
    hipLaunchKernelGGL((feat_shard_propose_kernel<T, M>), dim3(blocks), dim3(EK_BLOCK), 0, k->s,
                       (const T *)k->tiles, (const T *)row_dev, k->n, k->F, k->kdist,
                       k->kassign, cid, win_lo, win_count, p.ndist, p.nassign, p.amb,
                       p.counters, p.Kcap, (T *)p.MT, (T *)p.col);
    feat_pam_enqueue_search_cost(k, M, p.K, nullptr);
    hipLaunchKernelGGL(feat_shard_record_kernel, dim3(1), dim3(EK_BLOCK), 0, k->s,
                       p.part + 2 * (size_t)p.n_leaves, p.n_chunks, k->n, p.amb, p.counters,
                       p.nassign, cid, win_lo, win_count, (FeatPamOut *)out_dev);
}

extern "C" int ek_feat_pam_propose(ek_feat *k, int32_t cid, const void *row_dev,
                                   int32_t win_lo, int32_t win_count, void *out_dev)
{
    int rc = feat_shard_pam_state(k, "ek_feat_pam_propose", true);
    if (rc)
        return rc;
    FeatPam &p = *k->pam;
    if (!row_dev || !out_dev || cid < 0 || cid >= p.K || win_lo < 0 || win_count < 0 ||
        win_count > 32)
        return ek_set_error(EK_EARG, "ek_feat_pam_propose: bad argument (cluster %d of %d, "
                                     "window %d + %d)", cid, p.K, win_lo, win_count);
    if (p.sh_cid >= 0)
        return ek_set_error(EK_ESTATE, "ek_feat_pam_propose: the proposal for cluster %d "
                                       "waits for ek_feat_pam_commit", p.sh_cid);
    FE_HIP(hipSetDevice(k->device));
    p.sh_cid = cid;
    if (k->n == 0) {            // np.sum of no distances: 0.0; n = 0
        FE_HIP(hipMemsetAsync(out_dev, 0, sizeof(FeatPamOut), k->s));
        return EK_OK;
    }
    FE_HIP(hipMemsetAsync(p.counters, 0, 2 * sizeof(unsigned int), k->s));
    feat_dispatch(k, p.sh_metric, [&](auto t, auto m) {
        feat_shard_enqueue_propose<typename decltype(t)::type, decltype(m)::value>(
            k, p, cid, row_dev, win_lo, win_count, out_dev);
    });
    FE_HIP(hipGetLastError());
    return EK_OK;
}

extern "C" int ek_feat_pam_commit(ek_feat *k, int32_t accept)
{
    int rc = feat_shard_pam_state(k, "ek_feat_pam_commit", true);
    if (rc)
        return rc;
    FeatPam &p = *k->pam;
    if (p.sh_cid < 0)
        return ek_set_error(EK_ESTATE, "ek_feat_pam_commit: no proposal to decide on");
    const int32_t cid = p.sh_cid;
    p.sh_cid = -1;
    if (k->n == 0)
        return EK_OK;
    FE_HIP(hipSetDevice(k->device));
    if (accept) {               // the trial state becomes the state (kmedoids.py:684-690)
        std::swap(k->kdist, p.ndist);
        std::swap(k->kassign, p.nassign);
        return EK_OK;
    }
    feat_pam_enqueue_restore(k, cid);
    FE_HIP(hipGetLastError());
    return EK_OK;
}
