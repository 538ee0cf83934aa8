// ek_feat.h -- what the feature-space sources share (ek_features.hip,
// ek_feat_kcenters.hip, ek_feat_pam.hip, ek_feat_pam_shard.hip, ek_feat_assign.hip):
// the handle; the arithmetic of one (sample, point) distance -- FeatAcc's chain over
// the features in order, then feat_finish --; the one-vs-all loop built on it; the
// few device helpers every part needs; and the one place where an (element kind,
// metric) pair picks a kernel instantiation.
#pragma once
#include "ek_common.h"
#include "ek_pw.h"
#include "ek_reduce.h"

#include <type_traits>

extern int ek_set_error(int code, const char *fmt, ...);

// (a function one feature source has for another: not one of the library's symbols)
#define FEAT_LOCAL __attribute__((visibility("hidden")))

#define FT_CHUNK 32           // features per staged transposition chunk
#define FY_CHUNK 2048         // target-point features staged in LDS at a time

// per-workgroup partial of the arg-max over float64 distances
struct FeatBlockMax {
    double val;
    int64_t idx;
};
// the resident k-centers loop (ek_feat_kcenters)
struct FeatCtl {
    int64_t next;       // sample that becomes the next center
    int32_t n_done;     // centers applied by this run
    int32_t stopped;    // distances.max() <= cutoff (kcenters.py:217)
    double last_max;
};
// one shard of a k-centers run over several handles (ek_feat_kcenters_step)
struct FeatShardCtl {
    int32_t n_done;       // labels applied so far (last label + 1)
    int32_t stopped;      // a step found max <= cutoff: later steps return at once
    // arrival counters of the launch in flight (ek_arrive_last_tree: a million
    // samples are 3907 workgroups, and as many returning atomics on one address
    // serialise -- measured, they nearly doubled the step's time)
    unsigned int top;
    unsigned int pad;
    unsigned int leaves[EK_ARRIVE_G];
};

// working set of the PAM sweeps (ek_feat_pam.hip; ek_feat_pam_shard.hip)
struct FeatPam {
    int32_t K = 0, Kcap = 0;
    void *MT = nullptr;         // medoids' features, transposed: [F][Kcap] elements
    void *col = nullptr;        // [F] the column a proposal displaced
    int64_t *med = nullptr;     // [Kcap] the medoids' samples (for the table)
    int64_t *idx = nullptr;     // [1] the proposed sample (device)
    double *ndist = nullptr;    // trial state
    int32_t *nassign = nullptr;
    uint32_t *amb = nullptr;    // ambiguous members
    double *best_d = nullptr;
    int32_t *best_c = nullptr;
    unsigned int *counters = nullptr;   // [0] ambiguous members
    int32_t *blockcnt = nullptr;
    int64_t *scan = nullptr, *total = nullptr;
    double *part = nullptr;     // leaf sums + chunk sums (both columns)
    double *out2 = nullptr;
    EkPwShape *shapes = nullptr;
    int n_full = 0, n_leaves = 0, n_chunks = 0;
    // the sweep without a host round trip per proposal (round 4)
    struct FeatPamCtl *ctl = nullptr;   // device: stream position, status, last verdict
    uint32_t *raw_dev = nullptr;        // the caller's raw random outputs
    int64_t raw_cap = 0;
    int64_t *jdev = nullptr;            // [1] the member drawn
    int64_t *props_dev = nullptr;       // [Kcap] explicit proposals
    int32_t *accept_dev = nullptr;      // [Kcap]
    int32_t Kcap_async = 0;
    // windows of proposals (round 5): one pass over the samples for a window's distances
    struct FeatWin *win = nullptr;      // device: the window's draws and proposals
    void *Y = nullptr;                  // [FEAT_WIN][F] the proposals' features
    double *vecs = nullptr;             // [FEAT_WIN][n] every sample's distance to each
    int32_t *blockcntW = nullptr;       // [FEAT_WIN][workgroups] member counts
    int64_t *scanW = nullptr, *totalW = nullptr;
    int64_t n_windows = 0, n_stale = 0; // (since the context was made: a diagnostic)
    int win_width = 8;                  // slots of the next window of drawn proposals
    int plain_left = 0;                 // proposals to go one at a time before the next window
    // the ambiguous members' search, tiled (round 5)
    double *near_d = nullptr;           // [n][chunks of 256 medoids] a chunk's nearest
    int32_t *near_c = nullptr;
    unsigned int *near_tick = nullptr;  // [n / FN_MB + 1] arrivals per batch of members
    int32_t near_kc = 0;
    // one shard of a sweep over several handles (ek_feat_pam_propose, ek_feat_pam_shard.hip)
    int32_t *sh_blockcnt = nullptr;     // [EK_PAM_WIN][workgroups] member counts of a window
    int64_t *sh_scan = nullptr;         // ... their exclusive scans
    int64_t *sh_io = nullptr;           // [3 * EK_PAM_WIN] totals | members wanted | members found
    int64_t *sh_rows = nullptr;         // [2 * FS_GATHER] samples and table rows of a gather
    int32_t sh_metric = -1;             // the metric of ek_feat_pam_begin (-1: no sweep begun)
    int32_t sh_cid = -1;                // the proposal waiting for ek_feat_pam_commit
};

struct ek_feat {
    int device = 0;
    int64_t n = 0;
    int32_t F = 0;
    int32_t kind = 0;         // 0 float32, 1 float64, 2 int64
    int32_t esize = 4;
    int64_t n_tiles = 0;
    hipStream_t s = nullptr;
    void *tiles = nullptr;    // [n_tiles][F][EK_TILE] elements
    void *stage = nullptr;
    int64_t stage_rows = 0;
    void *y = nullptr;        // [F] elements
    double *out = nullptr;    // [n]
    bool loaded = false;
    // device-resident k-centers state (ek_feat_kcenters)
    double *kdist = nullptr;  // [n] float64, as the reference keeps it
    int32_t *kassign = nullptr;
    FeatBlockMax *bm = nullptr;
    FeatCtl *ctl = nullptr;
    int64_t *hist = nullptr;
    int32_t hist_cap = 0;
    FeatPam *pam = nullptr;
    // one shard of a k-centers run over several handles (ek_feat_kcenters_step)
    bool own_stream = true;   // false: s is the caller's (ek_feat_create_sharded)
    int64_t goff = 0;         // global index of local sample 0
    FeatShardCtl *sctl = nullptr;
    int64_t *shist_idx = nullptr;   // [shist_cap] winners' global indices
    double *shist_d = nullptr;      // ... and their distances before the update
    int32_t shist_cap = 0;
    // ek_feat_assign_nearest (ek_feat_assign.hip): the center table and, where the
    // centers are split over workgroups, each part's nearest per sample
    void *acent = nullptr;          // [acent_cap] bytes
    size_t acent_cap = 0;
    double *apart_d = nullptr;      // [apart_cap] (part, sample)
    int32_t *apart_c = nullptr;
    size_t apart_cap = 0;
};

#define FE_HIP(call)                                                           \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess)                                                  \
            return ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,      \
                                hipGetErrorString(e_), __FILE__, __LINE__);    \
    } while (0)

// ---- what one part does for another ------------------------------------------------
// ek_features.hip: k->out[i] = metric(sample i, k->y), enqueued
FEAT_LOCAL void feat_enqueue_distance(ek_feat *k, int32_t metric);
// ek_feat_kcenters.hip: kdist / kassign with the partials' and the loop's blocks;
// the same, and what the sharded steps keep beside them
FEAT_LOCAL int feat_state_alloc(ek_feat *k);
int feat_shard_alloc(ek_feat *k, int32_t label);
// ek_feat_pam.hip: the working set for K medoids; the ambiguous members' search and
// the two cost trees down to the chunk sums (three launches); column cid of the
// medoid table back from `col`
extern "C" void ek_feat_pam_release(ek_feat *k);
FEAT_LOCAL int feat_pam_alloc(ek_feat *k, FeatPam &p, int32_t K);
FEAT_LOCAL void feat_pam_enqueue_search_cost(ek_feat *k, int32_t metric, int32_t K,
                                             const int32_t *halt);
FEAT_LOCAL void feat_pam_enqueue_restore(ek_feat *k, int32_t cid);

// ---- (element kind, metric) -> <T, METRIC> -------------------------------------------
template <typename T> struct FeatType {
    using type = T;
};
template <int M> using FeatMetric = std::integral_constant<int, M>;

// the metric is one of the three and fits the element kind (libdist.pyx:77-95 compares
// integers; euclidean and manhattan take float32 / float64)
static inline int feat_metric_ok(const ek_feat *k, int32_t metric, const char *who)
{
    if (metric < 0 || metric > 2)
        return ek_set_error(EK_EARG, "%s: bad argument", who);
    if ((metric == 2) != (k->kind == 2))
        return ek_set_error(EK_EARG, "%s: hamming needs integer samples, the other metrics "
                                     "floating point", who);
    return EK_OK;
}

// fn(FeatType<T>{}, FeatMetric<M>{}) for the pair's instantiation, one of
// <float, 0> <float, 1> <double, 0> <double, 1> <long long, 2> (after feat_metric_ok)
template <typename Fn> static inline void feat_dispatch(const ek_feat *k, int32_t metric, Fn &&fn)
{
    if (k->kind == 2)
        fn(FeatType<long long>{}, FeatMetric<2>{});
    else if (k->kind == 0) {
        if (metric == 0)
            fn(FeatType<float>{}, FeatMetric<0>{});
        else
            fn(FeatType<float>{}, FeatMetric<1>{});
    } else {
        if (metric == 0)
            fn(FeatType<double>{}, FeatMetric<0>{});
        else
            fn(FeatType<double>{}, FeatMetric<1>{});
    }
}

// fn(FeatType<T>{}) for kernels that depend on the element type alone
template <typename Fn> static inline void feat_dispatch_type(const ek_feat *k, Fn &&fn)
{
    if (k->kind == 2)
        fn(FeatType<long long>{});
    else if (k->kind == 0)
        fn(FeatType<float>{});
    else
        fn(FeatType<double>{});
}

// ... and for kernels that only move elements: by their size (int64 goes as double)
template <typename Fn> static inline void feat_dispatch_size(const ek_feat *k, Fn &&fn)
{
    if (k->esize == 4)
        fn(FeatType<float>{});
    else
        fn(FeatType<double>{});
}

// ---- one (sample, point) distance ------------------------------------------------------
template <typename T, int METRIC> struct FeatAcc;
// euclidean
template <> struct FeatAcc<float, 0> {
    static __device__ __forceinline__ void add(double &acc, float x, float y)
    {
        const float d = x - y;           // float32 subtraction
        const float q = d * d;           // float32 product (powf(d, 2) == d*d)
        acc = acc + (double)q;
    }
};
template <> struct FeatAcc<double, 0> {
    static __device__ __forceinline__ void add(double &acc, double x, double y)
    {
        const double d = x - y;
        acc = acc + d * d;
    }
};
// manhattan
template <> struct FeatAcc<float, 1> {
    static __device__ __forceinline__ void add(double &acc, float x, float y)
    {
        const float d = x - y;
        acc = acc + __builtin_fabs((double)d);
    }
};
template <> struct FeatAcc<double, 1> {
    static __device__ __forceinline__ void add(double &acc, double x, double y)
    {
        acc = acc + __builtin_fabs(x - y);
    }
};
// hamming
template <> struct FeatAcc<long long, 2> {
    static __device__ __forceinline__ void add(double &acc, long long x,
                                               long long y)
    {
        if (x != y)
            acc = acc + 1.0;
    }
};

// what libdist.pyx does with a row's sum: sqrt (:143), nothing (:119), / n_features (:93)
template <int METRIC> __device__ __forceinline__ double feat_finish(double acc, int F)
{
    if (METRIC == 0)
        return __builtin_sqrt(acc);
    if (METRIC == 2)
        return acc / (double)F;
    return acc;
}

// sample f's column in the tiles: feature j is at [j * EK_TILE]
template <typename T, typename I>
__device__ __forceinline__ T *feat_tile_ptr(T *tiles, I f, int F)
{
    return tiles + (size_t)(f / EK_TILE) * (size_t)F * EK_TILE + (f % EK_TILE);
}

struct FeatNoChunkJob {
    __device__ __forceinline__ void operator()(int, int) const {}
};

// The unfinished float64 sum of the calling lane's sample (column p) against the point
// y, for a whole workgroup of EK_BLOCK lanes: y goes through LDS (ys[FY_CHUNK]) in
// pieces, each read as wave-wide broadcasts; the tile column is streamed past the
// caches.  job(j0, w) runs once per piece with ys[0..w) = y[j0..j0+w) in place.
template <typename T, int METRIC, typename Job = FeatNoChunkJob>
__device__ __forceinline__ double feat_one_vs_all(const T *p, const T *__restrict__ y, int F,
                                                  T *ys, Job job = Job())
{
    double acc = 0.0;
    for (int j0 = 0; j0 < F; j0 += FY_CHUNK) {
        const int w = (F - j0 < FY_CHUNK) ? (F - j0) : FY_CHUNK;
        __syncthreads();
        for (int j = threadIdx.x; j < w; j += EK_BLOCK)
            ys[j] = y[j0 + j];
        __syncthreads();
        job(j0, w);
#pragma unroll 8
        for (int j = 0; j < w; ++j)
            FeatAcc<T, METRIC>::add(acc, __builtin_nontemporal_load(
                                             p + (size_t)(j0 + j) * EK_TILE),
                                    ys[j]);
    }
    return acc;
}

// dst[j * dst_stride] = feature j of the sample whose column is p (zeros where !have),
// by a workgroup of nthreads
template <typename T>
__device__ __forceinline__ void feat_copy_row(T *dst, size_t dst_stride, const T *p, int F,
                                              int nthreads, bool have = true)
{
    for (int j = threadIdx.x; j < F; j += nthreads)
        dst[(size_t)j * dst_stride] = have ? p[(size_t)j * EK_TILE] : (T)0;
}

// a proposal goes in: y = the features of the sample whose column is p; column cid of
// the medoid table is saved in `col` and replaced by them
template <typename T>
__device__ __forceinline__ void feat_propose_row(const T *p, int F, int cid, int Kcap, T *MT,
                                                 T *col, T *y)
{
    for (int j = threadIdx.x; j < F; j += EK_BLOCK) {
        const T v = p[(size_t)j * EK_TILE];
        col[j] = MT[(size_t)j * Kcap + cid];
        MT[(size_t)j * Kcap + cid] = v;
        y[j] = v;
    }
}

// kmedoids.py:644-658 for sample f -- distance d and label a as they stand, distance x
// to the proposal for cluster cid -- into the trial state; a member of cid that is not
// closer to the proposal is ambiguous and goes to `amb` (counters[0] counts them).
// True where the sample changes cluster here (:644 with a != cid).
__device__ __forceinline__ bool feat_pam_classify(double d, int32_t a, double x, int32_t cid,
                                                  int64_t f, double *__restrict__ ndist,
                                                  int32_t *__restrict__ nassign,
                                                  uint32_t *__restrict__ amb,
                                                  unsigned int *__restrict__ counters)
{
    if (d > x) {                        // :644
        ndist[f] = x;
        nassign[f] = cid;
        return a != cid;
    }
    if (a != cid) {                     // :651
        ndist[f] = d;
        nassign[f] = a;
    } else {                            // :658
        amb[atomicAdd(&counters[0], 1u)] = (uint32_t)f;
    }
    return false;
}

// ---- arg-max over (float64 value, index): the largest value, the lowest index among
// equal ones (np.argmax's first) ----------------------------------------------------------
__device__ __forceinline__ bool feat_better(double v, int64_t i, double bv, int64_t bi)
{
    return (v > bv) || (v == bv && i < bi);
}

__device__ __forceinline__ void feat_wave_argmax(double &v, int64_t &i)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(v, off, 64);
        const int64_t oi = __shfl_xor(i, off, 64);
        if (feat_better(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
}

// The best pair of a workgroup, from every wave's best (feat_wave_argmax) through rv / ri:
// the caller's slots in LDS, one per wave -- their size is the workgroup's wave count.
// The waves' pairs into their slots, and a barrier
template <int WAVES>
__device__ __forceinline__ void feat_slots_put(double v, int64_t i, double (&rv)[WAVES],
                                               int64_t (&ri)[WAVES])
{
    if ((threadIdx.x & (EK_WAVE - 1)) == 0) {
        rv[threadIdx.x / EK_WAVE] = v;
        ri[threadIdx.x / EK_WAVE] = i;
    }
    __syncthreads();
}
// ... and the best of the slots, for a thread that holds slot 0's pair
template <int WAVES>
__device__ __forceinline__ void feat_slots_best(double &v, int64_t &i, const double (&rv)[WAVES],
                                                const int64_t (&ri)[WAVES])
{
#pragma unroll
    for (int w = 1; w < WAVES; ++w)
        if (feat_better(rv[w], ri[w], v, i)) {
            v = rv[w];
            i = ri[w];
        }
}
// the workgroup's best pair in every thread
template <int WAVES>
__device__ __forceinline__ void feat_block_argmax_all(double &v, int64_t &i, double (&rv)[WAVES],
                                                      int64_t (&ri)[WAVES])
{
    feat_wave_argmax(v, i);
    __syncthreads();                    // (rv / ri may still be read from a call before)
    feat_slots_put(v, i, rv, ri);
    v = rv[0];
    i = ri[0];
    feat_slots_best(v, i, rv, ri);
}

// block partial of (value, index) pairs held one per thread -> bm[blockIdx.x]
__device__ __forceinline__ void feat_block_partial(double v, int64_t i, FeatBlockMax *bm)
{
    __shared__ double rv[EK_BLOCK / EK_WAVE];
    __shared__ int64_t ri[EK_BLOCK / EK_WAVE];
    feat_wave_argmax(v, i);
    feat_slots_put(v, i, rv, ri);
    if (threadIdx.x == 0) {
        feat_slots_best(v, i, rv, ri);
        bm[blockIdx.x].val = v;
        bm[blockIdx.x].idx = i;
    }
}
