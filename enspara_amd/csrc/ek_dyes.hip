// ek_dyes.hip -- smFRET dye labelling on the device: dye point clouds placed on residues,
// the points that touch the protein removed, all pairwise distances histogrammed.
//
// Replaces dye_distance_distribution of the reference's enspara/geometry/
// dyes_from_expt_dist.py and what it calls (:235-287 remove_touches_protein, :326-345
// align_dye_to_res, :348-412 bincount_dists / pairwise_distance_distribution).
//
// The contract (include/enspara_hip.h has the full text):
//   align    float32, nothing fused: p_j = ((x*M[0][j] + y*M[1][j]) + z*M[2][j]) + t[j]
//   touch    float64: kept iff for every atom sqrt((dx*dx + dy*dy) + dz*dz) > cutoff,
//            d = double(atom) - double(point); kept points keep their order
//   pairs    float64 distances by the same formula; n1 * n2 <= 5e7: one chunk, else the
//            larger cloud (the second on a tie) in chunks of 2048 points; per chunk
//            nbins_c = int(dmax_c / bin_width) + 2, step_c = (nbins_c * bin_width) / nbins_c,
//            bin k iff double(k) * step_c <= d < double(k + 1) * step_c; counts added over
//            the chunks, nbins = max nbins_c
//
// No kernel takes a float64 square root.  The square root is correctly rounded and so
// monotone: sqrt(s) > c, sqrt(s) >= e and int(sqrt(s) / w) >= m each hold from one double
// s on and for none below it.  The host finds that double for every cutoff, every edge and
// every m (dy_sq_at_least / dy_div_at_least: a product, then steps of one ulp checked with
// the host's own sqrt and division), and the kernels compare squared distances with those
// tables.  The bin of a pair is guessed from a float32 square root and moved to where the
// table says it belongs.
//
//   touch    one lane per (frame, placement, point); the frame's atoms pass through the
//            LDS in batches of DY_STAGE as (x, y, z, threshold) doubles; a lane stops at the
//            first touching atom, a workgroup once none of its lanes is left.  -> keep bytes
//   compact  one workgroup per (frame, placement): ballot compaction of the kept points in
//            their order, aligned again (the same float32 expressions) and stored as doubles
//   max      one lane per point of the larger cloud, the other cloud read at uniform
//            addresses; the largest squared distance of every chunk by an integer atomic
//            maximum on the double's bits (they order as the doubles do, none is negative)
//   plan     nbins_c of every chunk by binary search of the maximum in the table of m
//   hist     as max; a workgroup's counts in the LDS (uint32, integer atomics, a lane adds a
//            run of equal bins at once), then added to the pair's int64 counts in memory
// Counts are integers: the order of the additions is free, every run gives the same bits.
//
// Bound.  nbins_c <= DY_MAX_BINS = 4096.  Every placement lies in the box t_j +- r_j, r_j =
// (rho * |column j of M| + (|t_j| + rho * |column j of M|) * 2^-20) * (1 + 2^-16), rho the
// largest norm of the cloud's points: Cauchy-Schwarz for the exact product, 2^-20 relative
// to the magnitudes for the three float32 products and three sums of the contract (each
// rounds by 2^-24 of at most |t_j| + 3 rho |M|), 2^-16 for the host's own rounding.  The
// diagonal of the box that holds a frame's four placements must be below 4093 bin widths
// (EK_EARG), and coordinates at most 2^20 nm.
#include "ek_common.h"
#include "ek_sq_threshold.h"

#include <math.h>
#include <new>
#include <vector>

extern int ek_set_error(int code, const char *fmt, ...);
int ek_mi_check_memory(size_t bytes, const char *who);

#define DY_HIP(call)                                                           \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define DY_WG 256
#define DY_STAGE 1024                       // atoms of one batch: 32 KiB of LDS
#define DY_MAX_POINTS (1 << 20)             // of a cloud
#define DY_MAX_BINS 4096                    // of a chunk's histogram
#define DY_CHUNK 2048                       // points of the larger cloud per chunk
#define DY_ONE_CHUNK_PAIRS ((int64_t)50000000)
#define DY_MAX_FRAMES 4096                  // of one upload: 4 placements each in grid.y
#define DY_MAX_COORD 1048576.0              // nm
#define DY_MAX_SPLIT 16                     // slices of the smaller cloud
#define DY_MIN_WIDTH 0x1p-40
#define DY_MAX_WIDTH 0x1p40

// ---- host: the thresholds ------------------------------------------------------------------
// (dy_sq_at_least, the smallest double s >= 0 with sqrt(s) >= e: ek_sq_threshold.h)

// the smallest double x >= 0 with x / w >= m
static double dy_div_at_least(double m, double w)
{
    double x = m * w;
    while (x > 0.0 && nextafter(x, 0.0) / w >= m)
        x = nextafter(x, 0.0);
    while (x / w < m)
        x = nextafter(x, INFINITY);
    return x;
}

struct DyTab {
    double *S = nullptr;        // [DY_MAX_BINS - 1] squared distance from which int(d / w) >= m
    int32_t *tix = nullptr;     // [DY_MAX_BINS + 1] which table of edges nbins_c reads
    double *q = nullptr;        // [nt][DY_MAX_BINS] squared distance from which d >= edge k
    float *inv = nullptr;       // [nt] 1 / step, for the guess
    int nS = DY_MAX_BINS - 1;
};

static void dy_tab_free(DyTab &T)
{
    (void)ek_dev_free(T.S);
    (void)ek_dev_free(T.tix);
    (void)ek_dev_free(T.q);
    (void)ek_dev_free(T.inv);
    T = DyTab();
}

static int dy_tab_upload(double w, DyTab &T, hipStream_t s)
{
    int rc = EK_OK;
    std::vector<double> S, q, steps;
    std::vector<int32_t> tix;
    std::vector<float> inv;
    try {
        S.resize(T.nS);
        tix.assign(DY_MAX_BINS + 1, 0);
        for (int m = 1; m <= T.nS; ++m)
            S[m - 1] = dy_sq_at_least(dy_div_at_least((double)m, w));
        for (int n = 2; n <= DY_MAX_BINS; ++n) {
            const double st = ((double)n * w) / (double)n;
            size_t t = 0;
            while (t < steps.size() && steps[t] != st)
                ++t;
            if (t == steps.size())
                steps.push_back(st);
            tix[n] = (int32_t)t;
        }
        q.resize(steps.size() * DY_MAX_BINS);
        inv.resize(steps.size());
        for (size_t t = 0; t < steps.size(); ++t) {
            inv[t] = (float)(1.0 / steps[t]);
            for (int k = 0; k < DY_MAX_BINS; ++k)
                q[t * DY_MAX_BINS + k] = dy_sq_at_least((double)k * steps[t]);
        }
    } catch (const std::bad_alloc &) {
        return ek_set_error(EK_ENOMEM, "ek_dyes: out of host memory");
    }
    DY_HIP(ek_dev_malloc(&T.S, S.size() * sizeof(double)));
    DY_HIP(ek_dev_malloc(&T.tix, tix.size() * sizeof(int32_t)));
    DY_HIP(ek_dev_malloc(&T.q, q.size() * sizeof(double)));
    DY_HIP(ek_dev_malloc(&T.inv, inv.size() * sizeof(float)));
    DY_HIP(hipMemcpyAsync(T.S, S.data(), S.size() * sizeof(double), hipMemcpyHostToDevice, s));
    DY_HIP(hipMemcpyAsync(T.tix, tix.data(), tix.size() * sizeof(int32_t),
                          hipMemcpyHostToDevice, s));
    DY_HIP(hipMemcpyAsync(T.q, q.data(), q.size() * sizeof(double), hipMemcpyHostToDevice, s));
    DY_HIP(hipMemcpyAsync(T.inv, inv.data(), inv.size() * sizeof(float), hipMemcpyHostToDevice,
                          s));
    DY_HIP(hipStreamSynchronize(s));        // (the vectors go with this frame)
done:
    return rc;
}

// ---- device ----------------------------------------------------------------------------------
__device__ inline void dy_align(const float *__restrict__ mt, float x, float y, float z,
                                float &ox, float &oy, float &oz)
{
    ox = ((x * mt[0] + y * mt[3]) + z * mt[6]) + mt[9];
    oy = ((x * mt[1] + y * mt[4]) + z * mt[7]) + mt[10];
    oz = ((x * mt[2] + y * mt[5]) + z * mt[8]) + mt[11];
}

// slot = 4 * frame + placement; placements 0, 1 are dye1 and 2, 3 dye2, on residue
// (placement & 1).  mt == nullptr: the points as they are (ek_dyes_touches).
__device__ inline void dy_point(int slot, int i, const float *__restrict__ Mt,
                                const float *__restrict__ dye1, const float *__restrict__ dye2,
                                float &px, float &py, float &pz)
{
    const float *d = ((slot & 3) < 2) ? dye1 : dye2;
    const float x = d[3 * (size_t)i], y = d[3 * (size_t)i + 1], z = d[3 * (size_t)i + 2];
    if (Mt)
        dy_align(Mt + ((size_t)(slot >> 2) * 2 + (slot & 1)) * 12, x, y, z, px, py, pz);
    else {
        px = x;
        py = y;
        pz = z;
    }
}

__global__ void __launch_bounds__(DY_WG)
dy_touch_kernel(const float *__restrict__ xyz, int32_t atoms, const double *__restrict__ thr,
                const float *__restrict__ Mt, const float *__restrict__ dye1, int32_t n1,
                const float *__restrict__ dye2, int32_t n2, int32_t maxn,
                uint8_t *__restrict__ keep)
{
    __shared__ double4 at[DY_STAGE];
    const int tid = threadIdx.x;
    const int slot = (int)blockIdx.y;
    const int32_t n = ((slot & 3) < 2) ? n1 : n2;
    const int32_t i0 = (int32_t)blockIdx.x * DY_WG;
    if (i0 >= n)
        return;
    const int32_t i = i0 + tid;
    const bool valid = i < n;
    float fx, fy, fz;
    dy_point(slot, valid ? i : i0, Mt, dye1, dye2, fx, fy, fz);
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    const float *X = xyz + (size_t)(slot >> 2) * atoms * 3;
    bool alive = valid;
    for (int32_t base = 0; base < atoms; base += DY_STAGE) {
        const int32_t cnt = (atoms - base < DY_STAGE) ? atoms - base : DY_STAGE;
        for (int32_t a = tid; a < cnt; a += DY_WG) {
            const size_t j = (size_t)(base + a);
            at[a] = make_double4((double)X[3 * j], (double)X[3 * j + 1], (double)X[3 * j + 2],
                                 thr[j]);
        }
        __syncthreads();
        if (alive)
            for (int32_t a = 0; a < cnt; ++a) {
                const double4 e = at[a];
                const double dx = e.x - px, dy = e.y - py, dz = e.z - pz;
                if (!((dx * dx + dy * dy) + dz * dz >= e.w)) {
                    alive = false;
                    break;
                }
            }
        // (also the barrier before the next batch overwrites the list)
        if (!__syncthreads_or(alive ? 1 : 0))
            break;
    }
    if (valid)
        keep[(size_t)slot * maxn + i] = alive ? 1 : 0;
}

__global__ void __launch_bounds__(DY_WG)
dy_compact_kernel(const uint8_t *__restrict__ keep, const float *__restrict__ Mt,
                  const float *__restrict__ dye1, int32_t n1, const float *__restrict__ dye2,
                  int32_t n2, int32_t maxn, double *__restrict__ pts, int32_t *__restrict__ cnt)
{
    __shared__ int wsum[DY_WG / EK_WAVE];
    const int tid = threadIdx.x, lane = tid & (EK_WAVE - 1), wave = tid / EK_WAVE;
    const int slot = (int)blockIdx.x;
    const int32_t n = ((slot & 3) < 2) ? n1 : n2;
    double *out = pts + (size_t)slot * maxn * 3;
    int32_t base = 0;
    for (int32_t i0 = 0; i0 < n; i0 += DY_WG) {
        const int32_t i = i0 + tid;
        const bool k = i < n && keep[(size_t)slot * maxn + i] != 0;
        const unsigned long long m = __ballot(k);
        if (lane == 0)
            wsum[wave] = __popcll(m);
        __syncthreads();
        int32_t off = base, tot = 0;
        for (int w = 0; w < DY_WG / EK_WAVE; ++w) {
            if (w < wave)
                off += wsum[w];
            tot += wsum[w];
        }
        if (k) {        // (off + rank < base + tot <= n <= maxn)
            float fx, fy, fz;
            dy_point(slot, i, Mt, dye1, dye2, fx, fy, fz);
            const size_t o = 3 * (size_t)(off + __popcll(m & (((unsigned long long)1 << lane) - 1)));
            out[o] = (double)fx;
            out[o + 1] = (double)fy;
            out[o + 2] = (double)fz;
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0)
        cnt[slot] = base;
}

// the two clouds of a pair and how the reference would chunk them
struct DyShape {
    int32_t big, small;         // slots; the chunks cut `big`
    int32_t nbig, nsmall;
    int32_t L;                  // points of a chunk (2^30: the pairs are one chunk)
    int32_t nchunks;            // 0: the pair has no pairs
};

__device__ inline DyShape dy_shape(const int32_t *__restrict__ cnt, int job)
{
    const int f4 = 4 * (job >> 1);
    const int sa = (job & 1) ? f4 + 1 : f4, sb = (job & 1) ? f4 + 2 : f4 + 3;
    const int32_t na = cnt[sa], nb = cnt[sb];
    DyShape r;
    const bool chunked = (int64_t)na * nb > DY_ONE_CHUNK_PAIRS;
    if (chunked && na > nb) {
        r.big = sa, r.small = sb, r.nbig = na, r.nsmall = nb;
    } else {
        r.big = sb, r.small = sa, r.nbig = nb, r.nsmall = na;
    }
    r.L = chunked ? DY_CHUNK : (1 << 30);
    r.nchunks = (na < 1 || nb < 1) ? 0 : chunked ? (r.nbig + DY_CHUNK - 1) / DY_CHUNK : 1;
    return r;
}

// this workgroup's part of a pair: points [i0, i0 + 256) of the larger cloud (one chunk:
// DY_CHUNK is a multiple of 256) against points [j0, j1) of the smaller
__device__ inline bool dy_part(const DyShape &sh, int split, int32_t &i0, int32_t &j0, int32_t &j1)
{
    i0 = (int32_t)blockIdx.x * DY_WG;
    if (sh.nchunks == 0 || i0 >= sh.nbig)
        return false;
    const int32_t per = (sh.nsmall + split - 1) / split;
    j0 = (int32_t)blockIdx.z * per;
    j1 = (sh.nsmall - j0 < per) ? sh.nsmall : j0 + per;
    return j0 < j1;
}

__global__ void __launch_bounds__(DY_WG)
dy_max_kernel(const double *__restrict__ pts, const int32_t *__restrict__ cnt, int32_t maxn,
              int32_t maxchunks, int split, unsigned long long *__restrict__ smax)
{
    __shared__ double wmax[DY_WG / EK_WAVE];
    const int tid = threadIdx.x, lane = tid & (EK_WAVE - 1), wave = tid / EK_WAVE;
    const int job = (int)blockIdx.y;
    const DyShape sh = dy_shape(cnt, job);
    int32_t i0, j0, j1;
    if (!dy_part(sh, split, i0, j0, j1))
        return;
    // (a lane past the end takes the block's first point again: a maximum does not mind)
    const int32_t i = (i0 + tid < sh.nbig) ? i0 + tid : i0;
    const double *P = pts + ((size_t)sh.big * maxn + i) * 3;
    const double *Q = pts + (size_t)sh.small * maxn * 3;
    const double px = P[0], py = P[1], pz = P[2];
    double m = 0.0;
    for (int32_t j = j0; j < j1; ++j) {
        const double dx = Q[3 * (size_t)j] - px, dy = Q[3 * (size_t)j + 1] - py,
                     dz = Q[3 * (size_t)j + 2] - pz;
        const double s = (dx * dx + dy * dy) + dz * dz;
        m = (s > m) ? s : m;
    }
    for (int o = EK_WAVE / 2; o > 0; o >>= 1) {
        const double v = __shfl_xor(m, o);
        m = (v > m) ? v : m;
    }
    if (lane == 0)
        wmax[wave] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < DY_WG / EK_WAVE; ++w)
            m = (wmax[w] > m) ? wmax[w] : m;
        atomicMax(&smax[(size_t)job * maxchunks + i0 / sh.L],
                  (unsigned long long)__double_as_longlong(m));
    }
}

__global__ void __launch_bounds__(DY_WG)
dy_plan_kernel(const int32_t *__restrict__ cnt, int32_t n_jobs, int32_t maxchunks,
               const unsigned long long *__restrict__ smax, const double *__restrict__ S,
               int32_t nS, int32_t cap, int32_t *__restrict__ nbins_c,
               int32_t *__restrict__ nbins, int32_t *__restrict__ err)
{
    const int64_t t = (int64_t)blockIdx.x * DY_WG + threadIdx.x;
    if (t >= (int64_t)n_jobs * maxchunks)
        return;
    const int job = (int)(t / maxchunks), c = (int)(t % maxchunks);
    const DyShape sh = dy_shape(cnt, job);
    int32_t nb = 0;
    if (c < sh.nchunks) {
        const double s = __longlong_as_double((long long)smax[t]);
        int lo = 0, hi = nS;            // the m in [1, nS] with s >= S[m - 1]
        while (lo < hi) {
            const int mid = (lo + hi) / 2;
            if (s >= S[mid])
                lo = mid + 1;
            else
                hi = mid;
        }
        nb = 2 + lo;
        if (nb > cap) {                 // beyond the bound the host derived: reported, never indexed
            atomicMax(err, 1);
            nb = cap;
        }
        atomicMax(&nbins[job], nb);
    }
    nbins_c[t] = nb;
}

__global__ void __launch_bounds__(DY_WG)
dy_hist_kernel(const double *__restrict__ pts, const int32_t *__restrict__ cnt, int32_t maxn,
               int32_t maxchunks, int split, const int32_t *__restrict__ nbins_c,
               const int32_t *__restrict__ tix, const double *__restrict__ q,
               const float *__restrict__ inv, int32_t cap,
               unsigned long long *__restrict__ hist)
{
    extern __shared__ double dy_lds[];          // cap edges, then cap counts
    double *qs = dy_lds;
    unsigned int *hs = (unsigned int *)(dy_lds + cap);
    const int tid = threadIdx.x;
    const int job = (int)blockIdx.y;
    const DyShape sh = dy_shape(cnt, job);
    int32_t i0, j0, j1;
    if (!dy_part(sh, split, i0, j0, j1))
        return;
    const int32_t nb = nbins_c[(size_t)job * maxchunks + i0 / sh.L];    // 2 <= nb <= cap
    if (nb < 2 || nb > cap)
        return;
    const int32_t t = tix[nb];
    for (int32_t k = tid; k < nb; k += DY_WG) {
        qs[k] = q[(size_t)t * DY_MAX_BINS + k];
        hs[k] = 0u;
    }
    __syncthreads();
    if (i0 + tid < sh.nbig) {
        const float scale = inv[t];
        const double *P = pts + ((size_t)sh.big * maxn + i0 + tid) * 3;
        const double *Q = pts + (size_t)sh.small * maxn * 3;
        const double px = P[0], py = P[1], pz = P[2];
        int32_t cur = 0;
        unsigned int run = 0;
        for (int32_t j = j0; j < j1; ++j) {
            const double dx = Q[3 * (size_t)j] - px, dy = Q[3 * (size_t)j + 1] - py,
                         dz = Q[3 * (size_t)j + 2] - pz;
            const double s = (dx * dx + dy * dy) + dz * dz;
            int32_t k = (int32_t)(sqrtf((float)s) * scale);     // a guess; the table decides
            k = (k < 0) ? 0 : (k > nb - 1) ? nb - 1 : k;
            while (k > 0 && s < qs[k])
                --k;
            while (k + 1 < nb && s >= qs[k + 1])
                ++k;
            if (k != cur) {
                if (run)
                    atomicAdd(&hs[cur], run);
                cur = k;
                run = 0;
            }
            ++run;
        }
        if (run)
            atomicAdd(&hs[cur], run);
    }
    __syncthreads();
    for (int32_t k = tid; k < nb; k += DY_WG)
        if (hs[k])
            atomicAdd(&hist[(size_t)job * cap + k], (unsigned long long)hs[k]);
}

// ---- host: what the stages share -----------------------------------------------------------
static int dy_split(int32_t maxn, int64_t n_jobs)
{
    const int64_t blocks = (int64_t)((maxn + DY_WG - 1) / DY_WG) * n_jobs;
    int64_t s = (2048 + blocks - 1) / blocks;
    return (int)(s < 1 ? 1 : s > DY_MAX_SPLIT ? DY_MAX_SPLIT : s);
}

// max, plan, hist of n_jobs pairs whose clouds and counts are on the device; smax, nbins
// and hist are cleared here
static int dy_launch_pairs(const double *pts, const int32_t *cnt, int32_t maxn, int64_t n_jobs,
                           int32_t maxchunks, const DyTab &T, int32_t cap,
                           unsigned long long *smax, int32_t *nbins_c, int32_t *nbins,
                           int32_t *err, unsigned long long *hist, hipStream_t s)
{
    int rc = EK_OK;
    const int split = dy_split(maxn, n_jobs);
    const dim3 grid((unsigned)((maxn + DY_WG - 1) / DY_WG), (unsigned)n_jobs, (unsigned)split);
    const size_t cells = (size_t)n_jobs * maxchunks;
    DY_HIP(hipMemsetAsync(smax, 0, cells * sizeof(unsigned long long), s));
    DY_HIP(hipMemsetAsync(nbins, 0, (size_t)n_jobs * sizeof(int32_t), s));
    DY_HIP(hipMemsetAsync(err, 0, sizeof(int32_t), s));
    DY_HIP(hipMemsetAsync(hist, 0, (size_t)n_jobs * cap * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(dy_max_kernel, grid, dim3(DY_WG), 0, s, pts, cnt, maxn, maxchunks, split,
                       smax);
    hipLaunchKernelGGL(dy_plan_kernel, dim3((unsigned)((cells + DY_WG - 1) / DY_WG)), dim3(DY_WG),
                       0, s, cnt, (int32_t)n_jobs, maxchunks, smax, T.S, T.nS, cap, nbins_c,
                       nbins, err);
    hipLaunchKernelGGL(dy_hist_kernel, grid, dim3(DY_WG),
                       (size_t)cap * (sizeof(double) + sizeof(unsigned int)), s, pts, cnt, maxn,
                       maxchunks, split, nbins_c, T.tix, T.q, T.inv, cap, hist);
    DY_HIP(hipGetLastError());
done:
    return rc;
}

static int dy_cap(double diag, double w, const char *who, int32_t *cap)
{
    if (!(diag < (double)(DY_MAX_BINS - 3) * w))
        return ek_set_error(EK_EARG, "%s: the clouds span %g nm, not below %d bin widths of %g "
                                     "nm", who, diag, DY_MAX_BINS - 3, w);
    const int64_t c = (int64_t)(diag / w) + 4;
    *cap = (int32_t)(c > DY_MAX_BINS ? DY_MAX_BINS : c);
    return EK_OK;
}

static int dy_check_width(double w, const char *who)
{
    if (!(w >= DY_MIN_WIDTH && w <= DY_MAX_WIDTH))
        return ek_set_error(EK_EARG, "%s: bin_width = %g is not in [2^-40, 2^40] nm", who, w);
    return EK_OK;
}

static int dy_check_coords(const float *x, size_t n, const char *who, const char *what)
{
    for (size_t q = 0; q < n; ++q)
        if (!(fabs((double)x[q]) <= DY_MAX_COORD))
            return ek_set_error(EK_EARG, "%s: %s %zu is not finite or beyond 2^20 nm", who, what, q);
    return EK_OK;
}

static int dy_thresholds(const double *cutoff, int32_t atoms, const char *who,
                         std::vector<double> &thr)
{
    try {
        thr.resize(atoms);
    } catch (const std::bad_alloc &) {
        return ek_set_error(EK_ENOMEM, "%s: out of host memory", who);
    }
    for (int32_t i = 0; i < atoms; ++i) {
        if (!(cutoff[i] > 0.0 && cutoff[i] <= DY_MAX_COORD))
            return ek_set_error(EK_EARG, "%s: radius + probe of atom %d is not in (0, 2^20] nm",
                                who, i);
        // kept iff sqrt(s) > cutoff iff sqrt(s) >= the next double iff s >= this
        thr[i] = dy_sq_at_least(nextafter(cutoff[i], INFINITY));
    }
    return EK_OK;
}

static int dy_set_device(int device)
{
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    return EK_OK;
}

// ---- the handle ----------------------------------------------------------------------------
struct ek_dyes {
    int device;
    int32_t atoms, n1, n2, maxn;
    double width, rho;          // bin width; the largest norm of a cloud's point
    double *thr;                // [atoms]
    float *dye1, *dye2;         // [n][3]
    DyTab tab;
    hipStream_t s;
    hipEvent_t ev[5];
    double ms[4];               // uploads, touch + compact, pairs, downloads: the last run's sums
    int64_t frames;             // of the last run
    std::vector<int32_t> kept;  // [frames][4]
    std::vector<int32_t> nbins; // [frames][2]
    std::vector<int64_t> counts;    // [sum of nbins]
};

static int dy_bind(ek_dyes *h, const char *who)
{
    if (!h)
        return ek_set_error(EK_EARG, "%s: null handle", who);
    return dy_set_device(h->device);
}

extern "C" int ek_dyes_close(ek_dyes *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(h->thr);
    (void)ek_dev_free(h->dye1);
    (void)ek_dev_free(h->dye2);
    dy_tab_free(h->tab);
    for (hipEvent_t e : h->ev)
        if (e)
            (void)ek_event_destroy(e);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    delete h;
    return EK_OK;
}

extern "C" int ek_dyes_open(int device, int32_t atoms, const double *cutoff, int32_t n1,
                            const float *dye1, int32_t n2, const float *dye2, double bin_width,
                            ek_dyes **out)
{
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "ek_dyes_open: null output");
    *out = nullptr;
    if (!cutoff || !dye1 || !dye2 || atoms < 1 || n1 < 1 || n2 < 1 || n1 > DY_MAX_POINTS ||
        n2 > DY_MAX_POINTS)
        return ek_set_error(EK_EARG, "ek_dyes_open: bad argument (atoms >= 1, 1 <= points <= %d)",
                            DY_MAX_POINTS);
    if ((rc = dy_check_width(bin_width, "ek_dyes_open")) != EK_OK ||
        (rc = dy_check_coords(dye1, 3 * (size_t)n1, "ek_dyes_open", "dye1 coordinate")) != EK_OK ||
        (rc = dy_check_coords(dye2, 3 * (size_t)n2, "ek_dyes_open", "dye2 coordinate")) != EK_OK)
        return rc;
    std::vector<double> thr;
    if ((rc = dy_thresholds(cutoff, atoms, "ek_dyes_open", thr)) != EK_OK ||
        (rc = dy_set_device(device)) != EK_OK)
        return rc;
    ek_dyes *h = new (std::nothrow) ek_dyes();
    if (!h)
        return ek_set_error(EK_ENOMEM, "ek_dyes_open: out of host memory");
    h->device = device;
    h->atoms = atoms;
    h->n1 = n1;
    h->n2 = n2;
    h->maxn = n1 > n2 ? n1 : n2;
    h->width = bin_width;
    for (int d = 0; d < 2; ++d) {
        const float *p = d ? dye2 : dye1;
        for (int32_t i = 0, n = d ? n2 : n1; i < n; ++i) {
            const double x = p[3 * (size_t)i], y = p[3 * (size_t)i + 1], z = p[3 * (size_t)i + 2];
            const double r = sqrt((x * x + y * y) + z * z);
            h->rho = r > h->rho ? r : h->rho;
        }
    }
    DY_HIP(ek_stream_create_flags(&h->s, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev)
        DY_HIP(ek_event_create(&e));
    DY_HIP(ek_dev_malloc(&h->thr, (size_t)atoms * sizeof(double)));
    DY_HIP(ek_dev_malloc(&h->dye1, 3 * (size_t)n1 * sizeof(float)));
    DY_HIP(ek_dev_malloc(&h->dye2, 3 * (size_t)n2 * sizeof(float)));
    DY_HIP(hipMemcpyAsync(h->thr, thr.data(), (size_t)atoms * sizeof(double),
                          hipMemcpyHostToDevice, h->s));
    DY_HIP(hipMemcpyAsync(h->dye1, dye1, 3 * (size_t)n1 * sizeof(float), hipMemcpyHostToDevice,
                          h->s));
    DY_HIP(hipMemcpyAsync(h->dye2, dye2, 3 * (size_t)n2 * sizeof(float), hipMemcpyHostToDevice,
                          h->s));
    if ((rc = dy_tab_upload(bin_width, h->tab, h->s)) != EK_OK)     // (synchronises the stream)
        goto done;
    *out = h;
    return EK_OK;
done:
    ek_dyes_close(h);
    return rc;
}

// the diagonal of the box that holds the frame's four placements (see the head of the file)
static double dy_frame_diag(const float *mt, double rho)
{
    double ext2 = 0.0;
    for (int j = 0; j < 3; ++j) {
        double lo = INFINITY, hi = -INFINITY;
        for (int r = 0; r < 2; ++r) {
            const float *m = mt + 12 * r;
            const double a = m[j], b = m[3 + j], c = m[6 + j], t = m[9 + j];
            const double reach = rho * sqrt((a * a + b * b) + c * c);
            const double rj = (reach + (fabs(t) + reach) * 0x1p-20) * (1.0 + 0x1p-16);
            lo = (t - rj < lo) ? t - rj : lo;
            hi = (t + rj > hi) ? t + rj : hi;
        }
        ext2 += (hi - lo) * (hi - lo);
    }
    return sqrt(ext2);
}

extern "C" int ek_dyes_run(ek_dyes *h, const float *xyz, int64_t frames, const float *Mt,
                           int64_t chunk_frames)
{
    int rc = dy_bind(h, "ek_dyes_run");
    if (rc != EK_OK)
        return rc;
    if (!xyz || !Mt || frames < 0 || chunk_frames < 0 || chunk_frames > DY_MAX_FRAMES)
        return ek_set_error(EK_EARG, "ek_dyes_run: bad argument (0 <= chunk_frames <= %d)",
                            DY_MAX_FRAMES);
    h->ms[0] = h->ms[1] = h->ms[2] = h->ms[3] = 0.0;
    h->frames = 0;
    h->kept.clear();
    h->nbins.clear();
    h->counts.clear();
    if (frames == 0)
        return EK_OK;
    if ((rc = dy_check_coords(xyz, (size_t)frames * h->atoms * 3, "ek_dyes_run",
                              "coordinate")) != EK_OK ||
        (rc = dy_check_coords(Mt, (size_t)frames * 24, "ek_dyes_run", "entry of Mt")) != EK_OK)
        return rc;
    double diag = 0.0;
    for (int64_t f = 0; f < frames; ++f) {
        const double d = dy_frame_diag(Mt + 24 * (size_t)f, h->rho);
        diag = d > diag ? d : diag;
    }
    int32_t cap = 0;
    if ((rc = dy_cap(diag, h->width, "ek_dyes_run", &cap)) != EK_OK)
        return rc;

    const int32_t maxn = h->maxn, maxchunks = (maxn + DY_CHUNK - 1) / DY_CHUNK;
    // the device's answer for a frame: kept [4], nbins [2], counts [2][cap]
    const size_t out_frame = 6 * sizeof(int32_t) + 2 * (size_t)cap * sizeof(int64_t);
    const size_t per_frame = (size_t)h->atoms * 3 * sizeof(float) + 24 * sizeof(float) +
                             4 * (size_t)maxn * (1 + 3 * sizeof(double)) +
                             2 * (size_t)maxchunks * (sizeof(int64_t) + sizeof(int32_t)) +
                             out_frame;
    int64_t chunk = chunk_frames;
    if (chunk == 0) {
        size_t free_b = 0, total_b = 0;
        hipError_t e = hipMemGetInfo(&free_b, &total_b);
        if (e != hipSuccess)
            return ek_set_error(EK_EHIP, "ek_dyes_run: hipMemGetInfo: %s", hipGetErrorString(e));
        chunk = (int64_t)(free_b / 2 / per_frame);
        if (chunk < 1)
            return ek_set_error(EK_ENOMEM, "ek_dyes_run: one frame of %d atoms and clouds of %d "
                                           "points does not fit %zu MiB of free device memory",
                                h->atoms, maxn, free_b >> 20);
        if (chunk > DY_MAX_FRAMES)
            chunk = DY_MAX_FRAMES;
    }
    if (chunk > frames)
        chunk = frames;
    rc = ek_mi_check_memory((size_t)chunk * per_frame + 16, "ek_dyes_run");
    if (rc != EK_OK)
        return rc;

    float *d_xyz = nullptr, *d_Mt = nullptr;
    uint8_t *d_keep = nullptr;
    double *d_pts = nullptr;
    unsigned long long *d_smax = nullptr;
    int32_t *d_nbc = nullptr;
    unsigned char *d_out = nullptr;     // hist [2 chunk][cap] | kept [4 chunk] | nbins [2 chunk] | err
    std::vector<unsigned char> host;
    const size_t hist_bytes = 2 * (size_t)chunk * cap * sizeof(int64_t);
    const size_t out_bytes = hist_bytes + ((size_t)chunk * 6 + 2) * sizeof(int32_t);
    try {
        host.resize(out_bytes);
        h->kept.reserve((size_t)frames * 4);
        h->nbins.reserve((size_t)frames * 2);
    } catch (const std::bad_alloc &) {
        return ek_set_error(EK_ENOMEM, "ek_dyes_run: out of host memory");
    }
    DY_HIP(ek_dev_malloc(&d_xyz, (size_t)chunk * h->atoms * 3 * sizeof(float)));
    DY_HIP(ek_dev_malloc(&d_Mt, (size_t)chunk * 24 * sizeof(float)));
    DY_HIP(ek_dev_malloc(&d_keep, 4 * (size_t)chunk * maxn));
    DY_HIP(ek_dev_malloc(&d_pts, 4 * (size_t)chunk * maxn * 3 * sizeof(double)));
    DY_HIP(ek_dev_malloc(&d_smax, 2 * (size_t)chunk * maxchunks * sizeof(unsigned long long)));
    DY_HIP(ek_dev_malloc(&d_nbc, 2 * (size_t)chunk * maxchunks * sizeof(int32_t)));
    DY_HIP(ek_dev_malloc(&d_out, out_bytes));
    for (int64_t f0 = 0; f0 < frames; f0 += chunk) {
        const int64_t nf = (frames - f0 < chunk) ? frames - f0 : chunk;
        unsigned long long *d_hist = (unsigned long long *)d_out;
        int32_t *d_kept = (int32_t *)(d_out + hist_bytes), *d_nbins = d_kept + 4 * chunk,
                *d_err = d_nbins + 2 * chunk;
        DY_HIP(hipEventRecord(h->ev[0], h->s));
        DY_HIP(hipMemcpyAsync(d_xyz, xyz + (size_t)f0 * h->atoms * 3,
                              (size_t)nf * h->atoms * 3 * sizeof(float), hipMemcpyHostToDevice,
                              h->s));
        DY_HIP(hipMemcpyAsync(d_Mt, Mt + (size_t)f0 * 24, (size_t)nf * 24 * sizeof(float),
                              hipMemcpyHostToDevice, h->s));
        DY_HIP(hipEventRecord(h->ev[1], h->s));
        hipLaunchKernelGGL(dy_touch_kernel,
                           dim3((unsigned)((maxn + DY_WG - 1) / DY_WG), (unsigned)(4 * nf)),
                           dim3(DY_WG), 0, h->s, d_xyz, h->atoms, h->thr, d_Mt, h->dye1, h->n1,
                           h->dye2, h->n2, maxn, d_keep);
        hipLaunchKernelGGL(dy_compact_kernel, dim3((unsigned)(4 * nf)), dim3(DY_WG), 0, h->s,
                           d_keep, d_Mt, h->dye1, h->n1, h->dye2, h->n2, maxn, d_pts, d_kept);
        DY_HIP(hipEventRecord(h->ev[2], h->s));
        if ((rc = dy_launch_pairs(d_pts, d_kept, maxn, 2 * nf, maxchunks, h->tab, cap, d_smax,
                                  d_nbc, d_nbins, d_err, d_hist, h->s)) != EK_OK)
            goto done;
        DY_HIP(hipEventRecord(h->ev[3], h->s));
        DY_HIP(hipMemcpyAsync(host.data(), d_out, out_bytes, hipMemcpyDeviceToHost, h->s));
        DY_HIP(hipEventRecord(h->ev[4], h->s));
        DY_HIP(hipStreamSynchronize(h->s));
        for (int q = 0; q < 4; ++q) {
            float ms = 0.f;
            DY_HIP(hipEventElapsedTime(&ms, h->ev[q], h->ev[q + 1]));
            h->ms[q] += ms;
        }
        const int64_t *hist = (const int64_t *)host.data();
        const int32_t *kept = (const int32_t *)(host.data() + hist_bytes), *nbins = kept + 4 * chunk,
                      *err = nbins + 2 * chunk;
        if (*err) {
            rc = ek_set_error(EK_EARG, "ek_dyes_run: a histogram of frames %lld .. needs more "
                                       "than %d bins", (long long)f0, cap);
            goto done;
        }
        try {
            h->kept.insert(h->kept.end(), kept, kept + 4 * nf);
            h->nbins.insert(h->nbins.end(), nbins, nbins + 2 * nf);
            for (int64_t j = 0; j < 2 * nf; ++j)
                h->counts.insert(h->counts.end(), hist + (size_t)j * cap,
                                 hist + (size_t)j * cap + nbins[j]);
        } catch (const std::bad_alloc &) {
            rc = ek_set_error(EK_ENOMEM, "ek_dyes_run: out of host memory");
            goto done;
        }
    }
    h->frames = frames;
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_xyz);
    (void)ek_dev_free(d_Mt);
    (void)ek_dev_free(d_keep);
    (void)ek_dev_free(d_pts);
    (void)ek_dev_free(d_smax);
    (void)ek_dev_free(d_nbc);
    (void)ek_dev_free(d_out);
    if (rc != EK_OK) {
        h->kept.clear();
        h->nbins.clear();
        h->counts.clear();
    }
    return rc;
}

extern "C" int ek_dyes_counts(ek_dyes *h, int64_t frames, int32_t *kept_out, int32_t *nbins_out)
{
    if (!h || !kept_out || !nbins_out)
        return ek_set_error(EK_EARG, "ek_dyes_counts: null argument");
    if (frames != h->frames)
        return ek_set_error(EK_ESTATE, "ek_dyes_counts: the last run had %lld frames, not %lld",
                            (long long)h->frames, (long long)frames);
    for (size_t q = 0; q < h->kept.size(); ++q)
        kept_out[q] = h->kept[q];
    for (size_t q = 0; q < h->nbins.size(); ++q)
        nbins_out[q] = h->nbins[q];
    return EK_OK;
}

extern "C" int ek_dyes_fetch(ek_dyes *h, int64_t *counts_out)
{
    if (!h || (!counts_out && !h->counts.empty()))
        return ek_set_error(EK_EARG, "ek_dyes_fetch: null argument");
    for (size_t q = 0; q < h->counts.size(); ++q)
        counts_out[q] = h->counts[q];
    return EK_OK;
}

extern "C" int ek_dyes_last_timing(ek_dyes *h, double *ms_out)
{
    if (!h || !ms_out)
        return ek_set_error(EK_EARG, "ek_dyes_last_timing: null argument");
    for (int i = 0; i < 4; ++i)
        ms_out[i] = h->ms[i];
    return EK_OK;
}

// ---- each stage alone ----------------------------------------------------------------------
extern "C" int ek_dyes_touches(int device, const float *xyz, int32_t atoms, const double *cutoff,
                               const float *coords, int32_t n, uint8_t *keep_out)
{
    int rc = EK_OK;
    if (!xyz || !cutoff || !coords || !keep_out || atoms < 1 || n < 1 || n > DY_MAX_POINTS)
        return ek_set_error(EK_EARG, "ek_dyes_touches: bad argument (atoms >= 1, 1 <= points <= "
                                     "%d)", DY_MAX_POINTS);
    if ((rc = dy_check_coords(xyz, 3 * (size_t)atoms, "ek_dyes_touches", "coordinate")) != EK_OK ||
        (rc = dy_check_coords(coords, 3 * (size_t)n, "ek_dyes_touches", "point coordinate")) !=
            EK_OK)
        return rc;
    std::vector<double> thr;
    if ((rc = dy_thresholds(cutoff, atoms, "ek_dyes_touches", thr)) != EK_OK ||
        (rc = dy_set_device(device)) != EK_OK)
        return rc;
    hipStream_t s = nullptr;
    float *d_xyz = nullptr, *d_c = nullptr;
    double *d_thr = nullptr;
    uint8_t *d_keep = nullptr;
    DY_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    DY_HIP(ek_dev_malloc(&d_xyz, 3 * (size_t)atoms * sizeof(float)));
    DY_HIP(ek_dev_malloc(&d_c, 3 * (size_t)n * sizeof(float)));
    DY_HIP(ek_dev_malloc(&d_thr, (size_t)atoms * sizeof(double)));
    DY_HIP(ek_dev_malloc(&d_keep, (size_t)n));
    DY_HIP(hipMemcpyAsync(d_xyz, xyz, 3 * (size_t)atoms * sizeof(float), hipMemcpyHostToDevice, s));
    DY_HIP(hipMemcpyAsync(d_c, coords, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
    DY_HIP(hipMemcpyAsync(d_thr, thr.data(), (size_t)atoms * sizeof(double),
                          hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(dy_touch_kernel, dim3((unsigned)((n + DY_WG - 1) / DY_WG), 1u), dim3(DY_WG),
                       0, s, d_xyz, atoms, d_thr, (const float *)nullptr, d_c, n, d_c, n, n,
                       d_keep);
    DY_HIP(hipGetLastError());
    DY_HIP(hipMemcpyAsync(keep_out, d_keep, (size_t)n, hipMemcpyDeviceToHost, s));
    DY_HIP(hipStreamSynchronize(s));
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_xyz);
    (void)ek_dev_free(d_c);
    (void)ek_dev_free(d_thr);
    (void)ek_dev_free(d_keep);
    if (s)
        (void)ek_stream_destroy(s);
    return rc;
}

extern "C" int ek_dyes_pair_hist(int device, const float *coords1, int32_t n1,
                                 const float *coords2, int32_t n2, double bin_width,
                                 int32_t *nbins_out, int64_t *counts_out)
{
    int rc = EK_OK;
    if (!coords1 || !coords2 || !nbins_out || !counts_out || n1 < 1 || n2 < 1 ||
        n1 > DY_MAX_POINTS || n2 > DY_MAX_POINTS)
        return ek_set_error(EK_EARG, "ek_dyes_pair_hist: bad argument (1 <= points <= %d)",
                            DY_MAX_POINTS);
    if ((rc = dy_check_width(bin_width, "ek_dyes_pair_hist")) != EK_OK ||
        (rc = dy_check_coords(coords1, 3 * (size_t)n1, "ek_dyes_pair_hist",
                              "coordinate of coords1")) != EK_OK ||
        (rc = dy_check_coords(coords2, 3 * (size_t)n2, "ek_dyes_pair_hist",
                              "coordinate of coords2")) != EK_OK)
        return rc;
    double ext2 = 0.0;
    for (int j = 0; j < 3; ++j) {
        double lo = INFINITY, hi = -INFINITY;
        for (int d = 0; d < 2; ++d) {
            const float *p = d ? coords2 : coords1;
            for (int32_t i = 0, n = d ? n2 : n1; i < n; ++i) {
                const double v = p[3 * (size_t)i + j];
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
        }
        ext2 += (hi - lo) * (hi - lo);
    }
    int32_t cap = 0;
    if ((rc = dy_cap(sqrt(ext2) * (1.0 + 0x1p-16), bin_width, "ek_dyes_pair_hist", &cap)) != EK_OK ||
        (rc = dy_set_device(device)) != EK_OK)
        return rc;
    // the layout of a run of one frame: coords1 in slot 0, coords2 in slot 3, pair 0 only
    const int32_t maxn = n1 > n2 ? n1 : n2, maxchunks = (maxn + DY_CHUNK - 1) / DY_CHUNK;
    const int32_t cnt[4] = {n1, 0, 0, n2};
    std::vector<double> pts;
    try {
        pts.assign(4 * (size_t)maxn * 3, 0.0);
    } catch (const std::bad_alloc &) {
        return ek_set_error(EK_ENOMEM, "ek_dyes_pair_hist: out of host memory");
    }
    for (size_t q = 0; q < 3 * (size_t)n1; ++q)
        pts[q] = (double)coords1[q];
    for (size_t q = 0; q < 3 * (size_t)n2; ++q)
        pts[3 * (size_t)maxn * 3 + q] = (double)coords2[q];
    hipStream_t s = nullptr;
    DyTab T;
    double *d_pts = nullptr;
    int32_t *d_cnt = nullptr, *d_nbc = nullptr, *d_nb = nullptr;
    unsigned long long *d_smax = nullptr, *d_hist = nullptr;
    int32_t nb[2] = {0, 0};
    DY_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    if ((rc = dy_tab_upload(bin_width, T, s)) != EK_OK)
        goto done;
    DY_HIP(ek_dev_malloc(&d_pts, pts.size() * sizeof(double)));
    DY_HIP(ek_dev_malloc(&d_cnt, sizeof(cnt)));
    DY_HIP(ek_dev_malloc(&d_nbc, (size_t)maxchunks * sizeof(int32_t)));
    DY_HIP(ek_dev_malloc(&d_nb, 2 * sizeof(int32_t)));          // nbins, err
    DY_HIP(ek_dev_malloc(&d_smax, (size_t)maxchunks * sizeof(unsigned long long)));
    DY_HIP(ek_dev_malloc(&d_hist, (size_t)cap * sizeof(unsigned long long)));
    DY_HIP(hipMemcpyAsync(d_pts, pts.data(), pts.size() * sizeof(double), hipMemcpyHostToDevice,
                          s));
    DY_HIP(hipMemcpyAsync(d_cnt, cnt, sizeof(cnt), hipMemcpyHostToDevice, s));
    if ((rc = dy_launch_pairs(d_pts, d_cnt, maxn, 1, maxchunks, T, cap, d_smax, d_nbc, d_nb,
                              d_nb + 1, d_hist, s)) != EK_OK)
        goto done;
    for (int k = 0; k < DY_MAX_BINS; ++k)
        counts_out[k] = 0;
    DY_HIP(hipMemcpyAsync(nb, d_nb, sizeof(nb), hipMemcpyDeviceToHost, s));
    DY_HIP(hipMemcpyAsync(counts_out, d_hist, (size_t)cap * sizeof(int64_t),
                          hipMemcpyDeviceToHost, s));
    DY_HIP(hipStreamSynchronize(s));
    if (nb[1]) {
        rc = ek_set_error(EK_EARG, "ek_dyes_pair_hist: the histogram needs more than %d bins", cap);
        goto done;
    }
    *nbins_out = nb[0];
done:
    if (s)
        (void)hipStreamSynchronize(s);
    dy_tab_free(T);
    (void)ek_dev_free(d_pts);
    (void)ek_dev_free(d_cnt);
    (void)ek_dev_free(d_nbc);
    (void)ek_dev_free(d_nb);
    (void)ek_dev_free(d_smax);
    (void)ek_dev_free(d_hist);
    if (s)
        (void)ek_stream_destroy(s);
    return rc;
}
