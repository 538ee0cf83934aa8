// ek_kmc_burst.h -- the burst sampler's chain loop, written once: a device template over the
// rule that colours a photon, and the host side of a call (ek_kmc.hip: the histogram rule;
// ek_dye_bursts.hip: the lifetime and the kappa-squared rule).
//
// A lane is a burst.  Its chain (first_burst + b) starts at the inverse CDF of the populations
// with u(KMC_INIT, chain, 0), hops with u(KMC_TRANS, chain, t) and serves its photons on the
// way: photon ph of the burst, standing at the flat position k, in state s, is
// rule.photon(s, chain, ph, k).  A rule draws from (seed, chain, ph) alone, so the chain is the
// same states whichever rule runs, and nothing depends on step_cap, on how the bursts are cut
// into calls or on whether the trajectories are kept.  A launch covers the frames t0 .. t0 + m
// - 1 in tiles of KMC_TS; (cur, kpos) is all that is carried; trajectories leave through the
// LDS tile as 64-byte runs per chain.  A chain that has to step from an empty row records the
// state in bad[0]; a rule that finds nothing to pick from in a state records it in bad[1]
// (integer atomicMin both); the caller raises.
#pragma once
#include "ek_common.h"
#include "ek_kmc_dev.h"
#include "ek_mi_launch.h"

#include <memory>
#include <new>

extern int ek_set_error(int code, const char *fmt, ...);

#define KMC_HIP(call)                                                               \
    do {                                                                            \
        hipError_t e_ = (call);                                                     \
        if (e_ != hipSuccess)                                                       \
            return ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,           \
                                hipGetErrorString(e_), __FILE__, __LINE__);         \
    } while (0)

#define KMC_LANE_WG 64          // lane form, bursts: one wave a workgroup (one LDS tile)
#define KMC_TS 16               // steps of a tile: 64-byte runs per chain
#define KMC_WG 256
#define KMC_STEP_CAP 16384      // steps of a launch unless the caller says otherwise
#define KMC_NO_BAD 0xffffffffu

// ---- device --------------------------------------------------------------------------------
// tile [64 chains][KMC_TS steps] of one wave -> out: chain c's cnt steps go to out[off ..],
// four chains (64 bytes each) per store instruction.  off, cnt: this lane's chain's.
__device__ __forceinline__ void kmc_tile_flush(const int32_t (*tile)[KMC_TS + 1], int lane,
                                               long long off, int cnt, int32_t *__restrict__ out)
{
#pragma unroll 4
    for (int i = 0; i < EK_WAVE / 4; ++i) {
        const int c = i * 4 + (lane >> 4), j = lane & (KMC_TS - 1);
        const long long offc = __shfl(off, c, EK_WAVE);
        const int cntc = __shfl(cnt, c, EK_WAVE);
        if (j < cntc)
            out[offc + j] = tile[c][j];
    }
}

// what a launch of any rule gets.  cur: the state at frame t0 (t0 > 0), kpos: the first photon
// not yet served.  traj (may be null): flat, burst b's states from toff[b].
struct KmcBurstArgs {
    KmcRows R;
    uint64_t seed;
    int64_t first_burst, n_bursts;
    const int64_t *foff, *frames;
    const double *pop_cdf;
    int32_t *cur;
    int64_t *kpos;
    int64_t t0, m;
    int32_t *traj;
    const int64_t *toff;
    uint32_t *bad;              // [2]: the empty row, the state the rule could not serve
};

// frames t0 .. t0 + m - 1 of every burst that reaches them
template <class Rule>
__device__ __forceinline__ void kmc_burst_loop(const KmcBurstArgs &A, const Rule &rule,
                                               int32_t (*tile)[KMC_TS + 1])
{
    const int lane = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * KMC_LANE_WG + lane;
    const bool live = b < A.n_bursts;
    const uint64_t chain = (uint64_t)(A.first_burst + b);
    const int64_t t0 = A.t0, m = A.m;
    const int64_t *__restrict__ frames = A.frames;
    int32_t *__restrict__ traj = A.traj;
    int64_t k0 = 0, k1 = 0, last = -1, k = 0, tbase = 0;
    int32_t s = 0;
    if (live) {
        k0 = A.foff[b];
        k1 = A.foff[b + 1];
        last = frames[k1 - 1];
        if (traj)
            tbase = A.toff[b];
        if (t0 == 0) {
            s = (int32_t)kmc_upper(A.pop_cdf, 0, A.R.n, kmc_uniform(A.seed, KMC_INIT, chain, 0));
            k = k0;
        } else if (t0 <= last) {
            s = A.cur[b];
            k = A.kpos[b];
        }
    }
    const int64_t tend = last < t0 + m - 1 ? last : t0 + m - 1;    // the last frame done here
    double u0 = 0.0, u1 = 0.0;
    bool first = true;
    for (int64_t tb = t0; __any(tb <= tend); tb += KMC_TS) {
        const int64_t left = tend - tb + 1;
        const int cnt = (int)(left < 0 ? 0 : left < KMC_TS ? left : KMC_TS);
        for (int j = 0; j < cnt; ++j) {
            const int64_t t = tb + j;
            tile[lane][j] = s;
            while (k < k1 && frames[k] == t) {
                rule.photon(s, chain, (uint64_t)(k - k0), k);
                ++k;
            }
            if (t < last) {
                if (!(t & 1) || first)
                    kmc_pair(A.seed, KMC_TRANS, chain, (uint64_t)t >> 1, u0, u1);
                first = false;
                s = kmc_step_lane(A.R, s, (t & 1) ? u1 : u0, A.bad);
            }
        }
        if (traj) {             // (the same in every lane)
            __syncthreads();
            kmc_tile_flush(tile, lane, (long long)(tbase + tb), cnt, traj);
            __syncthreads();
        }
    }
    if (live && t0 + m - 1 < last) {
        A.cur[b] = s;
        A.kpos[b] = k;
    }
}

template <class Rule>
__global__ void __launch_bounds__(KMC_LANE_WG) kmc_burst_kernel(KmcBurstArgs A, Rule rule)
{
    __shared__ int32_t tile[EK_WAVE][KMC_TS + 1];
    kmc_burst_loop(A, rule, tile);
}

// ---- host ----------------------------------------------------------------------------------
// what a call allocated, released whichever way the call returns
struct KmcScope {
    void *ptr[24];
    int n = 0;
    hipStream_t sync = nullptr;     // not owned: waited for before anything is freed
    hipStream_t own = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    template <class T> hipError_t alloc(T **p, size_t bytes)
    {
        if (n >= 24)
            return hipErrorOutOfMemory;
        hipError_t e = ek_dev_malloc((void **)p, bytes ? bytes : 1);
        if (e == hipSuccess)
            ptr[n++] = (void *)*p;
        return e;
    }
    hipError_t events()
    {
        for (hipEvent_t &e : ev) {
            hipError_t r = ek_event_create(&e);
            if (r != hipSuccess)
                return r;
        }
        return hipSuccess;
    }
    // bytes of host memory to a buffer of their own on the device
    template <class T> hipError_t upload(T **p, const T *src, size_t count, hipStream_t s)
    {
        hipError_t e = alloc(p, count * sizeof(T));
        if (e == hipSuccess && count > 0)
            e = hipMemcpyAsync(*p, src, count * sizeof(T), hipMemcpyHostToDevice, s);
        return e;
    }
    ~KmcScope()
    {
        if (sync)
            (void)hipStreamSynchronize(sync);
        if (own)
            (void)hipStreamSynchronize(own);
        for (int i = 0; i < n; ++i)
            (void)ek_dev_free(ptr[i]);
        for (hipEvent_t e : ev)
            if (e)
                (void)ek_event_destroy(e);
        if (own)
            (void)ek_stream_destroy(own);
    }
};

struct ek_kmc {
    int device;
    int32_t n;
    int64_t nnz;
    int64_t *d_indptr;
    int32_t *d_cols;
    double *d_cdf;
    hipStream_t s;
};

static inline KmcRows kmc_rows(const ek_kmc *h)
{
    KmcRows R;
    R.indptr = h->d_indptr;
    R.cols = h->d_cols;
    R.cdf = h->d_cdf;
    R.n = h->n;
    return R;
}

static inline int kmc_set_device(int device)
{
    hipError_t e0 = hipSetDevice(device);
    if (e0 != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
    return EK_OK;
}

static inline unsigned kmc_blocks(int64_t items, int per)
{
    return (unsigned)((items + per - 1) / per);
}

static inline int64_t kmc_bad(uint32_t w) { return w == KMC_NO_BAD ? (int64_t)-1 : (int64_t)w; }

// ms[q] = the time between the scope's events q and q + 1: upload, kernels, download
static inline int kmc_store_ms(KmcScope &sc, double *ms_out)
{
    float ms = 0.f;
    for (int q = 0; q < 3; ++q) {
        KMC_HIP(hipEventElapsedTime(&ms, sc.ev[q], sc.ev[q + 1]));
        ms_out[q] = ms;
    }
    return EK_OK;
}

// The bursts of one call under the rule a plan makes.  A plan is the rule's host side:
//   size_t bytes(int64_t n_ph)                     device bytes of its tables and outputs
//   int upload(KmcScope &, hipStream_t, int64_t n_ph)      allocate and upload them
//   Rule rule(uint64_t seed, uint8_t *d_flags, uint32_t *d_bad_state)
//   int download(hipStream_t, int64_t n_ph)        its outputs, asynchronously
// The driver owns what every rule has: the frames, the populations, (cur, kpos), the flag
// byte per photon, the trajectories and the two bad words.  ms: upload, kernels, download.
template <class Plan>
static inline int kmc_run_bursts(ek_kmc *h, const char *who, double *ms, uint64_t seed,
                                 int64_t first_burst, int64_t n_bursts,
                                 const int64_t *frame_off, const int64_t *frames,
                                 const double *pop_cdf, int64_t step_cap, uint8_t *flags_out,
                                 int32_t *traj_out, int64_t *bad_row_out,
                                 int64_t *bad_state_out, Plan &plan)
{
    int rc = EK_OK;
    if (!h || !frame_off || !frames || !pop_cdf || !flags_out || !bad_row_out || n_bursts < 1 ||
        n_bursts > ((int64_t)1 << 31) || first_burst < 0 || step_cap < 0 ||
        first_burst > ((int64_t)1 << 60) - n_bursts || frame_off[0] != 0)
        return ek_set_error(EK_EARG, "%s: bad argument (1 <= n_bursts <= 2^31, chains below "
                                     "2^60, frame_off[0] == 0, step_cap >= 0)", who);
    int64_t max_last = 0, traj_cells = 0;
    for (int64_t b = 0; b < n_bursts; ++b) {
        if (frame_off[b + 1] <= frame_off[b])
            return ek_set_error(EK_EARG, "%s: burst %lld has no photon", who, (long long)b);
        int64_t prev = 0;
        for (int64_t k = frame_off[b]; k < frame_off[b + 1]; ++k) {
            if (frames[k] < prev || frames[k] >= ((int64_t)1 << 40))
                return ek_set_error(EK_EARG, "%s: the frames of burst %lld are negative, "
                                             "decrease or exceed 2^40", who, (long long)b);
            prev = frames[k];
        }
        max_last = prev > max_last ? prev : max_last;
        traj_cells += prev + 1;
    }
    *bad_row_out = -1;
    if (bad_state_out)
        *bad_state_out = -1;
    if ((rc = kmc_set_device(h->device)) != EK_OK)
        return rc;
    const int64_t n_ph = frame_off[n_bursts];
    const size_t tb = traj_out ? (size_t)traj_cells * sizeof(int32_t) + (size_t)(n_bursts + 1) * 8
                               : 0;
    if ((rc = ek_mi_check_memory(tb + (size_t)n_ph * 9 + (size_t)n_bursts * 20 +
                                 (size_t)h->n * 8 + plan.bytes(n_ph) + 1024, who)) != EK_OK)
        return rc;
    const int64_t cap = step_cap > 0 ? step_cap : KMC_STEP_CAP;
    KmcScope sc;
    sc.sync = h->s;
    hipStream_t s = h->s;
    KmcBurstArgs A;
    int64_t *d_foff = nullptr, *d_frames = nullptr, *d_toff = nullptr;
    double *d_pop = nullptr;
    uint8_t *d_ph = nullptr;
    uint32_t bad[2] = {KMC_NO_BAD, KMC_NO_BAD};
    std::unique_ptr<int64_t[]> toff;
    KMC_HIP(sc.events());
    KMC_HIP(sc.alloc(&d_foff, (size_t)(n_bursts + 1) * sizeof(int64_t)));
    KMC_HIP(sc.alloc(&d_frames, (size_t)n_ph * sizeof(int64_t)));
    KMC_HIP(sc.alloc(&A.kpos, (size_t)n_bursts * sizeof(int64_t)));
    KMC_HIP(sc.alloc(&A.cur, (size_t)n_bursts * sizeof(int32_t)));
    KMC_HIP(sc.alloc(&d_pop, (size_t)h->n * sizeof(double)));
    KMC_HIP(sc.alloc(&d_ph, (size_t)n_ph));
    KMC_HIP(sc.alloc(&A.bad, sizeof(bad)));
    A.traj = nullptr;
    if (traj_out) {
        KMC_HIP(sc.alloc(&A.traj, (size_t)traj_cells * sizeof(int32_t)));
        KMC_HIP(sc.alloc(&d_toff, (size_t)(n_bursts + 1) * sizeof(int64_t)));
        toff.reset(new (std::nothrow) int64_t[n_bursts + 1]);
        if (!toff)
            return ek_set_error(EK_ENOMEM, "%s: out of host memory", who);
        toff[0] = 0;
        for (int64_t b = 0; b < n_bursts; ++b)
            toff[b + 1] = toff[b] + frames[frame_off[b + 1] - 1] + 1;
    }
    KMC_HIP(hipEventRecord(sc.ev[0], s));
    if ((rc = plan.upload(sc, s, n_ph)) != EK_OK)
        return rc;
    KMC_HIP(hipMemcpyAsync(d_foff, frame_off, (size_t)(n_bursts + 1) * sizeof(int64_t),
                           hipMemcpyHostToDevice, s));
    KMC_HIP(hipMemcpyAsync(d_frames, frames, (size_t)n_ph * sizeof(int64_t),
                           hipMemcpyHostToDevice, s));
    KMC_HIP(hipMemcpyAsync(d_pop, pop_cdf, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice,
                           s));
    if (traj_out)
        KMC_HIP(hipMemcpyAsync(d_toff, toff.get(), (size_t)(n_bursts + 1) * sizeof(int64_t),
                               hipMemcpyHostToDevice, s));
    KMC_HIP(hipMemsetAsync(A.bad, 0xff, sizeof(bad), s));
    KMC_HIP(hipStreamSynchronize(s));          // (the host arrays are read by now)
    KMC_HIP(hipEventRecord(sc.ev[1], s));
    A.R = kmc_rows(h);
    A.seed = seed;
    A.first_burst = first_burst;
    A.n_bursts = n_bursts;
    A.foff = d_foff;
    A.frames = d_frames;
    A.pop_cdf = d_pop;
    A.m = cap;
    A.toff = d_toff;
    auto rule = plan.rule(seed, d_ph, A.bad + 1);
    for (int64_t t0 = 0; t0 <= max_last; t0 += cap) {
        A.t0 = t0;
        hipLaunchKernelGGL(kmc_burst_kernel<decltype(rule)>,
                           dim3(kmc_blocks(n_bursts, KMC_LANE_WG)), dim3(KMC_LANE_WG), 0, s, A,
                           rule);
        KMC_HIP(hipGetLastError());
    }
    KMC_HIP(hipEventRecord(sc.ev[2], s));
    KMC_HIP(hipMemcpyAsync(flags_out, d_ph, (size_t)n_ph, hipMemcpyDeviceToHost, s));
    if ((rc = plan.download(s, n_ph)) != EK_OK)
        return rc;
    if (traj_out)
        KMC_HIP(hipMemcpyAsync(traj_out, A.traj, (size_t)traj_cells * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
    KMC_HIP(hipMemcpyAsync(bad, A.bad, sizeof(bad), hipMemcpyDeviceToHost, s));
    KMC_HIP(hipEventRecord(sc.ev[3], s));
    KMC_HIP(hipStreamSynchronize(s));
    if ((rc = kmc_store_ms(sc, ms)) != EK_OK)
        return rc;
    *bad_row_out = kmc_bad(bad[0]);
    if (bad_state_out)
        *bad_state_out = kmc_bad(bad[1]);
    return EK_OK;
}
