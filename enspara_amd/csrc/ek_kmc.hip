// ek_kmc.hip -- kinetic Monte Carlo on a transition matrix, smFRET burst sampling and the
// propagation of an ensemble.
//
// Replaces enspara/msm/synthetic_data.py (synthetic_trajectory :15-46, synthetic_ensemble
// :49-103) and the burst sampling of enspara/geometry/dyes_from_expt_dist.py
// (sample_FE_probs :546-559, _sample_FRET_histograms :562-604).  DESIGN.md 4k is the
// contract; in short:
//
// Uniforms.  Philox4x32-10, key = the 64-bit seed (low word first), counter = {i lo, i hi,
//   chain lo, stream << 28 | chain hi} with i = index >> 1.  The call's words a, b, c, d
//   give the doubles ((a >> 5) * 2^26 + (b >> 6)) * 2^-53 (index even) and the same of
//   c, d (index odd), both in [0, 1).  Streams: KMC_TRANS (index = the step left), KMC_INIT
//   (index 0), KMC_BIN, KMC_JITTER, KMC_COIN (index = the photon within its burst).
// A step.  The rows of T live compressed (indptr, cols, cdf = cumsum(nonzeros) / last, built
//   by the host).  The next state is the column of the first cdf entry > u: numpy's
//   Generator.choice(n, 1, p=row) fed the same double.
//   lane form   a lane per chain, binary search (kmc_upper); 16 steps are gathered in an
//               LDS tile per wave and written as 64-byte runs per chain (kmc_tile_flush)
//   wave form   a wave per chain: while the row is longer than 64 the lanes probe 64
//               evenly spaced pivots and a ballot picks the stretch (rows up to 4096
//               nonzeros: one such round), then one load per lane and a ballot.  Lane l
//               draws the double of step base + l; the states of 64 steps leave in one
//               256-byte store.
//   Both search the same cdf for the same first entry > u, so the states are the same.
//   A launch covers at most `step_cap` steps; (state, step index) is all that is carried.
// Ensemble.  p <- p T in a fixed order: dense, column j adds p[i] * T[i][j] over blocks of
//   KMC_ENS_ROWS rows in row order (lanes along the columns), then the blocks' partial sums
//   in block order; column-compressed, column j adds vals[k] * p[rows[k]] in storage
//   order.  p . observable: 256 partial sums over k = tid, tid + 256, .., then a tree
//   in the LDS.  No float atomics anywhere.
// Bursts.  A lane per burst: the chain starts at the inverse CDF of the populations, runs
//   to the burst's last frame and serves its photons on the way: bin by inverse CDF of the
//   state's histogram, d = centre + (u * bin_width - bin_width / 2), d2 = d * d, d6 = d2 *
//   d2 * d2, E = r06 / (r06 + d6), acceptor iff coin <= E.  One byte per photon.  The chain loop
//   and the host side of a call are ek_kmc_burst.h's, shared with the explicit-dye rules of
//   ek_dye_bursts.hip; this file has the histogram rule (KmcHistRule).
// A chain that has to step from a row without nonzeros records the state (integer
// atomicMin) and stays; the caller raises.
#include "ek_kmc_burst.h"

#define KMC_WAVE_WG 256         // wave form: four chains a workgroup
#define KMC_BUF_BYTES ((int64_t)256 << 20)  // the trajectories' device buffer
#define KMC_MIN_CHUNK 1024      // steps of a buffer at least, before the chains are split
#define KMC_WAVE_MAX_CHAINS 2048    // form 0: up to this many chains take a wave each
#define KMC_ENS_ROWS 64

static double kmc_ms[3];        // upload, kernels, download of the last call

struct KmcDist {
    const int64_t *off;         // [n_states + 1]
    const double *centres, *cdf;
};

// ---- the search (kmc_upper, kmc_step_lane: ek_kmc_dev.h) -------------------------------------
// s and u are the same in every lane of the wave
__device__ __forceinline__ int32_t kmc_step_wave(const KmcRows &R, int32_t s, double u, int lane,
                                                 uint32_t *bad)
{
    int64_t lo = R.indptr[s];
    int64_t len = R.indptr[s + 1] - lo;
    if (len <= 0) {
        if (lane == 0)
            atomicMin(bad, (uint32_t)s);
        return s;
    }
    while (len > EK_WAVE) {
        const int64_t stride = (len + EK_WAVE - 1) / EK_WAVE;
        const int64_t e = (int64_t)(lane + 1) * stride;
        const int64_t p = lo + (e < len ? e : len) - 1;
        const unsigned long long mask = __ballot(R.cdf[p] > u);
        // (no pivot > u cannot be for u < 1, the last cdf being 1.0: then the last stretch)
        const int64_t j = mask ? (int64_t)(__ffsll(mask) - 1) : (len - 1) / stride;
        const int64_t b = j * stride, e1 = (j + 1) * stride;
        len = (e1 < len ? e1 : len) - b;     // (lane j is the first whose pivot is > u: b < len)
        lo += b;
    }
    const bool pred = lane < len && R.cdf[lo + (lane < len ? lane : 0)] > u;
    const unsigned long long mask = __ballot(pred);
    const int64_t k = mask ? (int64_t)(__ffsll(mask) - 1) : len - 1;
    return R.cols[lo + k];
}

// ---- chains --------------------------------------------------------------------------------
// draws t0 .. t0 + m - 1 of every chain: state after draw t0 + j -> out[c * ld + col0 + j]
__global__ void __launch_bounds__(KMC_LANE_WG)
kmc_lane_kernel(KmcRows R, uint64_t seed, int64_t first_chain, int64_t n_chains,
                int32_t *__restrict__ cur, int64_t t0, int64_t m, int32_t *__restrict__ out,
                int64_t ld, int64_t col0, uint32_t *__restrict__ bad)
{
    __shared__ int32_t tile[EK_WAVE][KMC_TS + 1];
    const int lane = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * KMC_LANE_WG + lane;
    const bool live = c < n_chains;
    const uint64_t chain = (uint64_t)(first_chain + c);
    int32_t s = live ? cur[c] : 0;
    double u0 = 0.0, u1 = 0.0;
    for (int64_t j0 = 0; j0 < m; j0 += KMC_TS) {        // (m is the same in every lane)
        const int cnt = (int)(m - j0 < KMC_TS ? m - j0 : KMC_TS);
        if (live) {
            for (int j = 0; j < cnt; ++j) {
                const uint64_t idx = (uint64_t)(t0 + j0 + j);
                if (!(idx & 1) || (j0 == 0 && j == 0))
                    kmc_pair(seed, KMC_TRANS, chain, idx >> 1, u0, u1);
                s = kmc_step_lane(R, s, (idx & 1) ? u1 : u0, bad);
                tile[lane][j] = s;
            }
        }
        __syncthreads();
        kmc_tile_flush(tile, lane, (long long)(c * ld + col0 + j0), live ? cnt : 0, out);
        __syncthreads();
    }
    if (live)
        cur[c] = s;
}

__global__ void __launch_bounds__(KMC_WAVE_WG)
kmc_wave_kernel(KmcRows R, uint64_t seed, int64_t first_chain, int64_t n_chains,
                int32_t *__restrict__ cur, int64_t t0, int64_t m, int32_t *__restrict__ out,
                int64_t ld, int64_t col0, uint32_t *__restrict__ bad)
{
    const int lane = threadIdx.x & (EK_WAVE - 1);
    const int64_t c = (int64_t)blockIdx.x * (KMC_WAVE_WG / EK_WAVE) + threadIdx.x / EK_WAVE;
    if (c >= n_chains)          // (whole waves leave; no barrier below)
        return;
    const uint64_t chain = (uint64_t)(first_chain + c);
    int32_t s = cur[c];
    for (int64_t j0 = 0; j0 < m; j0 += EK_WAVE) {
        const int cnt = (int)(m - j0 < EK_WAVE ? m - j0 : EK_WAVE);
        const double mine = kmc_uniform(seed, KMC_TRANS, chain, (uint64_t)(t0 + j0 + lane));
        int32_t keep = 0;
        for (int j = 0; j < cnt; ++j) {
            const double u = __shfl(mine, j, EK_WAVE);
            s = __builtin_amdgcn_readfirstlane(kmc_step_wave(R, s, u, lane, bad));
            if (lane == j)
                keep = s;
        }
        if (lane < cnt)
            out[c * ld + col0 + j0 + lane] = keep;
    }
    if (lane == 0)
        cur[c] = s;
}

__global__ void __launch_bounds__(KMC_WG)
kmc_next_kernel(KmcRows R, int64_t n, const int32_t *__restrict__ states,
                const double *__restrict__ u, int32_t *__restrict__ next, uint32_t *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * KMC_WG + threadIdx.x;
    if (i >= n)
        return;
    const int32_t s = states[i];
    if (s < 0 || s >= R.n) {    // (the host has checked; never out of bounds)
        next[i] = -1;
        return;
    }
    next[i] = kmc_step_lane(R, s, u[i], bad);
}

// ---- photons -------------------------------------------------------------------------------
__device__ __forceinline__ double kmc_photon_E(const KmcDist &D, int32_t s, double u_bin,
                                               double u_jit, double bw, double r06)
{
    const int64_t k = kmc_upper(D.cdf, D.off[s], D.off[s + 1], u_bin);
    const double d = D.centres[k] + (u_jit * bw - bw / 2.0);
    const double d2 = d * d;
    const double d6 = d2 * d2 * d2;
    return r06 / (r06 + d6);
}

__global__ void __launch_bounds__(KMC_WG)
kmc_fret_probs_kernel(KmcDist D, int32_t n_states, uint64_t seed, uint64_t chain, int64_t n,
                      const int32_t *__restrict__ states, double bw, double r06,
                      double *__restrict__ E)
{
    const int64_t k = (int64_t)blockIdx.x * KMC_WG + threadIdx.x;
    if (k >= n)
        return;
    const int32_t s = states[k];
    if (s < 0 || s >= n_states || D.off[s + 1] <= D.off[s]) {   // (the host has checked)
        E[k] = 0.0;
        return;
    }
    E[k] = kmc_photon_E(D, s, kmc_uniform(seed, KMC_BIN, chain, (uint64_t)k),
                        kmc_uniform(seed, KMC_JITTER, chain, (uint64_t)k), bw, r06);
}

// the histogram rule of the burst loop (ek_kmc_burst.h): a distance from the state's histogram,
// its efficiency, a coin
struct KmcHistRule {
    KmcDist D;
    uint64_t seed;
    double bw, r06;
    uint8_t *photons;
    __device__ __forceinline__ void photon(int32_t s, uint64_t chain, uint64_t ph, int64_t k) const
    {
        const double E = kmc_photon_E(D, s, kmc_uniform(seed, KMC_BIN, chain, ph),
                                      kmc_uniform(seed, KMC_JITTER, chain, ph), bw, r06);
        photons[k] = kmc_uniform(seed, KMC_COIN, chain, ph) <= E ? 1 : 0;
    }
};

// ---- ensemble ------------------------------------------------------------------------------
__global__ void __launch_bounds__(KMC_WG)
kmc_ens_part_kernel(const double *__restrict__ T, const double *__restrict__ p, int32_t n,
                    double *__restrict__ part)
{
    const int64_t j = (int64_t)blockIdx.x * KMC_WG + threadIdx.x;
    if (j >= n)
        return;
    const int64_t i0 = (int64_t)blockIdx.y * KMC_ENS_ROWS;
    const int64_t i1 = i0 + KMC_ENS_ROWS < n ? i0 + KMC_ENS_ROWS : n;
    double acc = 0.0;
#pragma unroll 8
    for (int64_t i = i0; i < i1; ++i)
        acc = acc + p[i] * T[i * n + j];
    part[(int64_t)blockIdx.y * n + j] = acc;
}

__global__ void __launch_bounds__(KMC_WG)
kmc_ens_sum_kernel(const double *__restrict__ part, int32_t blocks, int32_t n,
                   double *__restrict__ pn)
{
    const int64_t j = (int64_t)blockIdx.x * KMC_WG + threadIdx.x;
    if (j >= n)
        return;
    double acc = 0.0;
    for (int32_t r = 0; r < blocks; ++r)
        acc = acc + part[(int64_t)r * n + j];
    pn[j] = acc;
}

__global__ void __launch_bounds__(KMC_WG)
kmc_ens_csc_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rows,
                   const double *__restrict__ vals, const double *__restrict__ p, int32_t n,
                   double *__restrict__ pn)
{
    const int64_t j = (int64_t)blockIdx.x * KMC_WG + threadIdx.x;
    if (j >= n)
        return;
    double acc = 0.0;
    for (int64_t k = colptr[j]; k < colptr[j + 1]; ++k)
        acc = acc + vals[k] * p[rows[k]];
    pn[j] = acc;
}

// one workgroup: out[0] = p . o
__global__ void __launch_bounds__(KMC_WG)
kmc_ens_dot_kernel(const double *__restrict__ p, const double *__restrict__ o, int32_t n,
                   double *__restrict__ out)
{
    __shared__ double sh[KMC_WG];
    double acc = 0.0;
    for (int32_t k = threadIdx.x; k < n; k += KMC_WG)
        acc = acc + p[k] * o[k];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int off = KMC_WG / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off)
            sh[threadIdx.x] = sh[threadIdx.x] + sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        out[0] = sh[0];
}

// ---- host ----------------------------------------------------------------------------------
extern "C" int ek_kmc_create(int device, int32_t n_states, const int64_t *indptr,
                             const int32_t *cols, const double *cdf, ek_kmc **out)
{
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "ek_kmc_create: null argument");
    *out = nullptr;
    if (n_states < 1 || !indptr || indptr[0] != 0)
        return ek_set_error(EK_EARG, "ek_kmc_create: n_states >= 1, indptr[0] == 0");
    for (int32_t i = 0; i < n_states; ++i)
        if (indptr[i + 1] < indptr[i])
            return ek_set_error(EK_EARG, "ek_kmc_create: indptr descends at row %d", i);
    const int64_t nnz = indptr[n_states];
    if (nnz > 0 && (!cols || !cdf))
        return ek_set_error(EK_EARG, "ek_kmc_create: null argument");
    for (int64_t k = 0; k < nnz; ++k)
        if (cols[k] < 0 || cols[k] >= n_states)
            return ek_set_error(EK_EARG, "ek_kmc_create: column %d of entry %lld is no state",
                                cols[k], (long long)k);
    if ((rc = kmc_set_device(device)) != EK_OK)
        return rc;
    const size_t ib = (size_t)(n_states + 1) * sizeof(int64_t), cb = (size_t)nnz * sizeof(int32_t),
                 fb = (size_t)nnz * sizeof(double);
    if ((rc = ek_mi_check_memory(ib + cb + fb, "ek_kmc_create")) != EK_OK)
        return rc;
    ek_kmc *h = new (std::nothrow) ek_kmc();
    if (!h)
        return ek_set_error(EK_ENOMEM, "ek_kmc_create: out of host memory");
    h->device = device;
    h->n = n_states;
    h->nnz = nnz;
    hipError_t e = ek_stream_create_flags(&h->s, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&h->d_indptr, ib);
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&h->d_cols, cb ? cb : 1);
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&h->d_cdf, fb ? fb : 1);
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->d_indptr, indptr, ib, hipMemcpyHostToDevice, h->s);
    if (e == hipSuccess && nnz > 0)
        e = hipMemcpyAsync(h->d_cols, cols, cb, hipMemcpyHostToDevice, h->s);
    if (e == hipSuccess && nnz > 0)
        e = hipMemcpyAsync(h->d_cdf, cdf, fb, hipMemcpyHostToDevice, h->s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(h->s);
    if (e != hipSuccess) {
        rc = ek_set_error(EK_EHIP, "ek_kmc_create: %s", hipGetErrorString(e));
        (void)ek_dev_free(h->d_indptr);
        (void)ek_dev_free(h->d_cols);
        (void)ek_dev_free(h->d_cdf);
        if (h->s)
            (void)ek_stream_destroy(h->s);
        delete h;
        return rc;
    }
    *out = h;
    return EK_OK;
}

extern "C" int ek_kmc_destroy(ek_kmc *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(h->d_indptr);
    (void)ek_dev_free(h->d_cols);
    (void)ek_dev_free(h->d_cdf);
    (void)ek_stream_destroy(h->s);
    delete h;
    return EK_OK;
}

extern "C" int ek_kmc_next(ek_kmc *h, int64_t n, const int32_t *states, const double *u,
                           int32_t *next_out, int64_t *bad_out)
{
    int rc = EK_OK;
    if (!h || n < 1 || n > ((int64_t)1 << 36) || !states || !u || !next_out || !bad_out)
        return ek_set_error(EK_EARG, "ek_kmc_next: bad argument (1 <= n <= 2^36)");
    if ((rc = kmc_set_device(h->device)) != EK_OK ||
        (rc = ek_mi_check_memory((size_t)n * 16 + 256, "ek_kmc_next")) != EK_OK)
        return rc;
    KmcScope sc;
    sc.sync = h->s;
    int32_t *d_s = nullptr, *d_next = nullptr;
    double *d_u = nullptr;
    uint32_t *d_bad = nullptr, bad = KMC_NO_BAD;
    KMC_HIP(sc.events());
    KMC_HIP(sc.alloc(&d_s, (size_t)n * sizeof(int32_t)));
    KMC_HIP(sc.alloc(&d_next, (size_t)n * sizeof(int32_t)));
    KMC_HIP(sc.alloc(&d_u, (size_t)n * sizeof(double)));
    KMC_HIP(sc.alloc(&d_bad, sizeof(uint32_t)));
    KMC_HIP(hipEventRecord(sc.ev[0], h->s));
    KMC_HIP(hipMemcpyAsync(d_s, states, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->s));
    KMC_HIP(hipMemcpyAsync(d_u, u, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->s));
    KMC_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(uint32_t), h->s));
    KMC_HIP(hipEventRecord(sc.ev[1], h->s));
    hipLaunchKernelGGL(kmc_next_kernel, dim3(kmc_blocks(n, KMC_WG)), dim3(KMC_WG), 0, h->s,
                       kmc_rows(h), n, d_s, d_u, d_next, d_bad);
    KMC_HIP(hipGetLastError());
    KMC_HIP(hipEventRecord(sc.ev[2], h->s));
    KMC_HIP(hipMemcpyAsync(next_out, d_next, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost,
                           h->s));
    KMC_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, h->s));
    KMC_HIP(hipEventRecord(sc.ev[3], h->s));
    KMC_HIP(hipStreamSynchronize(h->s));
    *bad_out = kmc_bad(bad);
    return kmc_store_ms(sc, kmc_ms);
}

extern "C" int ek_kmc_trajectories(ek_kmc *h, uint64_t seed, int64_t first_chain,
                                   int64_t n_chains, const int32_t *start_states,
                                   int64_t n_steps, int32_t form, int64_t step_cap, int32_t *out,
                                   int64_t *bad_out)
{
    int rc = EK_OK;
    if (!h || !start_states || !out || !bad_out || n_chains < 1 || n_steps < 1 ||
        first_chain < 0 || n_chains > ((int64_t)1 << 31) || step_cap < 0 || form < 0 || form > 2 ||
        first_chain > ((int64_t)1 << 60) - n_chains || n_steps > ((int64_t)1 << 62) / n_chains)
        return ek_set_error(EK_EARG, "ek_kmc_trajectories: bad argument (1 <= n_chains <= 2^31, "
                                     "n_steps >= 1, chains below 2^60, form 0 .. 2, step_cap >= 0)");
    for (int64_t c = 0; c < n_chains; ++c)
        if (start_states[c] < 0 || start_states[c] >= h->n)
            return ek_set_error(EK_EARG, "ek_kmc_trajectories: start state %d of chain %lld is "
                                         "no state of %d", start_states[c], (long long)c, h->n);
    *bad_out = -1;
    for (int64_t c = 0; c < n_chains; ++c)
        out[c * n_steps] = start_states[c];
    kmc_ms[0] = kmc_ms[1] = kmc_ms[2] = 0.0;
    const int64_t draws = n_steps - 1;
    if (draws == 0)
        return EK_OK;
    if ((rc = kmc_set_device(h->device)) != EK_OK)
        return rc;
    const int64_t cap = step_cap > 0 ? step_cap : KMC_STEP_CAP;
    const bool wave = form == 2 || (form == 0 && n_chains <= KMC_WAVE_MAX_CHAINS);
    // the buffer [nc chains][mc steps]: all chains and as many steps as fit; once fewer
    // than KMC_MIN_CHUNK steps would fit, fewer chains
    const int64_t cells = KMC_BUF_BYTES / (int64_t)sizeof(int32_t);
    int64_t mc = cells / n_chains;
    if (mc < KMC_MIN_CHUNK)
        mc = KMC_MIN_CHUNK;
    if (mc > draws)
        mc = draws;
    int64_t nc = cells / mc;
    if (nc > n_chains)
        nc = n_chains;
    if ((rc = ek_mi_check_memory((size_t)(nc * mc + nc) * sizeof(int32_t) + 256,
                                 "ek_kmc_trajectories")) != EK_OK)
        return rc;
    KmcScope sc;
    sc.sync = h->s;
    int32_t *d_buf = nullptr, *d_cur = nullptr;
    uint32_t *d_bad = nullptr, bad = KMC_NO_BAD;
    float ms = 0.f;
    KMC_HIP(sc.events());
    KMC_HIP(sc.alloc(&d_buf, (size_t)(nc * mc) * sizeof(int32_t)));
    KMC_HIP(sc.alloc(&d_cur, (size_t)nc * sizeof(int32_t)));
    KMC_HIP(sc.alloc(&d_bad, sizeof(uint32_t)));
    KMC_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(uint32_t), h->s));
    for (int64_t c0 = 0; c0 < n_chains; c0 += nc) {
        const int64_t ncc = n_chains - c0 < nc ? n_chains - c0 : nc;
        KMC_HIP(hipEventRecord(sc.ev[0], h->s));
        KMC_HIP(hipMemcpyAsync(d_cur, start_states + c0, (size_t)ncc * sizeof(int32_t),
                               hipMemcpyHostToDevice, h->s));
        KMC_HIP(hipEventRecord(sc.ev[1], h->s));
        KMC_HIP(hipStreamSynchronize(h->s));
        KMC_HIP(hipEventElapsedTime(&ms, sc.ev[0], sc.ev[1]));
        kmc_ms[0] += ms;
        for (int64_t ts = 0; ts < draws; ts += mc) {
            const int64_t mcc = draws - ts < mc ? draws - ts : mc;
            KMC_HIP(hipEventRecord(sc.ev[1], h->s));
            for (int64_t l0 = 0; l0 < mcc; l0 += cap) {
                const int64_t lm = mcc - l0 < cap ? mcc - l0 : cap;
                if (wave)
                    hipLaunchKernelGGL(kmc_wave_kernel,
                                       dim3(kmc_blocks(ncc, KMC_WAVE_WG / EK_WAVE)),
                                       dim3(KMC_WAVE_WG), 0, h->s, kmc_rows(h), seed,
                                       first_chain + c0, ncc, d_cur, ts + l0, lm, d_buf, mc, l0,
                                       d_bad);
                else
                    hipLaunchKernelGGL(kmc_lane_kernel, dim3(kmc_blocks(ncc, KMC_LANE_WG)),
                                       dim3(KMC_LANE_WG), 0, h->s, kmc_rows(h), seed,
                                       first_chain + c0, ncc, d_cur, ts + l0, lm, d_buf, mc, l0,
                                       d_bad);
                KMC_HIP(hipGetLastError());
            }
            KMC_HIP(hipEventRecord(sc.ev[2], h->s));
            KMC_HIP(hipMemcpy2DAsync(out + c0 * n_steps + 1 + ts, (size_t)n_steps * sizeof(int32_t),
                                     d_buf, (size_t)mc * sizeof(int32_t),
                                     (size_t)mcc * sizeof(int32_t), (size_t)ncc,
                                     hipMemcpyDeviceToHost, h->s));
            KMC_HIP(hipEventRecord(sc.ev[3], h->s));
            KMC_HIP(hipStreamSynchronize(h->s));
            KMC_HIP(hipEventElapsedTime(&ms, sc.ev[1], sc.ev[2]));
            kmc_ms[1] += ms;
            KMC_HIP(hipEventElapsedTime(&ms, sc.ev[2], sc.ev[3]));
            kmc_ms[2] += ms;
        }
    }
    KMC_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, h->s));
    KMC_HIP(hipStreamSynchronize(h->s));
    *bad_out = kmc_bad(bad);
    return EK_OK;
}

// ---- ensemble ------------------------------------------------------------------------------
extern "C" int ek_kmc_ensemble(int device, int32_t n, const double *T, const int64_t *colptr,
                               const int32_t *rows, const double *vals, const double *p0,
                               int64_t n_steps, const double *observable, double *p_out,
                               double *out)
{
    int rc = EK_OK;
    const bool dense = T != nullptr;
    if (n < 1 || n_steps < 1 || !p0 || !p_out || !out || (dense == (colptr != nullptr)) ||
        n_steps > ((int64_t)1 << 40) / n)
        return ek_set_error(EK_EARG, "ek_kmc_ensemble: bad argument (n, n_steps >= 1, either T "
                                     "or colptr / rows / vals)");
    int64_t nnz = 0;
    if (!dense) {
        if (colptr[0] != 0)
            return ek_set_error(EK_EARG, "ek_kmc_ensemble: colptr[0] != 0");
        for (int32_t j = 0; j < n; ++j)
            if (colptr[j + 1] < colptr[j])
                return ek_set_error(EK_EARG, "ek_kmc_ensemble: colptr descends at column %d", j);
        nnz = colptr[n];
        if (nnz > 0 && (!rows || !vals))
            return ek_set_error(EK_EARG, "ek_kmc_ensemble: null argument");
        for (int64_t k = 0; k < nnz; ++k)
            if (rows[k] < 0 || rows[k] >= n)
                return ek_set_error(EK_EARG, "ek_kmc_ensemble: row %d of entry %lld is no state",
                                    rows[k], (long long)k);
    }
    if ((rc = kmc_set_device(device)) != EK_OK)
        return rc;
    const size_t nb = (size_t)n * sizeof(double);
    const int32_t blocks = (n + KMC_ENS_ROWS - 1) / KMC_ENS_ROWS;
    const size_t mat_b = dense ? (size_t)n * n * sizeof(double) + (size_t)blocks * nb
                               : (size_t)(n + 1) * sizeof(int64_t) + (size_t)nnz * 12;
    // every p stays on the device ([n_steps][n]), or two of them and the [n_steps] products
    const size_t keep_b = observable ? 3 * nb + (size_t)n_steps * sizeof(double)
                                     : (size_t)n_steps * nb;
    if ((rc = ek_mi_check_memory(mat_b + keep_b + 1024, "ek_kmc_ensemble")) != EK_OK)
        return rc;
    KmcScope sc;
    double *d_T = nullptr, *d_part = nullptr, *d_vals = nullptr, *d_p = nullptr, *d_o = nullptr,
           *d_obs = nullptr;
    int64_t *d_colptr = nullptr;
    int32_t *d_rows = nullptr;
    KMC_HIP(ek_stream_create_flags(&sc.own, hipStreamNonBlocking));
    hipStream_t s = sc.own;
    KMC_HIP(sc.events());
    if (dense) {
        KMC_HIP(sc.alloc(&d_T, (size_t)n * n * sizeof(double)));
        KMC_HIP(sc.alloc(&d_part, (size_t)blocks * nb));
    } else {
        KMC_HIP(sc.alloc(&d_colptr, (size_t)(n + 1) * sizeof(int64_t)));
        KMC_HIP(sc.alloc(&d_rows, (size_t)nnz * sizeof(int32_t)));
        KMC_HIP(sc.alloc(&d_vals, (size_t)nnz * sizeof(double)));
    }
    KMC_HIP(sc.alloc(&d_p, observable ? 2 * nb : (size_t)n_steps * nb));
    if (observable) {
        KMC_HIP(sc.alloc(&d_o, nb));
        KMC_HIP(sc.alloc(&d_obs, (size_t)n_steps * sizeof(double)));
    }
    KMC_HIP(hipEventRecord(sc.ev[0], s));
    if (dense) {
        KMC_HIP(hipMemcpyAsync(d_T, T, (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, s));
    } else {
        KMC_HIP(hipMemcpyAsync(d_colptr, colptr, (size_t)(n + 1) * sizeof(int64_t),
                               hipMemcpyHostToDevice, s));
        if (nnz > 0) {
            KMC_HIP(hipMemcpyAsync(d_rows, rows, (size_t)nnz * sizeof(int32_t),
                                   hipMemcpyHostToDevice, s));
            KMC_HIP(hipMemcpyAsync(d_vals, vals, (size_t)nnz * sizeof(double),
                                   hipMemcpyHostToDevice, s));
        }
    }
    KMC_HIP(hipMemcpyAsync(d_p, p0, nb, hipMemcpyHostToDevice, s));
    if (observable)
        KMC_HIP(hipMemcpyAsync(d_o, observable, nb, hipMemcpyHostToDevice, s));
    KMC_HIP(hipEventRecord(sc.ev[1], s));
    {
        const dim3 wg(KMC_WG), gcol(kmc_blocks(n, KMC_WG));
        double *p = d_p;
        for (int64_t t = 0; t < n_steps; ++t) {
            if (observable)
                hipLaunchKernelGGL(kmc_ens_dot_kernel, dim3(1), wg, 0, s, p, d_o, n, d_obs + t);
            if (t + 1 == n_steps)
                break;
            double *pn = observable ? (p == d_p ? d_p + n : d_p) : p + n;
            if (dense) {
                hipLaunchKernelGGL(kmc_ens_part_kernel, dim3(gcol.x, (unsigned)blocks), wg, 0, s,
                                   d_T, p, n, d_part);
                hipLaunchKernelGGL(kmc_ens_sum_kernel, gcol, wg, 0, s, d_part, blocks, n, pn);
            } else {
                hipLaunchKernelGGL(kmc_ens_csc_kernel, gcol, wg, 0, s, d_colptr, d_rows, d_vals,
                                   p, n, pn);
            }
            p = pn;
        }
        KMC_HIP(hipGetLastError());
        KMC_HIP(hipEventRecord(sc.ev[2], s));
        KMC_HIP(hipMemcpyAsync(p_out, p, nb, hipMemcpyDeviceToHost, s));
        if (observable)
            KMC_HIP(hipMemcpyAsync(out, d_obs, (size_t)n_steps * sizeof(double),
                                   hipMemcpyDeviceToHost, s));
        else
            KMC_HIP(hipMemcpyAsync(out, d_p, (size_t)n_steps * nb, hipMemcpyDeviceToHost, s));
    }
    KMC_HIP(hipEventRecord(sc.ev[3], s));
    KMC_HIP(hipStreamSynchronize(s));
    return kmc_store_ms(sc, kmc_ms);
}

// ---- photons -------------------------------------------------------------------------------
// the per-state distance tables: every state has a bin, the offsets ascend
static int kmc_check_dist(int32_t n_states, const int64_t *dist_off, const double *centres,
                          const double *dist_cdf, const char *who)
{
    if (n_states < 1 || !dist_off || !centres || !dist_cdf || dist_off[0] != 0)
        return ek_set_error(EK_EARG, "%s: null distance tables or dist_off[0] != 0", who);
    for (int32_t i = 0; i < n_states; ++i)
        if (dist_off[i + 1] <= dist_off[i])
            return ek_set_error(EK_EARG, "%s: state %d has no distance bin", who, i);
    return EK_OK;
}

static int kmc_upload_dist(KmcScope &sc, hipStream_t s, int32_t n_states, const int64_t *dist_off,
                           const double *centres, const double *dist_cdf, KmcDist *D)
{
    int64_t *d_off = nullptr;
    double *d_c = nullptr, *d_f = nullptr;
    const size_t ob = (size_t)(n_states + 1) * sizeof(int64_t),
                 bb = (size_t)dist_off[n_states] * sizeof(double);
    KMC_HIP(sc.alloc(&d_off, ob));
    KMC_HIP(sc.alloc(&d_c, bb));
    KMC_HIP(sc.alloc(&d_f, bb));
    KMC_HIP(hipMemcpyAsync(d_off, dist_off, ob, hipMemcpyHostToDevice, s));
    KMC_HIP(hipMemcpyAsync(d_c, centres, bb, hipMemcpyHostToDevice, s));
    KMC_HIP(hipMemcpyAsync(d_f, dist_cdf, bb, hipMemcpyHostToDevice, s));
    D->off = d_off;
    D->centres = d_c;
    D->cdf = d_f;
    return EK_OK;
}

extern "C" int ek_kmc_fret_probs(int device, uint64_t seed, int64_t chain, int64_t n,
                                 const int32_t *states, int32_t n_states, const int64_t *dist_off,
                                 const double *centres, const double *dist_cdf, double bin_width,
                                 double r06, double *E_out)
{
    int rc = EK_OK;
    if (n < 1 || n > ((int64_t)1 << 36) || !states || !E_out || chain < 0 ||
        chain >= ((int64_t)1 << 60))
        return ek_set_error(EK_EARG, "ek_kmc_fret_probs: bad argument (1 <= n <= 2^36, 0 <= "
                                     "chain < 2^60)");
    if ((rc = kmc_check_dist(n_states, dist_off, centres, dist_cdf, "ek_kmc_fret_probs")) != EK_OK)
        return rc;
    for (int64_t k = 0; k < n; ++k)
        if (states[k] < 0 || states[k] >= n_states)
            return ek_set_error(EK_EARG, "ek_kmc_fret_probs: state %d of photon %lld is no "
                                         "state of %d", states[k], (long long)k, n_states);
    if ((rc = kmc_set_device(device)) != EK_OK ||
        (rc = ek_mi_check_memory((size_t)n * 12 + (size_t)dist_off[n_states] * 16 +
                                 (size_t)n_states * 8 + 1024, "ek_kmc_fret_probs")) != EK_OK)
        return rc;
    KmcScope sc;
    KmcDist D;
    int32_t *d_s = nullptr;
    double *d_E = nullptr;
    KMC_HIP(ek_stream_create_flags(&sc.own, hipStreamNonBlocking));
    hipStream_t s = sc.own;
    KMC_HIP(sc.events());
    KMC_HIP(sc.alloc(&d_s, (size_t)n * sizeof(int32_t)));
    KMC_HIP(sc.alloc(&d_E, (size_t)n * sizeof(double)));
    KMC_HIP(hipEventRecord(sc.ev[0], s));
    if ((rc = kmc_upload_dist(sc, s, n_states, dist_off, centres, dist_cdf, &D)) != EK_OK)
        return rc;
    KMC_HIP(hipMemcpyAsync(d_s, states, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    KMC_HIP(hipEventRecord(sc.ev[1], s));
    hipLaunchKernelGGL(kmc_fret_probs_kernel, dim3(kmc_blocks(n, KMC_WG)), dim3(KMC_WG), 0, s, D,
                       n_states, seed, (uint64_t)chain, n, d_s, bin_width, r06, d_E);
    KMC_HIP(hipGetLastError());
    KMC_HIP(hipEventRecord(sc.ev[2], s));
    KMC_HIP(hipMemcpyAsync(E_out, d_E, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    KMC_HIP(hipEventRecord(sc.ev[3], s));
    KMC_HIP(hipStreamSynchronize(s));
    return kmc_store_ms(sc, kmc_ms);
}

// the histogram rule's host side (kmc_run_bursts)
struct KmcHistPlan {
    int32_t n_states;
    const int64_t *dist_off;
    const double *centres, *dist_cdf;
    double bw, r06;
    KmcDist D;
    size_t bytes(int64_t) const
    {
        return (size_t)(n_states + 1) * 8 + (size_t)dist_off[n_states] * 16;
    }
    int upload(KmcScope &sc, hipStream_t s, int64_t)
    {
        return kmc_upload_dist(sc, s, n_states, dist_off, centres, dist_cdf, &D);
    }
    KmcHistRule rule(uint64_t seed, uint8_t *d_flags, uint32_t *) const
    {
        return KmcHistRule{D, seed, bw, r06, d_flags};
    }
    int download(hipStream_t, int64_t) { return EK_OK; }
};

extern "C" int ek_kmc_fret_bursts(ek_kmc *h, uint64_t seed, int64_t first_burst,
                                  int64_t n_bursts, const int64_t *frame_off,
                                  const int64_t *frames, const double *pop_cdf,
                                  const int64_t *dist_off, const double *centres,
                                  const double *dist_cdf, double bin_width, double r06,
                                  int64_t step_cap, uint8_t *photons_out, int32_t *traj_out,
                                  int64_t *bad_out)
{
    int rc = EK_OK;
    if (!h)
        return ek_set_error(EK_EARG, "ek_kmc_fret_bursts: null argument");
    if ((rc = kmc_check_dist(h->n, dist_off, centres, dist_cdf, "ek_kmc_fret_bursts")) != EK_OK)
        return rc;
    KmcHistPlan plan{h->n, dist_off, centres, dist_cdf, bin_width, r06, KmcDist()};
    return kmc_run_bursts(h, "ek_kmc_fret_bursts", kmc_ms, seed, first_burst, n_bursts,
                          frame_off, frames, pop_cdf, step_cap, photons_out, traj_out, bad_out,
                          nullptr, plan);
}

extern "C" int ek_kmc_last_timing(double *ms_out)
{
    if (!ms_out)
        return ek_set_error(EK_EARG, "ek_kmc_last_timing: null argument");
    for (int i = 0; i < 3; ++i)
        ms_out[i] = kmc_ms[i];
    return EK_OK;
}
