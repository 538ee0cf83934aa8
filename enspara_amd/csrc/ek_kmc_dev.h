// ek_kmc_dev.h -- what the samplers share on the device: the Philox doubles, the compressed
// rows and the search of a row's cdf (ek_kmc.hip, ek_dye_pair.hip, ek_dye_bursts.hip; DESIGN.md
// 4k, 4m, 4n).
//
// Uniforms.  Philox4x32-10, key = the 64-bit seed (low word first), counter = {i lo, i hi,
//   chain lo, stream << 28 | chain hi} with i = index >> 1: one call serves the indices
//   2 i and 2 i + 1.  The stream field has 4 bits, the chain 60.
#pragma once
#include "ek_common.h"

// ek_kmc.hip: chains and bursts
#define KMC_TRANS 0u
#define KMC_INIT 1u
#define KMC_BIN 2u
#define KMC_JITTER 3u
#define KMC_COIN 4u
// ek_dye_pair.hip: an excitation of a donor-acceptor pair of dye MSMs
#define KMC_DECAY 5u            // index = the step
#define KMC_DONOR 6u            // index 0: the initial state, t + 1: the hop of step t
#define KMC_ACCEPTOR 7u
#define KMC_FRET_COIN 8u        // index 0: the coin of the static and isotropic treatments
// ek_dye_bursts.hip: the photons of a burst with explicit dyes (index = the photon within its
// burst; the coin of the kappa-squared rule is KMC_COIN).  12 .. 15 are free.
#define KMC_EVENT 9u            // the entry of the state's photon events
#define KMC_DCONF 10u           // the donor's conformation
#define KMC_ACONF 11u           // the acceptor's

struct KmcRows {
    const int64_t *indptr;
    const int32_t *cols;
    const double *cdf;
    int32_t n;
};

// ---- uniforms ----------------------------------------------------------------------------
__device__ __forceinline__ void kmc_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                           uint32_t k0, uint32_t k1, uint32_t w[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0;
    w[1] = c1;
    w[2] = c2;
    w[3] = c3;
}

__device__ __forceinline__ double kmc_double(uint32_t a, uint32_t b)
{
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

// the two doubles of call i of (stream, chain): indices 2 i and 2 i + 1
__device__ __forceinline__ void kmc_pair(uint64_t seed, uint32_t stream, uint64_t chain,
                                         uint64_t i, double &u0, double &u1)
{
    uint32_t w[4];
    kmc_philox((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)chain,
               (stream << 28) | (uint32_t)(chain >> 32), (uint32_t)seed, (uint32_t)(seed >> 32),
               w);
    u0 = kmc_double(w[0], w[1]);
    u1 = kmc_double(w[2], w[3]);
}

__device__ __forceinline__ double kmc_uniform(uint64_t seed, uint32_t stream, uint64_t chain,
                                              uint64_t index)
{
    double u0, u1;
    kmc_pair(seed, stream, chain, index >> 1, u0, u1);
    return (index & 1) ? u1 : u0;
}

// ---- the search ----------------------------------------------------------------------------
// the first k of [lo, hi) with cdf[k] > u; hi - 1 if there is none (hi > lo)
__device__ __forceinline__ int64_t kmc_upper(const double *__restrict__ cdf, int64_t lo,
                                             int64_t hi, double u)
{
    int64_t a = lo, b = hi - 1;
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (cdf[m] > u)
            b = m;
        else
            a = m + 1;
    }
    return a;
}

__device__ __forceinline__ int32_t kmc_step_lane(const KmcRows &R, int32_t s, double u,
                                                 uint32_t *bad)
{
    const int64_t lo = R.indptr[s], hi = R.indptr[s + 1];
    if (hi <= lo) {
        atomicMin(bad, (uint32_t)s);
        return s;
    }
    return R.cols[kmc_upper(R.cdf, lo, hi, u)];
}
