// ek_msm_squeeze.h -- dropping the -1 frames of a set of trajectories on the device:
// the two-level compaction ek_msm.hip counts with, shared with ek_msm_boot.hip.
//
// The frames that are not -1 keep their order (reference
// enspara/msm/transition_matrices.py:156, before _transitions_helper pairs them):
// per-workgroup counts, one workgroup scans them, every workgroup places its
// survivors; cstart[t] = survivors before the first frame of trajectory t.  The same
// count / scan pair (MODE 1) compacts the cells of a count table that are not zero.
// Integer work only: every launch gives the same bytes.
#pragma once
#include "ek_common.h"

#include <algorithm>

static inline unsigned msm_blocks(int64_t n)
{
    return (unsigned)std::max<int64_t>(1, (n + EK_BLOCK - 1) / EK_BLOCK);
}

// ---- two-level compaction: count per workgroup, scan the counts, place ----------
#define MSM_WG 1024

// cnt[b] = elements of [1024 b, 1024 b + 1024) that survive
// (MODE 0: frames that are not -1; MODE 1: table cells that are not 0)
template <int MODE>
__global__ void __launch_bounds__(MSM_WG)
msm_count_kernel(const int32_t *__restrict__ a, int64_t n,
                 int32_t *__restrict__ cnt)
{
    const int64_t i = (int64_t)blockIdx.x * MSM_WG + threadIdx.x;
    const bool keep = i < n && (MODE == 0 ? a[i] != -1 : a[i] != 0);
    const int c = __syncthreads_count(keep);
    if (threadIdx.x == 0)
        cnt[blockIdx.x] = c;
}

// exclusive prefix sums of cnt[0 .. nb) by one workgroup -> off[0 .. nb], off[nb] = total
static __global__ void __launch_bounds__(MSM_WG)
msm_scan_kernel(const int32_t *__restrict__ cnt, int64_t nb,
                int64_t *__restrict__ off)
{
    __shared__ int64_t part[MSM_WG];
    __shared__ int64_t wsum[MSM_WG / EK_WAVE];
    const int t = threadIdx.x;
    const int64_t per = (nb + MSM_WG - 1) / MSM_WG;
    const int64_t lo = (int64_t)t * per, hi = (lo + per < nb) ? lo + per : nb;
    int64_t s = 0;
    // (a thread's counts are read in batches of sixteen loads in flight: one after the
    // other, each waiting for the one before, the 24 of a 5000-state table's scan were
    // 25 us of nothing but latency -- twice per call)
    constexpr int UB = 16;
    for (int64_t b0 = lo; b0 < hi; b0 += UB) {
        int32_t v[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u)
            v[u] = b0 + u < hi ? cnt[b0 + u] : 0;
#pragma unroll
        for (int u = 0; u < UB; ++u)
            s += v[u];
    }
    // scan of the 1024 partial sums: inside the waves, then over the 16 waves
    int64_t incl = s;
    const int lane = t & (EK_WAVE - 1), wv = t / EK_WAVE;
#pragma unroll
    for (int o = 1; o < EK_WAVE; o <<= 1) {
        const int64_t v = __shfl_up(incl, o, EK_WAVE);
        if (lane >= o)
            incl += v;
    }
    if (lane == EK_WAVE - 1)
        wsum[wv] = incl;
    __syncthreads();
    int64_t base = 0;
    for (int w = 0; w < wv; ++w)
        base += wsum[w];
    part[t] = base + incl - s;
    __syncthreads();
    int64_t run = part[t];
    for (int64_t b0 = lo; b0 < hi; b0 += UB) {
        int32_t v[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u)
            v[u] = b0 + u < hi ? cnt[b0 + u] : 0;
#pragma unroll
        for (int u = 0; u < UB; ++u)
            if (b0 + u < hi) {
                off[b0 + u] = run;
                run += v[u];
            }
    }
    if (t == MSM_WG - 1)
        off[nb] = base + incl;
}

// position of this thread's element among the survivors of its workgroup
__device__ __forceinline__ int msm_wg_rank(bool keep)
{
    __shared__ int wcnt[MSM_WG / EK_WAVE];
    const int lane = threadIdx.x & (EK_WAVE - 1), wv = threadIdx.x / EK_WAVE;
    const unsigned long long m = __ballot(keep);
    if (lane == 0)
        wcnt[wv] = __popcll(m);
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wv; ++w)
        before += wcnt[w];
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

// the frames that are not -1, in order (transition_matrices.py:156)
static __global__ void __launch_bounds__(MSM_WG)
msm_squeeze_kernel(const int32_t *__restrict__ a, int64_t n,
                   const int64_t *__restrict__ off, int32_t *__restrict__ c)
{
    const int64_t i = (int64_t)blockIdx.x * MSM_WG + threadIdx.x;
    const bool keep = i < n && a[i] != -1;
    const int r = msm_wg_rank(keep);
    if (keep)
        c[off[blockIdx.x] + r] = a[i];
}

// cstart[t] = survivors before the first frame of trajectory t; cstart[n_trj] = all
// (one wave per trajectory: what its workgroup of the squeeze placed before it)
static __global__ void __launch_bounds__(EK_BLOCK)
msm_cstart2_kernel(const int32_t *__restrict__ a, int64_t n,
                   const int64_t *__restrict__ start,
                   const int64_t *__restrict__ off, int64_t nb, int64_t n_trj,
                   int64_t *__restrict__ cstart)
{
    const int64_t t = (int64_t)blockIdx.x * (EK_BLOCK / EK_WAVE) +
                      threadIdx.x / EK_WAVE;
    const int lane = threadIdx.x & (EK_WAVE - 1);
    if (t > n_trj)
        return;
    if (t == n_trj || start[t] >= n) {
        if (lane == 0)
            cstart[t] = off[nb];
        return;
    }
    const int64_t b = start[t] / MSM_WG;
    int before = 0;
    for (int64_t i = b * MSM_WG + lane; i < start[t]; i += EK_WAVE)
        before += (a[i] != -1) ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        before += __shfl_xor(before, o, EK_WAVE);
    if (lane == 0)
        cstart[t] = off[b] + before;
}
