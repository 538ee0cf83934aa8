// ek_feat_assign.hip -- every sample against a table of K centers in feature
// space: the nearest center and the distance to it, resident on the device.
//
// Reference: the scan of enspara/cluster/util.py:186-203 around one of the
// libdist metrics --
//   assignments = zeros(n); distances = full(n, inf)
//   for i, center in enumerate(centers):
//       d = metric(X, center); closer = d < distances
//       distances[closer] = d[closer]; assignments[closer] = i
// -- which with only the metric on the device costs a launch, a read-back of n
// float64 and three numpy passes over n per center.  Here one launch does the
// whole scan: one lane owns one sample (the feature-major tiles of 256 samples
// the handle already holds), FA_TC centers at a time are staged in LDS in slices
// of FA_FC features and read as wave-wide broadcasts, the lane keeps FA_TC
// float64 sums in registers -- each one (sample, center) pair's FeatAcc chain
// over the features in order, finished by feat_finish: the arithmetic of
// feat_distance_kernel, bit for bit -- and carries its running (minimum, label)
// across the center tiles in ascending order, updating on strict <: NaN is never
// taken, the lowest index wins ties, a row with no distance below +inf keeps
// label 0.  A sample's feature is loaded once per FA_TC centers.
//
// Few samples and many centers would leave most of the device idle: the centers
// are then split into contiguous parts over gridDim.y, every part leaves its
// (minimum, label) per sample, and a second launch scans the parts in ascending
// order with the same strict < -- the first minimum of the first part that holds
// it, which is the first minimum overall.
#include "ek_feat.h"

#include <algorithm>

#define FA_TC 32      // centers per tile = float64 sums per lane
#define FA_FC 64      // features per staged slice: FA_FC * FA_TC * 8 B = 16 KiB of LDS
#define FA_FILL 1024  // workgroups wanted before the centers stay in one part

template <typename T, int METRIC>
__global__ void __launch_bounds__(EK_BLOCK)
feat_assign_kernel(const T *__restrict__ tiles, const T *__restrict__ C, int64_t n,
                   int F, int K, int kper, double *__restrict__ dist,
                   int32_t *__restrict__ assign, double *__restrict__ part_d,
                   int32_t *__restrict__ part_c)
{
    __shared__ T cs[FA_FC][FA_TC];
    const int64_t f = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    // (lanes past n read the zeros the last tile is padded with)
    const T *p = feat_tile_ptr(tiles, f, F);
    const int k0 = (int)blockIdx.y * kper;
    const int k1 = (K - k0 < kper) ? K : k0 + kper;
    double best = __builtin_inf();
    int32_t bc = 0;
    for (int c0 = k0; c0 < k1; c0 += FA_TC) {
        double acc[FA_TC];
#pragma unroll
        for (int c = 0; c < FA_TC; ++c)
            acc[c] = 0.0;
        for (int j0 = 0; j0 < F; j0 += FA_FC) {
            const int w = (F - j0 < FA_FC) ? (F - j0) : FA_FC;
            __syncthreads();
            for (int e = threadIdx.x; e < FA_TC * FA_FC; e += EK_BLOCK) {
                const int c = e / FA_FC, j = e % FA_FC;
                cs[j][c] = (c0 + c < k1 && j < w) ? C[(size_t)(c0 + c) * F + j0 + j] : (T)0;
            }
            __syncthreads();
#pragma unroll 2
            for (int j = 0; j < w; ++j) {
                const T x = p[(size_t)(j0 + j) * EK_TILE];
#pragma unroll
                for (int c = 0; c < FA_TC; ++c)
                    FeatAcc<T, METRIC>::add(acc[c], x, cs[j][c]);
            }
        }
#pragma unroll
        for (int c = 0; c < FA_TC; ++c) {
            const double a = feat_finish<METRIC>(acc[c], F);
            if (c0 + c < k1 && a < best) {      // util.py:201: strict <
                best = a;
                bc = c0 + c;
            }
        }
    }
    if (f >= n)
        return;
    if (gridDim.y == 1) {
        dist[f] = best;
        assign[f] = bc;
    } else {
        part_d[(size_t)blockIdx.y * n + f] = best;
        part_c[(size_t)blockIdx.y * n + f] = bc;
    }
}

// the parts' nearest in ascending order of their centers
__global__ void __launch_bounds__(EK_BLOCK)
feat_assign_merge_kernel(const double *__restrict__ part_d,
                         const int32_t *__restrict__ part_c, int parts, int64_t n,
                         double *__restrict__ dist, int32_t *__restrict__ assign)
{
    const int64_t f = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    if (f >= n)
        return;
    double best = __builtin_inf();
    int32_t bc = 0;
    for (int q = 0; q < parts; ++q) {
        const double a = part_d[(size_t)q * n + f];
        if (a < best) {
            best = a;
            bc = part_c[(size_t)q * n + f];
        }
    }
    dist[f] = best;
    assign[f] = bc;
}

extern "C" int ek_feat_assign_nearest(ek_feat *k, int32_t metric, const void *centers_host,
                                      int32_t n_centers)
{
    if (!k || metric < 0 || metric > 2 || n_centers < 0 || (!centers_host && n_centers > 0))
        return ek_set_error(EK_EARG, "ek_feat_assign_nearest: bad argument");
    if (!k->loaded)
        return ek_set_error(EK_ESTATE, "ek_feat_assign_nearest: no samples loaded");
    int rc = feat_metric_ok(k, metric, "ek_feat_assign_nearest");
    if (rc)
        return rc;
    FE_HIP(hipSetDevice(k->device));
    if ((rc = feat_shard_alloc(k, 0)))
        return rc;
    if (k->n == 0)
        return EK_OK;
    const int32_t K = n_centers;
    const size_t cb = (size_t)K * (size_t)k->F * k->esize;
    if (cb > k->acent_cap) {
        FE_HIP(hipStreamSynchronize(k->s));
        (void)ek_dev_free(k->acent);
        k->acent = nullptr;
        k->acent_cap = 0;
        FE_HIP(ek_dev_malloc(&k->acent, cb));
        k->acent_cap = cb;
    }
    if (cb)
        FE_HIP(hipMemcpyAsync(k->acent, centers_host, cb, hipMemcpyHostToDevice, k->s));
    // parts: whole center tiles each; one part once the samples alone fill the device
    const int64_t nb = (k->n + EK_BLOCK - 1) / EK_BLOCK;
    const int32_t ktiles = (K + FA_TC - 1) / FA_TC;
    int32_t parts = 1;
    if (nb < FA_FILL && ktiles > 1)
        parts = (int32_t)std::min<int64_t>(ktiles, (FA_FILL + nb - 1) / nb);
    const int32_t kper = std::max((ktiles + parts - 1) / parts, 1) * FA_TC;
    parts = std::max((K + kper - 1) / kper, 1);
    if (parts > 1 && (size_t)parts * (size_t)k->n > k->apart_cap) {
        FE_HIP(hipStreamSynchronize(k->s));
        (void)ek_dev_free(k->apart_d);
        (void)ek_dev_free(k->apart_c);
        k->apart_d = nullptr;
        k->apart_c = nullptr;
        k->apart_cap = 0;
        const size_t cap = (size_t)parts * (size_t)k->n;
        FE_HIP(ek_dev_malloc((void **)&k->apart_d, cap * sizeof(double)));
        FE_HIP(ek_dev_malloc((void **)&k->apart_c, cap * sizeof(int32_t)));
        k->apart_cap = cap;
    }
    feat_dispatch(k, metric, [&](auto t, auto m) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((feat_assign_kernel<T, decltype(m)::value>),
                           dim3((unsigned)nb, parts), dim3(EK_BLOCK), 0, k->s,
                           (const T *)k->tiles, (const T *)k->acent, k->n, k->F, K, kper,
                           k->kdist, k->kassign, k->apart_d, k->apart_c);
    });
    FE_HIP(hipGetLastError());
    if (parts > 1) {
        hipLaunchKernelGGL(feat_assign_merge_kernel, dim3((unsigned)nb), dim3(EK_BLOCK), 0,
                           k->s, k->apart_d, k->apart_c, (int)parts, k->n, k->kdist,
                           k->kassign);
        FE_HIP(hipGetLastError());
    }
    // (centers_host is the caller's again on return)
    FE_HIP(hipStreamSynchronize(k->s));
    return EK_OK;
}
