// ek_msm_mle.hip -- the reversible maximum-likelihood MSM builder: Prinz's
// fixed-point sweeps (Prinz et al., J. Chem. Phys. 134, 174105 (2011)) on the
// device, every sweep of a fit inside ONE launch.
//
// Replaces the iteration of the reference's builders.mle
// (enspara/msm/builders.py:215-318, the pure-Python loop its `mle` calls).
//
// A sweep is the diagonal pass (every state on its own) and then one update per
// off-diagonal pair (i, j), i < j, which the reference visits in lexicographic
// order.  An update reads and writes X[i,j] (= X[j,i]), X_rs[i] and X_rs[j] and
// nothing else, so any schedule that keeps the relative order of every two updates
// that share a state performs the same floating-point operations on the same
// operands: the result is the sequential sweep's bit for bit.  The host puts the
// pairs into LEVELS (enspara_amd/msm/builders.py, _mle_schedule): no two pairs of a
// level share a state, and every earlier pair that shares a state with a pair lies
// in a smaller level.  Here a level's pairs are spread over the lanes of a single
// workgroup and a workgroup barrier separates the levels; a dense sweep over n
// states is 2n - 3 barriers instead of n(n-1)/2 dependent updates.
//
// The work is a latency chain, not bandwidth: the pair data of a level is
// contiguous (level-major layout), the first MLE_WG pairs of the NEXT level are
// fetched before the current level is computed (a pair belongs to one level and
// one lane, so nothing the current level writes is read by that fetch), and the
// row sums X_rs, C_rs stay in LDS for the whole launch when 16 n bytes fit
// (MLE_LDS_ROWSUM_BYTES); beyond that they are read and written in global memory
// by the same code (EK_MSM_MLE_GLOBAL=1 forces that form at any n: tests).
//
// Arithmetic: the reference's expressions, operation by operation (the library is
// built with -ffp-contract=off: no fused multiply-add), IEEE sqrt and division.
// Only `logl`, which decides the stop, is summed in another order than the
// reference's -- lane partials, a butterfly over the wave, the waves in order --
// but in the SAME order on every run.
#include "ek_common.h"

#include <stdlib.h>

#include <algorithm>
#include <new>

extern int ek_set_error(int code, const char *fmt, ...);

#define MLE_HIP(call)                                                          \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define MLE_WG 1024
#define MLE_WAVES (MLE_WG / EK_WAVE)
// head of the dynamic LDS: the waves' partial sums of logl and the verdict
#define MLE_LDS_HEAD (MLE_WAVES + 2)
// X_rs and C_rs of n states are 16 n bytes: 9216 states in LDS (of the CU's 160 KiB)
#define MLE_LDS_ROWSUM_BYTES (144 * 1024)

struct MleOut {
    long long n_iter;       // sweeps that ran
    double logl;            // of the last one
};

// one off-diagonal update (builders.py:271-299); returns the pair's share of logl
__device__ __forceinline__ double mle_pair(int i, int j, double cij, double cji,
                                           double x, double *x_rs,
                                           const double *c_rs, double *x_out)
{
    const double cri = c_rs[i], crj = c_rs[j];
    double xri = x_rs[i], xrj = x_rs[j];
    const double s = cij + cji;
    const double a = (cri - cij) + (crj - cji);
    const double b = cri * (xrj - x) + crj * (xri - x) - s * (xri + xrj - 2.0 * x);
    const double c = -s * (xri - x) * (xrj - x);
    double v = x;
    if (a != 0.0)
        v = (-b + sqrt(b * b - 4.0 * a * c)) / (2.0 * a);
    xri = xri + (v - x);
    xrj = xrj + (v - x);
    x_rs[i] = xri;
    x_rs[j] = xrj;
    *x_out = v;
    if (v > 0.0) {
        const double lv = log(v);
        return (cij * lv / xri) + (cji * lv / xrj);
    }
    return 0.0;
}

template <bool LDS>
__global__ void __launch_bounds__(MLE_WG)
msm_mle_prinz_kernel(int32_t n, int32_t n_levels,
                     const int64_t *__restrict__ level_ptr,
                     const int32_t *__restrict__ pair_i,
                     const int32_t *__restrict__ pair_j,
                     const double *__restrict__ c_ij,
                     const double *__restrict__ c_ji,
                     const double *__restrict__ c_diag, const double *c_rs_g,
                     double *__restrict__ x_pairs, double *__restrict__ x_diag,
                     double *x_rs_g, double tol, long long max_iter,
                     MleOut *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double mle_lds[];
    double *red = mle_lds;                      // [MLE_WAVES] partials, [1] verdict
    double *x_rs = LDS ? mle_lds + MLE_LDS_HEAD : x_rs_g;
    double *c_rs_l = mle_lds + MLE_LDS_HEAD + n;
    const double *c_rs = LDS ? c_rs_l : c_rs_g;
    const int tid = threadIdx.x;
    const int lane = tid & (EK_WAVE - 1), wv = tid / EK_WAVE;

    if (LDS) {
        for (int i = tid; i < n; i += MLE_WG) {
            x_rs[i] = x_rs_g[i];
            c_rs_l[i] = c_rs_g[i];
        }
    }
    __syncthreads();

    double oldlogl = 0.0, logl = 0.0;
    long long it = 0;
    for (;;) {
        double acc = 0.0;
        // ---- the diagonal (builders.py:257-266): every state on its own
        for (int i = tid; i < n; i += MLE_WG) {
            const double cii = c_diag[i], xii = x_diag[i];
            const double den = c_rs[i] - cii;
            double rs = x_rs[i];
            double nx = xii;
            if (den > 0.0)
                nx = cii * (rs - xii) / den;
            rs = rs + (nx - xii);
            x_rs[i] = rs;
            x_diag[i] = nx;
            if (nx > 0.0)
                acc += cii * log(nx / rs);
        }
        __syncthreads();

        // ---- the levels, in order; lane t takes pairs lo + t, lo + t + MLE_WG, ..
        // of level [lo, hi); its first pair of the next level is already on its way
        int64_t lo = 0, hi = 0, nhi = 0, nnhi = 0;
        if (n_levels > 0) {
            lo = level_ptr[0];
            hi = level_ptr[1];
            nhi = level_ptr[n_levels > 1 ? 2 : 1];
            nnhi = level_ptr[n_levels > 2 ? 3 : (n_levels > 1 ? 2 : 1)];
        }
        int ci = 0, cj = 0;
        double ccij = 0.0, ccji = 0.0, cx = 0.0;
        if (lo + tid < hi) {
            const int64_t p = lo + tid;
            ci = pair_i[p];
            cj = pair_j[p];
            ccij = c_ij[p];
            ccji = c_ji[p];
            cx = x_pairs[p];
        }
        for (int L = 0; L < n_levels; ++L) {
            // (the end of the level after the next two: asked for two levels early)
            const int64_t far = level_ptr[L + 4 <= n_levels ? L + 4 : n_levels];
            int ni = 0, nj = 0;
            double ncij = 0.0, ncji = 0.0, nx = 0.0;
            const int64_t q = hi + tid;
            if (q < nhi) {
                ni = pair_i[q];
                nj = pair_j[q];
                ncij = c_ij[q];
                ncji = c_ji[q];
                nx = x_pairs[q];
            }
            int64_t p = lo + tid;
            if (p < hi) {
                double v;
                acc += mle_pair(ci, cj, ccij, ccji, cx, x_rs, c_rs, &v);
                x_pairs[p] = v;
                for (p += MLE_WG; p < hi; p += MLE_WG) {
                    acc += mle_pair(pair_i[p], pair_j[p], c_ij[p], c_ji[p], x_pairs[p],
                                    x_rs, c_rs, &v);
                    x_pairs[p] = v;
                }
            }
            __syncthreads();
            ci = ni;
            cj = nj;
            ccij = ncij;
            ccji = ncji;
            cx = nx;
            lo = hi;
            hi = nhi;
            nhi = nnhi;
            nnhi = far;
        }

        // ---- logl of the sweep, in a fixed order: butterfly over the wave, then
        // the waves in order
#pragma unroll
        for (int o = EK_WAVE / 2; o >= 1; o >>= 1)
            acc += __shfl_xor(acc, o, EK_WAVE);
        if (lane == 0)
            red[wv] = acc;
        __syncthreads();
        if (tid == 0) {
            double s = 0.0;
            for (int w = 0; w < MLE_WAVES; ++w)
                s += red[w];
            // builders.py:302-305: go on while |logl - oldlogl| > tol
            red[MLE_WAVES] = s;
            red[MLE_WAVES + 1] = (fabs(s - oldlogl) > tol) ? 1.0 : 0.0;
        }
        __syncthreads();
        logl = red[MLE_WAVES];
        const bool go_on = red[MLE_WAVES + 1] != 0.0;
        ++it;
        if (!go_on || it >= max_iter)
            break;
        oldlogl = logl;
        __syncthreads();        // (red is written again by the next sweep)
    }

    if (LDS) {
        for (int i = tid; i < n; i += MLE_WG)
            x_rs_g[i] = x_rs[i];
    }
    if (tid == 0) {
        out->n_iter = it;
        out->logl = logl;
    }
}

template <typename T>
static hipError_t mle_upload(T **dst, const T *src, int64_t count, hipStream_t s)
{
    hipError_t e = ek_dev_malloc((void **)dst, (size_t)std::max<int64_t>(count, 1) * sizeof(T));
    if (e == hipSuccess && count > 0)
        e = hipMemcpyAsync(*dst, src, (size_t)count * sizeof(T), hipMemcpyHostToDevice, s);
    return e;
}

extern "C" int ek_msm_mle_prinz(int device, int32_t n, int64_t n_pairs, int32_t n_levels,
                                const int64_t *level_ptr, const int32_t *pair_i,
                                const int32_t *pair_j, const double *c_ij,
                                const double *c_ji, const double *c_diag,
                                const double *c_rs, double *x_pairs, double *x_diag,
                                double *x_rs, double tol, int64_t max_iter,
                                int64_t *n_iter_out, double *logl_out)
{
    int rc = EK_OK;
    if (n < 1 || n_pairs < 0 || n_levels < 0 || !level_ptr || !c_diag || !c_rs ||
        !x_diag || !x_rs || max_iter < 1 || !n_iter_out || !logl_out ||
        (n_pairs > 0 && (!pair_i || !pair_j || !c_ij || !c_ji || !x_pairs)))
        return ek_set_error(EK_EARG, "ek_msm_mle_prinz: bad argument");
    // the schedule is what keeps the kernel's accesses inside its arrays and its
    // lanes off each other's states: check all of it here
    if (level_ptr[0] != 0 || level_ptr[n_levels] != n_pairs)
        return ek_set_error(EK_EARG, "ek_msm_mle_prinz: level_ptr does not span the "
                                     "%lld pairs", (long long)n_pairs);
    {
        int32_t *seen = new (std::nothrow) int32_t[(size_t)n];
        if (!seen)
            return ek_set_error(EK_ENOMEM, "ek_msm_mle_prinz: out of host memory");
        std::fill(seen, seen + n, -1);
        const char *what = nullptr;
        for (int32_t l = 0; l < n_levels && !what; ++l) {
            if (level_ptr[l + 1] < level_ptr[l] || level_ptr[l + 1] > n_pairs) {
                what = "level_ptr is not monotone";
                break;
            }
            for (int64_t p = level_ptr[l]; p < level_ptr[l + 1]; ++p) {
                const int32_t i = pair_i[p], j = pair_j[p];
                if (i < 0 || j <= i || j >= n) {
                    what = "a pair is not 0 <= i < j < n";
                    break;
                }
                if (seen[i] == l || seen[j] == l) {
                    what = "two pairs of a level share a state";
                    break;
                }
                seen[i] = l;
                seen[j] = l;
            }
        }
        delete[] seen;
        if (what)
            return ek_set_error(EK_EARG, "ek_msm_mle_prinz: %s", what);
    }

    const char *env = getenv("EK_MSM_MLE_GLOBAL");
    const bool in_lds = !(env && env[0] == '1') &&
                        (size_t)16 * (size_t)n <= (size_t)MLE_LDS_ROWSUM_BYTES;
    const size_t lds = (size_t)8 * (MLE_LDS_HEAD + (in_lds ? 2 * (size_t)n : 0));

    int64_t *d_lp = nullptr;
    int32_t *d_pi = nullptr, *d_pj = nullptr;
    double *d_cij = nullptr, *d_cji = nullptr, *d_cd = nullptr, *d_crs = nullptr;
    double *d_xp = nullptr, *d_xd = nullptr, *d_xrs = nullptr;
    MleOut *d_out = nullptr;
    MleOut h_out = {0, 0.0};
    hipStream_t s = nullptr;
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess)
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device,
                                hipGetErrorString(e0));
    }
    MLE_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    MLE_HIP(mle_upload(&d_lp, level_ptr, (int64_t)n_levels + 1, s));
    MLE_HIP(mle_upload(&d_pi, pair_i, n_pairs, s));
    MLE_HIP(mle_upload(&d_pj, pair_j, n_pairs, s));
    MLE_HIP(mle_upload(&d_cij, c_ij, n_pairs, s));
    MLE_HIP(mle_upload(&d_cji, c_ji, n_pairs, s));
    MLE_HIP(mle_upload(&d_cd, c_diag, (int64_t)n, s));
    MLE_HIP(mle_upload(&d_crs, c_rs, (int64_t)n, s));
    MLE_HIP(mle_upload(&d_xp, (const double *)x_pairs, n_pairs, s));
    MLE_HIP(mle_upload(&d_xd, (const double *)x_diag, (int64_t)n, s));
    MLE_HIP(mle_upload(&d_xrs, (const double *)x_rs, (int64_t)n, s));
    MLE_HIP(ek_dev_malloc((void **)&d_out, sizeof(MleOut)));
    if (in_lds) {
        if (lds > 48 * 1024)
            MLE_HIP(hipFuncSetAttribute((const void *)msm_mle_prinz_kernel<true>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds));
        hipLaunchKernelGGL(msm_mle_prinz_kernel<true>, dim3(1), dim3(MLE_WG), lds, s, n,
                           n_levels, d_lp, d_pi, d_pj, d_cij, d_cji, d_cd, d_crs, d_xp,
                           d_xd, d_xrs, tol, (long long)max_iter, d_out);
    } else {
        hipLaunchKernelGGL(msm_mle_prinz_kernel<false>, dim3(1), dim3(MLE_WG), lds, s, n,
                           n_levels, d_lp, d_pi, d_pj, d_cij, d_cji, d_cd, d_crs, d_xp,
                           d_xd, d_xrs, tol, (long long)max_iter, d_out);
    }
    MLE_HIP(hipGetLastError());
    if (n_pairs > 0)
        MLE_HIP(hipMemcpyAsync(x_pairs, d_xp, (size_t)n_pairs * sizeof(double),
                               hipMemcpyDeviceToHost, s));
    MLE_HIP(hipMemcpyAsync(x_diag, d_xd, (size_t)n * sizeof(double),
                           hipMemcpyDeviceToHost, s));
    MLE_HIP(hipMemcpyAsync(x_rs, d_xrs, (size_t)n * sizeof(double), hipMemcpyDeviceToHost,
                           s));
    MLE_HIP(hipMemcpyAsync(&h_out, d_out, sizeof(MleOut), hipMemcpyDeviceToHost, s));
    MLE_HIP(hipStreamSynchronize(s));
    *n_iter_out = (int64_t)h_out.n_iter;
    *logl_out = h_out.logl;
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_lp);
    (void)ek_dev_free(d_pi);
    (void)ek_dev_free(d_pj);
    (void)ek_dev_free(d_cij);
    (void)ek_dev_free(d_cji);
    (void)ek_dev_free(d_cd);
    (void)ek_dev_free(d_crs);
    (void)ek_dev_free(d_xp);
    (void)ek_dev_free(d_xd);
    (void)ek_dev_free(d_xrs);
    (void)ek_dev_free(d_out);
    if (s)
        (void)ek_stream_destroy(s);
    return rc;
}
