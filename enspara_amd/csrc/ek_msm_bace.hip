// ek_msm_bace.hip -- BACE coarse-graining of a count matrix (Bowman, J. Chem.
// Phys. 137, 134111 (2012)): the Bayes factors of the prune step and the whole
// merge loop on the device.
//
// Replaces the arithmetic of the reference's enspara/msm/bace.py: multiDistHelper
// (:235-252, one float64 reduction with two logarithms per term for every pair),
// mergeTwoClosestStates (:122-161) and the dense arg-max of calcDMat (:207-211).
// The bookkeeping of labels stays on the host (enspara_amd/msm/bace.py): it is
// O(n) per merge and is rebuilt from the merge records this file returns.
//
// A step is four launches on one stream, none of which the host waits for:
//   merge    rows / columns minX, minY of c and dMat (one thread per state)
//   pair     one workgroup per state d; those with d != minX and c[minX, d] > 1
//            recompute dMat[minX, d], the others leave at once (this IS the
//            compaction of row minX: a list would be written and read once)
//   argmax1  per-workgroup (value, flat index) maxima of dMat
//   argmax2  their maximum -> the step's record and the next merge's operands
// The kernel boundary is what carries c, dMat and the record from one launch to
// the next; nothing crosses workgroups inside a launch.  A step that finds no
// pair left (the largest entry of dMat is 0) sets `stop`, and every later launch
// returns at its first instruction.
//
// Types are the reference's: c, w and every sum float64 (no fused multiply-add:
// -ffp-contract=off), the sum rounded to float32, inverted in float32 into dMat,
// and the reported factor 1 / dMat[minX, minY] in float32 again.  The sum's order
// is the device's own (lane partials in steps of BACE_WG, a butterfly over the
// wave, the waves in order) and the same on every run; the reference's is a BLAS
// dot of unspecified order.  Arg-max: largest value, first row-major index on
// ties, NaN before everything (numpy's argmax).
#include "ek_common.h"

#include <new>

extern int ek_set_error(int code, const char *fmt, ...);

#define BACE_HIP(call)                                                         \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define BACE_WG 256
#define BACE_WAVES (BACE_WG / EK_WAVE)
#define BACE_MAX_N 16384            // c is 8 n^2 bytes: 2 GiB here; n^2 fits 32 bits
#define BACE_ARGMAX_BLOCKS 1024     // at most; 16 entries per thread below that
#define BACE_ARGMAX_PER_THREAD 16

// one step's record (enspara_amd/msm/bace.py reads it as a structured array)
struct BaceRec {
    int32_t x, y;       // minX, minY
    float bf;           // 1 / dMat[minX, minY]
    int32_t status;     // 0 a pair, 1 no pair left (dMat's maximum is 0), 2 not run
};
static_assert(sizeof(BaceRec) == 16, "BaceRec layout");

// the operands of the next merge; written by argmax2 only
struct BaceCur {
    int32_t x, y;
    int32_t ux, uy;     // unmerged[x], unmerged[y] as the merge finds them
    int32_t stop;
    int32_t pad[3];
};

struct BaceMax {
    float val;
    uint32_t idx;
};

// numpy's argmax order: NaN first, then the larger value, then the smaller index
__device__ __forceinline__ bool bace_better(float v, uint32_t i, float bv, uint32_t bi)
{
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn)
        return vn;
    if (vn)
        return i < bi;
    return (v > bv) || (v == bv && i < bi);
}

// sum over the workgroup in a fixed order, the result in every thread
__device__ __forceinline__ double bace_block_sum(double v, double *red)
{
#pragma unroll
    for (int o = EK_WAVE / 2; o >= 1; o >>= 1)
        v += __shfl_xor(v, o, EK_WAVE);
    if ((threadIdx.x & (EK_WAVE - 1)) == 0)
        red[threadIdx.x / EK_WAVE] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < BACE_WAVES; ++w)
        s += red[w];
    __syncthreads();
    return s;
}

// one state's terms of a pair's sum (bace.py:248-251): p = c / w, cp = the pooled
// distribution, a1 += c1 log(p1 / cp), a2 += c2 log(p2 / cp)
__device__ __forceinline__ void bace_term(double c1, double c2, double p1, double w2,
                                          double wsum, double &a1, double &a2)
{
    const double p2 = c2 / w2;
    const double cp = (c1 + c2) / wsum;
    a1 += c1 * log(p1 / cp);
    a2 += c2 * log(p2 / cp);
}

// ---- prune: every state against the pseudo-state (bace.py:341-369) -----------
// c1 = pseud (float32(1) / float32(n), promoted), w1 = 1; c2 = c[s, :] + 1 / n
__global__ void __launch_bounds__(BACE_WG)
bace_prune_kernel(int32_t n, const double *__restrict__ c, const double *__restrict__ w,
                  double pseud, double pc, float *__restrict__ d_out)
{
    __shared__ double red[BACE_WAVES];
    const int s = blockIdx.x;
    const double w2 = w[s], wsum = 1.0 + w2;
    const double p1 = pseud / 1.0;
    const double *row = c + (size_t)s * n;
    double a1 = 0.0, a2 = 0.0;
    for (int k = threadIdx.x; k < n; k += BACE_WG)
        bace_term(pseud, row[k] + pc, p1, w2, wsum, a1, a2);
    const double s1 = bace_block_sum(a1, red);
    const double s2 = bace_block_sum(a2, red);
    if (threadIdx.x == 0)
        d_out[s] = (float)(s1 + s2);
}

// ---- the pair kernel -------------------------------------------------------------
// ROW = false: workgroup b takes pair list[b] (the initial matrix: d > s, c[s, d] > 1)
// ROW = true:  workgroup d takes (minX, d) if d != minX and c[minX, d] > 1
template <bool ROW>
__global__ void __launch_bounds__(BACE_WG)
bace_pair_kernel(int32_t n, const double *__restrict__ c, const double *__restrict__ w,
                 const int32_t *__restrict__ unmerged, const int32_t *__restrict__ kept,
                 const int2 *__restrict__ list, const BaceCur *__restrict__ cur,
                 double pc, float *__restrict__ dmat)
{
    __shared__ double red[BACE_WAVES];
    int s, d;
    // (the same for the whole workgroup: all of it leaves or none)
    if (ROW) {
        if (cur->stop)
            return;
        s = cur->x;
        d = blockIdx.x;
        if (d == s || !(c[(size_t)s * n + d] > 1.0))
            return;
    } else {
        s = list[blockIdx.x].x;
        d = list[blockIdx.x].y;
    }
    const double w1 = w[s], w2 = w[d], wsum = w1 + w2;
    const bool us = unmerged[s] != 0, ud = unmerged[d] != 0;
    const double *r1 = c + (size_t)s * n, *r2 = c + (size_t)d * n;
    double a1 = 0.0, a2 = 0.0;
    for (int k = threadIdx.x; k < n; k += BACE_WG) {
        if (!kept[k])
            continue;
        const bool uk = unmerged[k] != 0;
        // bace.py:226, :245: the pseudo-count of two states nothing was merged into
        const double c1 = r1[k] + ((us && uk) ? pc : 0.0);
        const double c2 = r2[k] + ((ud && uk) ? pc : 0.0);
        bace_term(c1, c2, c1 / w1, w2, wsum, a1, a2);
    }
    const double s1 = bace_block_sum(a1, red);
    const double s2 = bace_block_sum(a2, red);
    if (threadIdx.x == 0) {
        const float df = (float)(s1 + s2);
        dmat[(size_t)s * n + d] = 1.0f / df;
    }
}

// ---- the merge (bace.py:128-153), thread k: column k of rows X, Y and row k of
// columns X, Y; thread X also the four entries where they cross, w and the flags.
// In the reference's order: a still-unmerged X gets its pseudo-counts written into
// row X (unmerged[X] still set: c[X, X] too), its flag is cleared, then column X
// (c[X, X] not again); the same for Y, which by then sees unmerged[X] == 0; row X
// += row Y; column X += column Y (of the rows just updated: c[X, X] receives
// c[X, Y] + c[Y, Y] as well); row and column Y = 0.
__global__ void __launch_bounds__(BACE_WG)
bace_merge_kernel(int32_t n, double *__restrict__ c, double *__restrict__ w,
                  int32_t *__restrict__ unmerged, int32_t *__restrict__ kept,
                  const BaceCur *__restrict__ cur, double pc, float *__restrict__ dmat)
{
    if (cur->stop)
        return;
    const int k = blockIdx.x * BACE_WG + threadIdx.x;
    if (k >= n)
        return;
    const int X = cur->x, Y = cur->y;
    const bool uX = cur->ux != 0, uY = cur->uy != 0;
    const size_t rX = (size_t)X * n, rY = (size_t)Y * n, rk = (size_t)k * n;
    dmat[rX + k] = 0.0f;
    dmat[rY + k] = 0.0f;
    dmat[rk + X] = 0.0f;
    dmat[rk + Y] = 0.0f;
    if (k == X) {
        const double xx = c[rX + X] + (uX ? pc : 0.0);
        const double xy = c[rX + Y] + ((uX && uY) ? pc : 0.0);
        const double yx = c[rY + X] + ((uX && uY) ? pc : 0.0);
        const double yy = c[rY + Y] + (uY ? pc : 0.0);
        c[rX + X] = (xx + yx) + (xy + yy);
        c[rX + Y] = 0.0;
        c[rY + X] = 0.0;
        c[rY + Y] = 0.0;
        w[X] = w[X] + w[Y];
        w[Y] = 0.0;
        unmerged[X] = 0;
        unmerged[Y] = 0;
        kept[Y] = 0;
    } else if (k != Y && kept[k]) {
        const bool uk = unmerged[k] != 0;
        const double a = c[rX + k] + ((uX && uk) ? pc : 0.0);
        const double b = c[rY + k] + ((uY && uk) ? pc : 0.0);
        c[rX + k] = a + b;
        c[rY + k] = 0.0;
        const double a2 = c[rk + X] + ((uX && uk) ? pc : 0.0);
        const double b2 = c[rk + Y] + ((uY && uk) ? pc : 0.0);
        c[rk + X] = a2 + b2;
        c[rk + Y] = 0.0;
    }
}

// ---- arg-max of dMat, two stages ---------------------------------------------------
__device__ __forceinline__ void bace_block_argmax(float &v, uint32_t &i, BaceMax *red)
{
#pragma unroll
    for (int o = EK_WAVE / 2; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(v, o, EK_WAVE);
        const uint32_t oi = (uint32_t)__shfl_xor((int)i, o, EK_WAVE);
        if (bace_better(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
    if ((threadIdx.x & (EK_WAVE - 1)) == 0) {
        red[threadIdx.x / EK_WAVE].val = v;
        red[threadIdx.x / EK_WAVE].idx = i;
    }
    __syncthreads();
    v = red[0].val;
    i = red[0].idx;
#pragma unroll
    for (int w = 1; w < BACE_WAVES; ++w)
        if (bace_better(red[w].val, red[w].idx, v, i)) {
            v = red[w].val;
            i = red[w].idx;
        }
}

__global__ void __launch_bounds__(BACE_WG)
bace_argmax1_kernel(const float *__restrict__ dmat, uint32_t total,
                    const BaceCur *__restrict__ cur, BaceMax *__restrict__ part)
{
    __shared__ BaceMax red[BACE_WAVES];
    if (cur->stop)
        return;
    // (an index no entry has: every entry, -inf included, is better)
    float v = -INFINITY;
    uint32_t idx = 0xffffffffu;
    const uint32_t gid = blockIdx.x * BACE_WG + threadIdx.x;
    const uint32_t stride = gridDim.x * BACE_WG;
    const uint32_t total4 = total / 4;
    const float4 *d4 = (const float4 *)dmat;
    for (uint32_t q = gid; q < total4; q += stride) {
        const float4 f = d4[q];
        const float e[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (bace_better(e[j], 4 * q + j, v, idx)) {
                v = e[j];
                idx = 4 * q + j;
            }
    }
    for (uint32_t t = 4 * total4 + gid; t < total; t += stride)
        if (bace_better(dmat[t], t, v, idx)) {
            v = dmat[t];
            idx = t;
        }
    bace_block_argmax(v, idx, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x].val = v;
        part[blockIdx.x].idx = idx;
    }
}

__global__ void __launch_bounds__(BACE_WG)
bace_argmax2_kernel(int32_t n, const BaceMax *__restrict__ part, int32_t n_part,
                    const int32_t *__restrict__ unmerged, BaceCur *__restrict__ cur,
                    BaceRec *__restrict__ rec)
{
    __shared__ BaceMax red[BACE_WAVES];
    if (cur->stop) {
        if (threadIdx.x == 0) {
            rec->x = -1;
            rec->y = -1;
            rec->bf = 0.0f;
            rec->status = 2;
        }
        return;
    }
    float v = -INFINITY;
    uint32_t idx = 0xffffffffu;
    for (int b = threadIdx.x; b < n_part; b += BACE_WG)
        if (bace_better(part[b].val, part[b].idx, v, idx)) {
            v = part[b].val;
            idx = part[b].idx;
        }
    bace_block_argmax(v, idx, red);
    if (threadIdx.x == 0) {
        const int32_t x = (int32_t)(idx / (uint32_t)n), y = (int32_t)(idx % (uint32_t)n);
        const bool none = (v == 0.0f);      // only a pair that was computed is not 0
        rec->x = x;
        rec->y = y;
        rec->bf = 1.0f / v;                 // bace.py:211
        rec->status = none ? 1 : 0;
        cur->x = x;
        cur->y = y;
        cur->ux = unmerged[x];
        cur->uy = unmerged[y];
        if (none)
            cur->stop = 1;
    }
}

static int bace_argmax_blocks(size_t total)
{
    const size_t per = (size_t)BACE_WG * BACE_ARGMAX_PER_THREAD;
    size_t b = (total + per - 1) / per;
    if (b < 1)
        b = 1;
    if (b > BACE_ARGMAX_BLOCKS)
        b = BACE_ARGMAX_BLOCKS;
    return (int)b;
}

static bool bace_counts_ok(const double *c, size_t count)
{
    for (size_t i = 0; i < count; ++i)
        if (!(c[i] >= 0.0) || c[i] > 1.7976931348623157e308)
            return false;
    return true;
}

extern "C" int ek_msm_bace_prune(int device, int32_t n, const double *c, const double *w,
                                 float *d_out)
{
    int rc = EK_OK;
    if (n < 1 || n > BACE_MAX_N || !c || !w || !d_out)
        return ek_set_error(EK_EARG, "ek_msm_bace_prune: bad argument (1 <= n <= %d)",
                            BACE_MAX_N);
    const size_t nn = (size_t)n * (size_t)n;
    double *d_c = nullptr, *d_w = nullptr;
    float *d_d = nullptr;
    hipStream_t s = nullptr;
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess)
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device,
                                hipGetErrorString(e0));
    }
    BACE_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    BACE_HIP(ek_dev_malloc((void **)&d_c, nn * sizeof(double)));
    BACE_HIP(ek_dev_malloc((void **)&d_w, (size_t)n * sizeof(double)));
    BACE_HIP(ek_dev_malloc((void **)&d_d, (size_t)n * sizeof(float)));
    BACE_HIP(hipMemcpyAsync(d_c, c, nn * sizeof(double), hipMemcpyHostToDevice, s));
    BACE_HIP(hipMemcpyAsync(d_w, w, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
    {
        // bace.py:345-346: the pseudo-state is built in float32
        const float pseud = 1.0f / (float)n;
        hipLaunchKernelGGL(bace_prune_kernel, dim3(n), dim3(BACE_WG), 0, s, n, d_c, d_w,
                           (double)pseud, 1.0 / (double)n, d_d);
    }
    BACE_HIP(hipGetLastError());
    BACE_HIP(hipMemcpyAsync(d_out, d_d, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    BACE_HIP(hipStreamSynchronize(s));
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_c);
    (void)ek_dev_free(d_w);
    (void)ek_dev_free(d_d);
    if (s)
        (void)ek_stream_destroy(s);
    return rc;
}

extern "C" int ek_msm_bace_run(int device, int32_t n, const double *c, const double *w,
                               const int32_t *kept, int32_t n_kept, int32_t n_macrostates,
                               int32_t n_merges, void *records_out, int32_t dmat_steps,
                               float *dmat_out)
{
    int rc = EK_OK;
    if (n < 2 || n > BACE_MAX_N || !c || !w || !kept || n_kept < 1 || n_kept > n ||
        n_macrostates < 1 || n_merges < 0 || !records_out || dmat_steps < 0 ||
        (dmat_steps > 0 && !dmat_out) || dmat_steps > n_merges + 1)
        return ek_set_error(EK_EARG, "ek_msm_bace_run: bad argument (2 <= n <= %d)",
                            BACE_MAX_N);
    if (n_merges != (n_kept > n_macrostates ? n_kept - n_macrostates : 0))
        return ek_set_error(EK_EARG, "ek_msm_bace_run: %d merges do not take %d states to "
                                     "%d macrostates", n_merges, n_kept, n_macrostates);
    for (int32_t i = 0; i < n_kept; ++i)
        if (kept[i] < 0 || kept[i] >= n || (i > 0 && kept[i] <= kept[i - 1]))
            return ek_set_error(EK_EARG, "ek_msm_bace_run: the kept states are not "
                                         "increasing indices below n");
    const size_t nn = (size_t)n * (size_t)n;
    if (!bace_counts_ok(c, nn) || !bace_counts_ok(w, (size_t)n))
        return ek_set_error(EK_EARG, "ek_msm_bace_run: counts are finite and not negative");

    // the kept mask, and the initial work list (bace.py:19-42 without an update state):
    // s kept, d > s, c[s, d] > 1
    int32_t *h_mask = new (std::nothrow) int32_t[(size_t)n]();
    size_t n_list = 0;
    int2 *h_list = nullptr;
    if (h_mask) {
        for (int32_t i = 0; i < n_kept; ++i) {
            h_mask[kept[i]] = 1;
            const double *row = c + (size_t)kept[i] * n;
            for (int32_t d = kept[i] + 1; d < n; ++d)
                n_list += row[d] > 1.0;
        }
        h_list = new (std::nothrow) int2[n_list ? n_list : 1];
    }
    if (!h_mask || !h_list) {
        delete[] h_mask;
        delete[] h_list;
        return ek_set_error(EK_ENOMEM, "ek_msm_bace_run: out of host memory");
    }
    {
        size_t p = 0;
        for (int32_t i = 0; i < n_kept; ++i) {
            const double *row = c + (size_t)kept[i] * n;
            for (int32_t d = kept[i] + 1; d < n; ++d)
                if (row[d] > 1.0)
                    h_list[p++] = make_int2(kept[i], d);
        }
    }

    const double pc = 1.0 / (double)n;      // bace.py:129: unmerged / c.shape[0]
    const int nb_max = bace_argmax_blocks(nn);
    const int n_rec = n_merges + 1;
    const int nb_state = (n + BACE_WG - 1) / BACE_WG;
    double *d_c = nullptr, *d_w = nullptr;
    float *d_dmat = nullptr;
    int32_t *d_um = nullptr, *d_kept = nullptr;
    int2 *d_list = nullptr;
    BaceMax *d_part = nullptr;
    BaceRec *d_rec = nullptr;
    BaceCur *d_cur = nullptr;
    hipStream_t s = nullptr;
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess) {
            delete[] h_mask;
            delete[] h_list;
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device,
                                hipGetErrorString(e0));
        }
    }
    BACE_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    BACE_HIP(ek_dev_malloc((void **)&d_c, nn * sizeof(double)));
    BACE_HIP(ek_dev_malloc((void **)&d_dmat, nn * sizeof(float)));
    BACE_HIP(ek_dev_malloc((void **)&d_w, (size_t)n * sizeof(double)));
    BACE_HIP(ek_dev_malloc((void **)&d_um, (size_t)n * sizeof(int32_t)));
    BACE_HIP(ek_dev_malloc((void **)&d_kept, (size_t)n * sizeof(int32_t)));
    BACE_HIP(ek_dev_malloc((void **)&d_list, (n_list ? n_list : 1) * sizeof(int2)));
    BACE_HIP(ek_dev_malloc((void **)&d_part, (size_t)nb_max * sizeof(BaceMax)));
    BACE_HIP(ek_dev_malloc((void **)&d_rec, (size_t)n_rec * sizeof(BaceRec)));
    BACE_HIP(ek_dev_malloc((void **)&d_cur, sizeof(BaceCur)));
    BACE_HIP(hipMemcpyAsync(d_c, c, nn * sizeof(double), hipMemcpyHostToDevice, s));
    BACE_HIP(hipMemcpyAsync(d_w, w, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
    // (bace.py:88-89: unmerged starts as the kept mask)
    BACE_HIP(hipMemcpyAsync(d_um, h_mask, (size_t)n * sizeof(int32_t),
                            hipMemcpyHostToDevice, s));
    BACE_HIP(hipMemcpyAsync(d_kept, h_mask, (size_t)n * sizeof(int32_t),
                            hipMemcpyHostToDevice, s));
    if (n_list)
        BACE_HIP(hipMemcpyAsync(d_list, h_list, n_list * sizeof(int2),
                                hipMemcpyHostToDevice, s));
    BACE_HIP(hipMemsetAsync(d_dmat, 0, nn * sizeof(float), s));
    BACE_HIP(hipMemsetAsync(d_cur, 0, sizeof(BaceCur), s));
    BACE_HIP(hipMemsetAsync(d_rec, 0, (size_t)n_rec * sizeof(BaceRec), s));

    for (int step = 0; step < n_rec; ++step) {
        if (step == 0) {
            if (n_list)
                hipLaunchKernelGGL(bace_pair_kernel<false>, dim3((unsigned)n_list),
                                   dim3(BACE_WG), 0, s, n, d_c, d_w, d_um, d_kept, d_list,
                                   d_cur, pc, d_dmat);
        } else {
            hipLaunchKernelGGL(bace_merge_kernel, dim3(nb_state), dim3(BACE_WG), 0, s, n,
                               d_c, d_w, d_um, d_kept, d_cur, pc, d_dmat);
            hipLaunchKernelGGL(bace_pair_kernel<true>, dim3(n), dim3(BACE_WG), 0, s, n, d_c,
                               d_w, d_um, d_kept, d_list, d_cur, pc, d_dmat);
        }
        hipLaunchKernelGGL(bace_argmax1_kernel, dim3(nb_max), dim3(BACE_WG), 0, s, d_dmat,
                           (uint32_t)nn, d_cur, d_part);
        hipLaunchKernelGGL(bace_argmax2_kernel, dim3(1), dim3(BACE_WG), 0, s, n, d_part,
                           nb_max, d_um, d_cur, d_rec + step);
        // (tests only: dMat as this step leaves it)
        if (step < dmat_steps)
            BACE_HIP(hipMemcpyAsync(dmat_out + (size_t)step * nn, d_dmat, nn * sizeof(float),
                                    hipMemcpyDeviceToHost, s));
    }
    BACE_HIP(hipGetLastError());
    BACE_HIP(hipMemcpyAsync(records_out, d_rec, (size_t)n_rec * sizeof(BaceRec),
                            hipMemcpyDeviceToHost, s));
    BACE_HIP(hipStreamSynchronize(s));
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_c);
    (void)ek_dev_free(d_dmat);
    (void)ek_dev_free(d_w);
    (void)ek_dev_free(d_um);
    (void)ek_dev_free(d_kept);
    (void)ek_dev_free(d_list);
    (void)ek_dev_free(d_part);
    (void)ek_dev_free(d_rec);
    (void)ek_dev_free(d_cur);
    if (s)
        (void)ek_stream_destroy(s);
    delete[] h_mask;
    delete[] h_list;
    return rc;
}
