// ek_msm_boot.hip -- the transition counts of every bootstrap resample in one pass
// over the frames (enspara_amd/msm/bootstrap.py; the contract is DESIGN.md 4p).
//
// Replaces the loop of the reference's enspara/msm/bootstrap.py, one
// assigns_to_counts + builder per trial.  A trial draws UNITS (trajectories, or blocks
// of them) with replacement, so its count matrix is  C_trial = sum_u mult[u][trial] *
// C_u,  mult = how often the trial drew unit u: every C_trial lives on the sparsity
// pattern P of the full data's counts (CSR: indptr / cols, sorted), and one walk over
// the frames fills the table  T[cell of P][trial], int32, R = trials rounded up to 64
// columns.
//   1. SQUEEZE   the -1 frames out, per unit (ek_msm_squeeze.h, as ek_msm_counts).
//   2. CELLS     one thread per squeezed position p: cell[p] = index in P of
//                (c[p], c[p + lag]) by a lower bound in the CSR row, -1 where p starts
//                no transition (p + lag past its unit's end; not sliding: also
//                (p - unit start) % lag != 0).  A pair that P does not hold, or a state
//                outside [0, n_states), raises a flag: the entry point fails.
//   3. SCATTER   grid = (chunks of `chunk` consecutive positions) x (blocks of 64
//                trials), one wave each, lane = trial.  The wave walks its chunk with
//                wave-uniform control flow, keeps mult[unit][lane] in a register (one
//                coalesced 256-byte load per unit it enters) and sums it while the cell
//                stays the same -- a trajectory dwells, so a hot diagonal cell costs one
//                atomic per run, not per frame --; when the cell or the unit changes or
//                the chunk ends: one atomicAdd of 64 x 4 contiguous bytes, lanes with
//                nothing to add left out.  Integer adds commute: the table's bytes do
//                not depend on the chunk length or on the order the waves arrive in.
//   4. BUILD     per (trial, row of the symmetrised pattern S) one wave: v = T[ij] +
//                T[ji] as integers, the row sum exact, inv = (w > 0) ? 1 / w : 0, out =
//                inv * v: the two roundings of msm_rownorm_kernel (ek_msm.hip).
// Device memory: nnz x R x 4 bytes for the life of the handle; the frames, their cells
// and the multiplicities only inside ek_msm_boot_open.
#include "ek_common.h"
#include "ek_msm_squeeze.h"

#include <new>
#include <stdlib.h>

extern int ek_set_error(int code, const char *fmt, ...);
int ek_mi_check_memory(size_t bytes, const char *who);

#define BOOT_HIP(call)                                                         \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define BOOT_CHUNK 256                      // positions per wave of the scatter, by default
#define BOOT_BATCH_CELLS ((int64_t)1 << 25) // (trial, cell) pairs of one fetch / build launch

struct ek_msm_boot {
    int device;
    int32_t n_states, n_trials, R;
    int64_t nnz;
    int32_t *table;             // [nnz][R]
    hipStream_t s;
    hipEvent_t ev[3];
    double ms[3];               // squeeze + cells, scatter, the last build
};

// ---- 2. cells -------------------------------------------------------------------------
// flag bits: 1 a state outside [0, n_states), 2 a transition the pattern does not hold
__global__ void __launch_bounds__(EK_BLOCK)
boot_cells_kernel(const int32_t *__restrict__ c, const int64_t *__restrict__ cstart,
                  int64_t n_units, int32_t lag, int sliding, int32_t n_states,
                  const int64_t *__restrict__ indptr, const int32_t *__restrict__ cols,
                  int32_t *__restrict__ cell, int32_t *__restrict__ flag)
{
    const int64_t p = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    const int64_t m = cstart[n_units];
    if (p >= m)
        return;
    // unit of p: last u with cstart[u] <= p (an empty unit never is)
    int64_t lo = 0, hi = n_units - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (cstart[mid] <= p)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int64_t ts = cstart[lo], te = cstart[lo + 1];
    const int32_t from = c[p];
    if (from < 0 || from >= n_states) {
        atomicOr(flag, 1);
        cell[p] = -1;
        return;
    }
    bool ok = (p + lag < te);
    if (ok && !sliding)
        ok = ((p - ts) % lag) == 0;
    if (!ok) {
        cell[p] = -1;
        return;
    }
    const int32_t to = c[p + lag];      // (p + lag < te <= m)
    if (to < 0 || to >= n_states) {
        atomicOr(flag, 1);
        cell[p] = -1;
        return;
    }
    int64_t a = indptr[from], b = indptr[from + 1];
    const int64_t row_end = b;
    while (a < b) {                     // first entry of the row with cols >= to
        const int64_t mid = (a + b) >> 1;
        if (cols[mid] < to)
            a = mid + 1;
        else
            b = mid;
    }
    if (a >= row_end || cols[a] != to) {
        atomicOr(flag, 2);
        cell[p] = -1;
        return;
    }
    cell[p] = (int32_t)a;
}

// ---- 3. scatter -----------------------------------------------------------------------
__device__ __forceinline__ void boot_flush(int32_t *__restrict__ table, int32_t cur, int32_t R,
                                           int col, int32_t &acc)
{
    if (cur >= 0 && acc != 0)
        atomicAdd(&table[(size_t)cur * R + col], acc);
    acc = 0;
}

__global__ void __launch_bounds__(EK_WAVE)
boot_scatter_kernel(const int32_t *__restrict__ cell, const int64_t *__restrict__ cstart,
                    int64_t n_units, const int32_t *__restrict__ mult, int32_t R,
                    int32_t chunk, int32_t *__restrict__ table)
{
    const int lane = threadIdx.x;
    const int col = blockIdx.y * EK_WAVE + lane;    // < R: the grid has R / 64 rows
    const int64_t m = cstart[n_units];
    const int64_t base = (int64_t)blockIdx.x * chunk;
    if (base >= m)
        return;
    const int64_t end = (base + chunk < m) ? base + chunk : m;
    // unit of `base`: last u with cstart[u] <= base
    int64_t u = 0, hi = n_units - 1;
    while (u < hi) {
        const int64_t mid = (u + hi + 1) >> 1;
        if (cstart[mid] <= base)
            u = mid;
        else
            hi = mid - 1;
    }
    int64_t next = cstart[u + 1];
    int32_t w = mult[(size_t)u * R + col];
    int32_t acc = 0, cur = -1;
    for (int64_t q = base; q < end; q += EK_WAVE) {
        // 64 cells in one coalesced load, then handed round lane by lane
        const int32_t mine = (q + lane < end) ? cell[q + lane] : -1;
        const int cnt = (end - q < EK_WAVE) ? (int)(end - q) : EK_WAVE;
        for (int j = 0; j < cnt; ++j) {
            const int64_t p = q + j;
            if (p >= next) {            // (p < m = cstart[n_units]: u stays below n_units)
                boot_flush(table, cur, R, col, acc);
                cur = -1;
                do {
                    ++u;
                    next = cstart[u + 1];
                } while (p >= next);
                w = mult[(size_t)u * R + col];
            }
            const int32_t k = __builtin_amdgcn_readlane(mine, j);
            if (k != cur) {
                boot_flush(table, cur, R, col, acc);
                cur = k;
            }
            if (k >= 0)
                acc += w;
        }
    }
    boot_flush(table, cur, R, col, acc);
}

// ---- fetch: [cell][trial] int32 -> [trial][cell] int64 --------------------------------
__global__ void __launch_bounds__(EK_BLOCK)
boot_fetch_kernel(const int32_t *__restrict__ table, int64_t nnz, int32_t R, int32_t t0,
                  int32_t t1, int64_t *__restrict__ out)
{
    __shared__ int32_t tile[EK_WAVE][EK_WAVE + 1];
    const int lx = threadIdx.x & (EK_WAVE - 1), ly = threadIdx.x / EK_WAVE;
    const int64_t c0 = (int64_t)blockIdx.x * EK_WAVE;
    const int32_t tb = t0 + (int32_t)blockIdx.y * EK_WAVE;
    for (int k = 0; k < 16; ++k) {
        const int64_t cr = c0 + ly * 16 + k;
        const int32_t t = tb + lx;
        tile[ly * 16 + k][lx] = (cr < nnz && t < t1) ? table[(size_t)cr * R + t] : 0;
    }
    __syncthreads();
    for (int k = 0; k < 16; ++k) {
        const int32_t t = tb + ly * 16 + k;
        const int64_t cw = c0 + lx;
        if (t < t1 && cw < nnz)
            out[(size_t)(t - t0) * nnz + cw] = (int64_t)tile[lx][ly * 16 + k];
    }
}

// ---- 4. build -------------------------------------------------------------------------
// wave -> (trial = t0 + wave % nt, row = wave / nt): neighbouring waves read neighbouring
// columns of the same table rows
__global__ void __launch_bounds__(EK_BLOCK)
boot_build_kernel(const int32_t *__restrict__ table, int32_t R, int32_t n_states,
                  int64_t nnzS, const int64_t *__restrict__ indptrS,
                  const int64_t *__restrict__ idx_ij, const int64_t *__restrict__ idx_ji,
                  int32_t t0, int32_t nt, double *__restrict__ probs,
                  double *__restrict__ rowsum)
{
    const int64_t wv = (int64_t)blockIdx.x * (EK_BLOCK / EK_WAVE) + threadIdx.x / EK_WAVE;
    const int lane = threadIdx.x & (EK_WAVE - 1);
    if (wv >= (int64_t)nt * n_states)
        return;
    const int32_t tl = (int32_t)(wv % nt), row = (int32_t)(wv / nt);
    const int32_t t = t0 + tl;
    const int64_t lo = indptrS[row], hi = indptrS[row + 1];
    long long s = 0;
    for (int64_t j = lo + lane; j < hi; j += EK_WAVE) {
        const int64_t a = idx_ij[j], b = idx_ji[j];
        const long long v = (a >= 0 ? (long long)table[(size_t)a * R + t] : 0ll) +
                            (b >= 0 ? (long long)table[(size_t)b * R + t] : 0ll);
        s += v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        s += __shfl_xor(s, o, EK_WAVE);
    const double w = (double)s;         // exact: integers below 2^53
    const double inv = (w > 0.0) ? 1.0 / w : 0.0;
    for (int64_t j = lo + lane; j < hi; j += EK_WAVE) {
        const int64_t a = idx_ij[j], b = idx_ji[j];
        const long long v = (a >= 0 ? (long long)table[(size_t)a * R + t] : 0ll) +
                            (b >= 0 ? (long long)table[(size_t)b * R + t] : 0ll);
        probs[(size_t)tl * nnzS + j] = inv * (double)v;
    }
    if (lane == 0)
        rowsum[(size_t)tl * n_states + row] = w;
}

static int boot_bind(ek_msm_boot *h, const char *who)
{
    if (!h)
        return ek_set_error(EK_EARG, "%s: null handle", who);
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", h->device, hipGetErrorString(e));
    return EK_OK;
}

extern "C" int ek_msm_boot_close(ek_msm_boot *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(h->table);
    for (hipEvent_t e : h->ev)
        if (e)
            (void)ek_event_destroy(e);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    delete h;
    return EK_OK;
}

extern "C" int ek_msm_boot_open(int device, const int32_t *assigns, const int64_t *lengths,
                                int64_t n_units, int32_t lag_time, int32_t sliding_window,
                                int32_t n_states, int64_t nnz, const int64_t *indptr,
                                const int32_t *cols, int32_t n_trials, const int32_t *mult,
                                int32_t chunk, ek_msm_boot **out)
{
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "ek_msm_boot_open: null output");
    *out = nullptr;
    if (!assigns || !lengths || !indptr || !cols || !mult || n_units < 1 || lag_time < 1 ||
        n_states < 1 || nnz < 1 || n_trials < 1 || chunk < 0)
        return ek_set_error(EK_EARG, "ek_msm_boot_open: bad argument");
    if (n_trials > INT32_MAX - EK_WAVE || nnz > INT32_MAX)
        return ek_set_error(EK_EARG, "ek_msm_boot_open: %d trials, %lld cells: too many",
                            n_trials, (long long)nnz);
    if (chunk == 0)
        chunk = BOOT_CHUNK;
    const int32_t R = (n_trials + EK_WAVE - 1) / EK_WAVE * EK_WAVE;
    int64_t n = 0;
    for (int64_t u = 0; u < n_units; ++u) {
        if (lengths[u] < 0)
            return ek_set_error(EK_EARG, "ek_msm_boot_open: negative length");
        n += lengths[u];
        if (n >= ((int64_t)1 << 31))
            return ek_set_error(EK_EARG, "ek_msm_boot_open: 2^31 frames or more");
    }
    if (n < 1)
        return ek_set_error(EK_EARG, "ek_msm_boot_open: no frames");
    // the pattern: a CSR matrix of n_states rows, columns ascending inside a row
    if (indptr[0] != 0 || indptr[n_states] != nnz)
        return ek_set_error(EK_EARG, "ek_msm_boot_open: indptr does not span the %lld cells",
                            (long long)nnz);
    for (int32_t i = 0; i < n_states; ++i) {
        if (indptr[i + 1] < indptr[i] || indptr[i + 1] > nnz)
            return ek_set_error(EK_EARG, "ek_msm_boot_open: indptr decreases at row %d", i);
        for (int64_t j = indptr[i]; j < indptr[i + 1]; ++j)
            if (cols[j] < 0 || cols[j] >= n_states || (j > indptr[i] && cols[j] <= cols[j - 1]))
                return ek_set_error(EK_EARG, "ek_msm_boot_open: row %d of the pattern is not "
                                             "sorted inside [0, %d)", i, n_states);
    }
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess)
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
    }
    ek_msm_boot *h = new (std::nothrow) ek_msm_boot();
    int64_t *starts = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n_units + 1));
    if (!h || !starts) {
        delete h;
        free(starts);
        return ek_set_error(EK_ENOMEM, "ek_msm_boot_open: out of host memory");
    }
    starts[0] = 0;
    for (int64_t u = 0; u < n_units; ++u)
        starts[u + 1] = starts[u] + lengths[u];
    h->device = device;
    h->n_states = n_states;
    h->n_trials = n_trials;
    h->R = R;
    h->nnz = nnz;

    const int64_t nb = (n + MSM_WG - 1) / MSM_WG;
    const size_t table_bytes = (size_t)nnz * R * sizeof(int32_t);
    const size_t mult_bytes = (size_t)n_units * R * sizeof(int32_t);
    int32_t *d_a = nullptr, *d_c = nullptr, *d_cnt = nullptr, *d_cell = nullptr, *d_cols = nullptr;
    int32_t *d_mult = nullptr, *d_flag = nullptr;
    int64_t *d_off = nullptr, *d_start = nullptr, *d_cstart = nullptr, *d_indptr = nullptr;
    int32_t flag = 0;
    float ms = 0.f;
    rc = ek_mi_check_memory(table_bytes + mult_bytes + (size_t)n * 12 + (size_t)nnz * 4,
                            "ek_msm_boot_open");
    if (rc != EK_OK)
        goto done;
    BOOT_HIP(ek_stream_create_flags(&h->s, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev)
        BOOT_HIP(ek_event_create(&e));
    BOOT_HIP(ek_dev_malloc(&h->table, table_bytes));
    BOOT_HIP(ek_dev_malloc(&d_a, (size_t)n * sizeof(int32_t)));
    BOOT_HIP(ek_dev_malloc(&d_c, (size_t)n * sizeof(int32_t)));
    BOOT_HIP(ek_dev_malloc(&d_cell, (size_t)n * sizeof(int32_t)));
    BOOT_HIP(ek_dev_malloc(&d_cnt, (size_t)nb * sizeof(int32_t)));
    BOOT_HIP(ek_dev_malloc(&d_off, (size_t)(nb + 1) * sizeof(int64_t)));
    BOOT_HIP(ek_dev_malloc(&d_start, (size_t)(n_units + 1) * sizeof(int64_t)));
    BOOT_HIP(ek_dev_malloc(&d_cstart, (size_t)(n_units + 1) * sizeof(int64_t)));
    BOOT_HIP(ek_dev_malloc(&d_indptr, (size_t)(n_states + 1) * sizeof(int64_t)));
    BOOT_HIP(ek_dev_malloc(&d_cols, (size_t)nnz * sizeof(int32_t)));
    BOOT_HIP(ek_dev_malloc(&d_mult, mult_bytes));
    BOOT_HIP(ek_dev_malloc(&d_flag, sizeof(int32_t)));
    BOOT_HIP(hipMemcpyAsync(d_a, assigns, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice,
                            h->s));
    BOOT_HIP(hipMemcpyAsync(d_start, starts, (size_t)(n_units + 1) * sizeof(int64_t),
                            hipMemcpyHostToDevice, h->s));
    BOOT_HIP(hipMemcpyAsync(d_indptr, indptr, (size_t)(n_states + 1) * sizeof(int64_t),
                            hipMemcpyHostToDevice, h->s));
    BOOT_HIP(hipMemcpyAsync(d_cols, cols, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice,
                            h->s));
    BOOT_HIP(hipMemcpyAsync(d_mult, mult, mult_bytes, hipMemcpyHostToDevice, h->s));
    BOOT_HIP(hipMemsetAsync(h->table, 0, table_bytes, h->s));
    BOOT_HIP(hipMemsetAsync(d_flag, 0, sizeof(int32_t), h->s));
    BOOT_HIP(hipEventRecord(h->ev[0], h->s));
    // 1. drop the -1 frames
    hipLaunchKernelGGL(msm_count_kernel<0>, dim3((unsigned)nb), dim3(MSM_WG), 0, h->s, d_a, n,
                       d_cnt);
    hipLaunchKernelGGL(msm_scan_kernel, dim3(1), dim3(MSM_WG), 0, h->s, d_cnt, nb, d_off);
    hipLaunchKernelGGL(msm_squeeze_kernel, dim3((unsigned)nb), dim3(MSM_WG), 0, h->s, d_a, n,
                       d_off, d_c);
    hipLaunchKernelGGL(msm_cstart2_kernel, dim3(msm_blocks((n_units + 1) * EK_WAVE)),
                       dim3(EK_BLOCK), 0, h->s, d_a, n, d_start, d_off, nb, n_units, d_cstart);
    // 2. the cell of every position (a launch over all frames; the survivors' count
    //    stays on the device)
    hipLaunchKernelGGL(boot_cells_kernel, dim3(msm_blocks(n)), dim3(EK_BLOCK), 0, h->s, d_c,
                       d_cstart, n_units, lag_time, sliding_window, n_states, d_indptr, d_cols,
                       d_cell, d_flag);
    BOOT_HIP(hipEventRecord(h->ev[1], h->s));
    BOOT_HIP(hipGetLastError());
    BOOT_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(int32_t), hipMemcpyDeviceToHost, h->s));
    BOOT_HIP(hipStreamSynchronize(h->s));
    BOOT_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms[0] = ms;
    if (flag & 1) {
        rc = ek_set_error(EK_EARG, "ek_msm_boot_open: a state lies outside [0, %d)", n_states);
        goto done;
    }
    if (flag & 2) {
        rc = ek_set_error(EK_ESTATE, "ek_msm_boot_open: a transition of the frames is not in "
                                     "the pattern (the pattern is not the full data's)");
        goto done;
    }
    // 3. the table
    BOOT_HIP(hipEventRecord(h->ev[1], h->s));
    hipLaunchKernelGGL(boot_scatter_kernel,
                       dim3((unsigned)((n + chunk - 1) / chunk), (unsigned)(R / EK_WAVE)),
                       dim3(EK_WAVE), 0, h->s, d_cell, d_cstart, n_units, d_mult, R, chunk,
                       h->table);
    BOOT_HIP(hipEventRecord(h->ev[2], h->s));
    BOOT_HIP(hipGetLastError());
    BOOT_HIP(hipStreamSynchronize(h->s));
    BOOT_HIP(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
    h->ms[1] = ms;
done:
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_a);
    (void)ek_dev_free(d_c);
    (void)ek_dev_free(d_cell);
    (void)ek_dev_free(d_cnt);
    (void)ek_dev_free(d_off);
    (void)ek_dev_free(d_start);
    (void)ek_dev_free(d_cstart);
    (void)ek_dev_free(d_indptr);
    (void)ek_dev_free(d_cols);
    (void)ek_dev_free(d_mult);
    (void)ek_dev_free(d_flag);
    free(starts);
    if (rc != EK_OK) {
        ek_msm_boot_close(h);
        return rc;
    }
    *out = h;
    return EK_OK;
}

// trials of one fetch / build launch: whole blocks of 64, about BOOT_BATCH_CELLS cells
static int32_t boot_batch(int64_t cells_per_trial, int32_t n)
{
    int64_t b = BOOT_BATCH_CELLS / (cells_per_trial > 0 ? cells_per_trial : 1);
    b = b / EK_WAVE * EK_WAVE;
    if (b < EK_WAVE)
        b = EK_WAVE;
    return (int32_t)(b < n ? b : n);
}

extern "C" int ek_msm_boot_fetch(ek_msm_boot *h, int32_t r0, int32_t r1, int64_t *out)
{
    int rc = boot_bind(h, "ek_msm_boot_fetch");
    if (rc != EK_OK)
        return rc;
    if (!out || r0 < 0 || r1 < r0 || r1 > h->n_trials)
        return ek_set_error(EK_EARG, "ek_msm_boot_fetch: trials [%d, %d) of %d", r0, r1,
                            h->n_trials);
    if (r1 == r0)
        return EK_OK;
    const int32_t batch = boot_batch(h->nnz, r1 - r0);
    int64_t *d_out = nullptr;
    BOOT_HIP(ek_dev_malloc(&d_out, (size_t)batch * h->nnz * sizeof(int64_t)));
    for (int32_t t0 = r0; t0 < r1; t0 += batch) {
        const int32_t t1 = (r1 - t0 < batch) ? r1 : t0 + batch;
        hipLaunchKernelGGL(boot_fetch_kernel,
                           dim3((unsigned)((h->nnz + EK_WAVE - 1) / EK_WAVE),
                                (unsigned)((t1 - t0 + EK_WAVE - 1) / EK_WAVE)),
                           dim3(EK_BLOCK), 0, h->s, h->table, h->nnz, h->R, t0, t1, d_out);
        BOOT_HIP(hipGetLastError());
        BOOT_HIP(hipMemcpyAsync(out + (size_t)(t0 - r0) * h->nnz, d_out,
                                (size_t)(t1 - t0) * h->nnz * sizeof(int64_t),
                                hipMemcpyDeviceToHost, h->s));
        BOOT_HIP(hipStreamSynchronize(h->s));
    }
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_out);
    return rc;
}

extern "C" int ek_msm_boot_build(ek_msm_boot *h, int64_t nnzS, const int64_t *indptrS,
                                 const int64_t *idx_ij, const int64_t *idx_ji,
                                 double *probs_out, double *rowsum_out)
{
    int rc = boot_bind(h, "ek_msm_boot_build");
    if (rc != EK_OK)
        return rc;
    if (!indptrS || !idx_ij || !idx_ji || !probs_out || !rowsum_out || nnzS < 1)
        return ek_set_error(EK_EARG, "ek_msm_boot_build: bad argument");
    const int32_t ns = h->n_states;
    if (indptrS[0] != 0 || indptrS[ns] != nnzS)
        return ek_set_error(EK_EARG, "ek_msm_boot_build: indptr does not span the %lld cells",
                            (long long)nnzS);
    for (int32_t i = 0; i < ns; ++i)
        if (indptrS[i + 1] < indptrS[i] || indptrS[i + 1] > nnzS)
            return ek_set_error(EK_EARG, "ek_msm_boot_build: indptr decreases at row %d", i);
    for (int64_t j = 0; j < nnzS; ++j)
        if (idx_ij[j] < -1 || idx_ij[j] >= h->nnz || idx_ji[j] < -1 || idx_ji[j] >= h->nnz)
            return ek_set_error(EK_EARG, "ek_msm_boot_build: cell %lld points outside the "
                                         "table's %lld cells", (long long)j, (long long)h->nnz);
    h->ms[2] = 0.0;
    const int32_t batch = boot_batch(nnzS > ns ? nnzS : ns, h->n_trials);
    int64_t *d_ip = nullptr, *d_ij = nullptr, *d_ji = nullptr;
    double *d_p = nullptr, *d_rs = nullptr;
    BOOT_HIP(ek_dev_malloc(&d_ip, (size_t)(ns + 1) * sizeof(int64_t)));
    BOOT_HIP(ek_dev_malloc(&d_ij, (size_t)nnzS * sizeof(int64_t)));
    BOOT_HIP(ek_dev_malloc(&d_ji, (size_t)nnzS * sizeof(int64_t)));
    BOOT_HIP(ek_dev_malloc(&d_p, (size_t)batch * nnzS * sizeof(double)));
    BOOT_HIP(ek_dev_malloc(&d_rs, (size_t)batch * ns * sizeof(double)));
    BOOT_HIP(hipMemcpyAsync(d_ip, indptrS, (size_t)(ns + 1) * sizeof(int64_t),
                            hipMemcpyHostToDevice, h->s));
    BOOT_HIP(hipMemcpyAsync(d_ij, idx_ij, (size_t)nnzS * sizeof(int64_t), hipMemcpyHostToDevice,
                            h->s));
    BOOT_HIP(hipMemcpyAsync(d_ji, idx_ji, (size_t)nnzS * sizeof(int64_t), hipMemcpyHostToDevice,
                            h->s));
    for (int32_t t0 = 0; t0 < h->n_trials; t0 += batch) {
        const int32_t nt = (h->n_trials - t0 < batch) ? h->n_trials - t0 : batch;
        const int64_t waves = (int64_t)nt * ns;
        float ms = 0.f;
        BOOT_HIP(hipEventRecord(h->ev[0], h->s));
        hipLaunchKernelGGL(boot_build_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(EK_BLOCK),
                           0, h->s, h->table, h->R, ns, nnzS, d_ip, d_ij, d_ji, t0, nt, d_p,
                           d_rs);
        BOOT_HIP(hipEventRecord(h->ev[1], h->s));
        BOOT_HIP(hipGetLastError());
        BOOT_HIP(hipMemcpyAsync(probs_out + (size_t)t0 * nnzS, d_p,
                                (size_t)nt * nnzS * sizeof(double), hipMemcpyDeviceToHost,
                                h->s));
        BOOT_HIP(hipMemcpyAsync(rowsum_out + (size_t)t0 * ns, d_rs,
                                (size_t)nt * ns * sizeof(double), hipMemcpyDeviceToHost, h->s));
        BOOT_HIP(hipStreamSynchronize(h->s));
        BOOT_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        h->ms[2] += ms;
    }
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_ip);
    (void)ek_dev_free(d_ij);
    (void)ek_dev_free(d_ji);
    (void)ek_dev_free(d_p);
    (void)ek_dev_free(d_rs);
    return rc;
}

extern "C" int ek_msm_boot_last_timing(ek_msm_boot *h, double *ms_out)
{
    if (!h || !ms_out)
        return ek_set_error(EK_EARG, "ek_msm_boot_last_timing: null argument");
    for (int i = 0; i < 3; ++i)
        ms_out[i] = h->ms[i];
    return EK_OK;
}
