// ek_entropy.hip -- relative entropy of transition matrices, Shannon entropy of rows and
// the state histogram of discrete features.
//
// Replaces the arithmetic of the reference's enspara/info_theory/entropy.py
// (kl_divergence :199-258, js_divergence :261-264, shannon_entropy :172-196, the dense
// counts + prior -> builders.normalize of Q_from_assignments :16-41) and of
// compute_rotamer_counts in enspara/apps/compute-shannon-entropy.py :155-195.
//
// Row sums (KL, Jensen-Shannon, Shannon).  All float64, nothing fused.
//   term   KL: t = P * log(P / Q); a NaN t counts as 0 (P = 0 whatever Q is), P > 0 with
//          Q = 0 gives +inf.  JS: m = 0.5 * (P + Q) in registers, the two sums of
//          P * log(P / m) and Q * log(Q / m).  Shannon: x * log(x) for x > 0, else 0, the
//          row sum negated; with `normalize` x = p / (the row's sum), the sum taken first
//          in the order below.
//   order  A row is walked by a group of G lanes of one wave, G = 1 (cols <= 8), 8 (cols
//          <= 128) or 64.  The row's elements e0 .. e0 + cols - 1 of the flat array split
//          into a head (one element, only if e0 is odd: the rest is then 16-byte
//          aligned), pairs and a tail (one element, if one is left).  Lane g adds, onto one
//          accumulator that starts at 0: the head (g = 0 only), then the pairs g, g + G,
//          g + 2 G, .. (16-byte loads), first element before second, then the tail (g = 0
//          only).  The G accumulators are added by a butterfly: for off = G/2, G/4, .., 1
//          every lane adds the accumulator of lane g ^ off to its own (a + b == b + a, so
//          all lanes hold the same bits).  The order depends on (e0 & 1, cols) alone: the
//          same bits on every run, no float atomics.
//   flags  bit 0: some element of P is negative, bit 1: some element of Q; one integer
//          atomic-or per lane that saw one.
//
// Resident Q (ek_ent_kl_counts).  Q [n][n] is filled with 0.0 + prior, the sparse counts
// are scattered as (double)count + prior (numpy's int64 -> float64, then the add of
// Q_from_assignments), and each row is normalised as ek_msm.hip's msm_rownorm_kernel does
// for builders.normalize: the row sum added sequentially in column order (the zeros scipy's
// CSR drops add nothing), inv = 1 / sum once (0 for an empty row), Q = inv * Q.  Then the
// KL kernel runs on P and Q.
//
// State counts.  codes [frames][F] bytes -> counts [F][n_states] uint64.  A workgroup is
// 64 features (lanes along the feature axis: a wave's byte loads are one contiguous 64 B)
// by 4 waves that take every fourth frame of the workgroup's chunks of ENT_SC_CHUNK frames.
// n_states <= 4: a lane keeps its column's counters in registers.  More: the workgroup
// keeps [n_states][64] uint32 counters in the LDS (256 n_states bytes, allocated by the
// launch: 5 states leave the CU's occupancy alone, 255 take 65 280 bytes; integer LDS
// atomics between its four waves).  Either adds what it counted to the uint64 totals with integer atomics, exact in
// any order.  A code >= n_states counts nowhere.
#include "ek_common.h"
#include "ek_mi_launch.h"

#include <math.h>
#include <new>

extern int ek_set_error(int code, const char *fmt, ...);

#define ENT_HIP(call)                                                          \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define ENT_WG 256
#define ENT_G1_COLS 8           // rows up to this wide: one lane a row
#define ENT_G8_COLS 128         // ... up to this wide: eight lanes a row; wider: a wave
#define ENT_SC_CHUNK 8192       // frames of one chunk of the state-count kernels
#define ENT_SC_REG 4            // states a lane counts in registers
#define ENT_SC_MAX_GRID_Y 4096

static double ent_ms[3];        // upload, building Q (ek_ent_kl_counts), row kernel: the last call's

static int ent_group(int64_t cols) { return cols <= ENT_G1_COLS ? 1 : cols <= ENT_G8_COLS ? 8 : 64; }

// ---- the walk of one row by G lanes (see the head of this file) -------------------------
// one(e): the element of flat index e; two(e): the 16-byte aligned pair at e, e + 1
template <int G, class One, class Two>
__device__ __forceinline__ void ent_walk(int64_t e0, int64_t cols, int g, One one, Two two)
{
    if (cols <= 0)
        return;
    const int64_t head = e0 & 1;
    const int64_t pairs = (cols - head) >> 1;
    const int64_t tail = (cols - head) & 1;
    if (g == 0 && head)
        one(e0);
#pragma unroll 2
    for (int64_t k = g; k < pairs; k += G)
        two(e0 + head + 2 * k);
    if (g == 0 && tail)
        one(e0 + cols - 1);
}

template <int G>
__device__ __forceinline__ double ent_butterfly(double a)
{
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1)
        a = a + __shfl_xor(a, off, EK_WAVE);
    return a;
}

__device__ __forceinline__ double ent_kl_term(double p, double q)
{
    const double t = p * log(p / q);
    return t != t ? 0.0 : t;
}

// out_a[r] = sum_j P log(P / Q); JS: out_a[r], out_b[r] = the sums against m = 0.5 (P + Q)
template <int G, int JS>
__global__ void __launch_bounds__(ENT_WG)
ent_kl_kernel(const double *__restrict__ P, const double *__restrict__ Q, int64_t rows,
              int64_t cols, double *__restrict__ out_a, double *__restrict__ out_b,
              uint32_t *__restrict__ flags)
{
    const int64_t gid = (int64_t)blockIdx.x * ENT_WG + threadIdx.x;
    const int64_t row = gid / G;
    const int g = (int)(gid % G);
    const bool live = row < rows;       // (no early return: the butterfly takes every lane)
    double a = 0.0, b = 0.0;
    uint32_t bad = 0;
    auto term = [&](double p, double q) {
        bad |= (p < 0.0 ? 1u : 0u) | (q < 0.0 ? 2u : 0u);
        if (JS) {
            const double m = 0.5 * (p + q);
            a = a + ent_kl_term(p, m);
            b = b + ent_kl_term(q, m);
        } else {
            a = a + ent_kl_term(p, q);
        }
    };
    ent_walk<G>(
        row * cols, live ? cols : 0, g, [&](int64_t e) { term(P[e], Q[e]); },
        [&](int64_t e) {
            const double2 p = *reinterpret_cast<const double2 *>(P + e);
            const double2 q = *reinterpret_cast<const double2 *>(Q + e);
            term(p.x, q.x);
            term(p.y, q.y);
        });
    a = ent_butterfly<G>(a);
    if (JS)
        b = ent_butterfly<G>(b);
    if (live && g == 0) {
        out_a[row] = a;
        if (JS)
            out_b[row] = b;
    }
    if (bad)
        atomicOr(flags, bad);
}

template <int G>
__global__ void __launch_bounds__(ENT_WG)
ent_shannon_kernel(const double *__restrict__ p, int64_t rows, int64_t cols, int normalize,
                   double *__restrict__ out)
{
    const int64_t gid = (int64_t)blockIdx.x * ENT_WG + threadIdx.x;
    const int64_t row = gid / G;
    const int g = (int)(gid % G);
    const bool live = row < rows;
    const int64_t e0 = row * cols, c = live ? cols : 0;
    double sum = 1.0;
    if (normalize) {
        double s = 0.0;
        ent_walk<G>(
            e0, c, g, [&](int64_t e) { s = s + p[e]; },
            [&](int64_t e) {
                const double2 v = *reinterpret_cast<const double2 *>(p + e);
                s = s + v.x;
                s = s + v.y;
            });
        sum = ent_butterfly<G>(s);
    }
    double a = 0.0;
    auto term = [&](double x) {
        if (normalize)
            x = x / sum;
        a = a + (x > 0.0 ? x * log(x) : 0.0);
    };
    ent_walk<G>(
        e0, c, g, [&](int64_t e) { term(p[e]); },
        [&](int64_t e) {
            const double2 v = *reinterpret_cast<const double2 *>(p + e);
            term(v.x);
            term(v.y);
        });
    a = ent_butterfly<G>(a);
    if (live && g == 0)
        out[row] = -a;
}

static unsigned ent_row_blocks(int64_t rows, int G)
{
    return (unsigned)((rows * G + ENT_WG - 1) / ENT_WG);
}

static void ent_launch_kl(const double *P, const double *Q, int64_t rows, int64_t cols, int js,
                          double *out_a, double *out_b, uint32_t *flags, hipStream_t s)
{
    const int G = ent_group(cols);
    const dim3 grid(ent_row_blocks(rows, G)), wg(ENT_WG);
#define ENT_KL(G_, JS_)                                                                  \
    hipLaunchKernelGGL((ent_kl_kernel<G_, JS_>), grid, wg, 0, s, P, Q, rows, cols, out_a, \
                       out_b, flags)
    if (js) {
        if (G == 1) ENT_KL(1, 1); else if (G == 8) ENT_KL(8, 1); else ENT_KL(64, 1);
    } else {
        if (G == 1) ENT_KL(1, 0); else if (G == 8) ENT_KL(8, 0); else ENT_KL(64, 0);
    }
#undef ENT_KL
}

// rows x cols the row kernels take: the grid fits, the flat index fits
static int ent_check_rows(int64_t rows, int64_t cols, const char *who)
{
    if (rows < 1 || cols < 1 || rows > ((int64_t)1 << 40) / cols ||
        (rows * ent_group(cols) + ENT_WG - 1) / ENT_WG > 0x7fffffff)
        return ek_set_error(EK_EARG, "%s: %lld x %lld is empty or too large", who,
                            (long long)rows, (long long)cols);
    return EK_OK;
}

static int ent_set_device(int device)
{
    hipError_t e0 = hipSetDevice(device);
    if (e0 != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
    return EK_OK;
}

static int ent_kl_run(int device, int64_t rows, int64_t cols, const double *P, const double *Q,
                      int js, double *out_a, double *out_b, uint32_t *flags_out, const char *who)
{
    int rc = EK_OK;
    if (!P || !Q || !out_a || (js && !out_b) || !flags_out)
        return ek_set_error(EK_EARG, "%s: null argument", who);
    if ((rc = ent_check_rows(rows, cols, who)) != EK_OK || (rc = ent_set_device(device)) != EK_OK)
        return rc;
    const size_t in_b = (size_t)rows * cols * sizeof(double), out_b_ = (size_t)rows * sizeof(double);
    if ((rc = ek_mi_check_memory(2 * in_b + 2 * out_b_ + 256, who)) != EK_OK)
        return rc;
    double *d_P = nullptr, *d_Q = nullptr, *d_a = nullptr, *d_b = nullptr;
    uint32_t *d_flags = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float ms = 0.f;
    ENT_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    for (hipEvent_t &e : ev)
        ENT_HIP(ek_event_create(&e));
    ENT_HIP(ek_dev_malloc((void **)&d_P, in_b));
    ENT_HIP(ek_dev_malloc((void **)&d_Q, in_b));
    ENT_HIP(ek_dev_malloc((void **)&d_a, out_b_));
    ENT_HIP(ek_dev_malloc((void **)&d_b, out_b_));
    ENT_HIP(ek_dev_malloc((void **)&d_flags, sizeof(uint32_t)));
    ENT_HIP(hipEventRecord(ev[0], s));
    ENT_HIP(hipMemcpyAsync(d_P, P, in_b, hipMemcpyHostToDevice, s));
    ENT_HIP(hipMemcpyAsync(d_Q, Q, in_b, hipMemcpyHostToDevice, s));
    ENT_HIP(hipMemsetAsync(d_flags, 0, sizeof(uint32_t), s));
    ENT_HIP(hipEventRecord(ev[1], s));
    ent_launch_kl(d_P, d_Q, rows, cols, js, d_a, d_b, d_flags, s);
    ENT_HIP(hipEventRecord(ev[2], s));
    ENT_HIP(hipGetLastError());
    ENT_HIP(hipMemcpyAsync(out_a, d_a, out_b_, hipMemcpyDeviceToHost, s));
    if (js)
        ENT_HIP(hipMemcpyAsync(out_b, d_b, out_b_, hipMemcpyDeviceToHost, s));
    ENT_HIP(hipMemcpyAsync(flags_out, d_flags, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ENT_HIP(hipStreamSynchronize(s));
    ENT_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    ent_ms[0] = ms;
    ent_ms[1] = 0.0;
    ENT_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
    ent_ms[2] = ms;
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_P);
    (void)ek_dev_free(d_Q);
    (void)ek_dev_free(d_a);
    (void)ek_dev_free(d_b);
    (void)ek_dev_free(d_flags);
    for (hipEvent_t e : ev)
        if (e)
            (void)ek_event_destroy(e);
    if (s)
        (void)ek_stream_destroy(s);
    return rc;
}

extern "C" int ek_ent_kl_rows(int device, int64_t rows, int64_t cols, const double *P,
                              const double *Q, double *out, uint32_t *flags_out)
{
    return ent_kl_run(device, rows, cols, P, Q, 0, out, nullptr, flags_out, "ek_ent_kl_rows");
}

extern "C" int ek_ent_js_rows(int device, int64_t rows, int64_t cols, const double *P,
                              const double *Q, double *out_p, double *out_q, uint32_t *flags_out)
{
    return ent_kl_run(device, rows, cols, P, Q, 1, out_p, out_q, flags_out, "ek_ent_js_rows");
}

extern "C" int ek_ent_shannon_rows(int device, int64_t rows, int64_t cols, const double *p,
                                   int32_t normalize, double *out)
{
    int rc = EK_OK;
    if (!p || !out)
        return ek_set_error(EK_EARG, "ek_ent_shannon_rows: null argument");
    if ((rc = ent_check_rows(rows, cols, "ek_ent_shannon_rows")) != EK_OK ||
        (rc = ent_set_device(device)) != EK_OK)
        return rc;
    const size_t in_b = (size_t)rows * cols * sizeof(double), out_b = (size_t)rows * sizeof(double);
    if ((rc = ek_mi_check_memory(in_b + out_b, "ek_ent_shannon_rows")) != EK_OK)
        return rc;
    double *d_p = nullptr, *d_out = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float ms = 0.f;
    const int G = ent_group(cols);
    const dim3 grid(ent_row_blocks(rows, G)), wg(ENT_WG);
    const int norm = normalize ? 1 : 0;
    ENT_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    for (hipEvent_t &e : ev)
        ENT_HIP(ek_event_create(&e));
    ENT_HIP(ek_dev_malloc((void **)&d_p, in_b));
    ENT_HIP(ek_dev_malloc((void **)&d_out, out_b));
    ENT_HIP(hipEventRecord(ev[0], s));
    ENT_HIP(hipMemcpyAsync(d_p, p, in_b, hipMemcpyHostToDevice, s));
    ENT_HIP(hipEventRecord(ev[1], s));
    if (G == 1)
        hipLaunchKernelGGL(ent_shannon_kernel<1>, grid, wg, 0, s, d_p, rows, cols, norm, d_out);
    else if (G == 8)
        hipLaunchKernelGGL(ent_shannon_kernel<8>, grid, wg, 0, s, d_p, rows, cols, norm, d_out);
    else
        hipLaunchKernelGGL(ent_shannon_kernel<64>, grid, wg, 0, s, d_p, rows, cols, norm, d_out);
    ENT_HIP(hipEventRecord(ev[2], s));
    ENT_HIP(hipGetLastError());
    ENT_HIP(hipMemcpyAsync(out, d_out, out_b, hipMemcpyDeviceToHost, s));
    ENT_HIP(hipStreamSynchronize(s));
    ENT_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    ent_ms[0] = ms;
    ent_ms[1] = 0.0;
    ENT_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
    ent_ms[2] = ms;
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_p);
    (void)ek_dev_free(d_out);
    for (hipEvent_t e : ev)
        if (e)
            (void)ek_event_destroy(e);
    if (s)
        (void)ek_stream_destroy(s);
    return rc;
}

// ---- Q from sparse counts, resident ----------------------------------------------------
__global__ void __launch_bounds__(ENT_WG)
ent_fill_kernel(double *__restrict__ Q, int64_t cells, double prior)
{
    const int64_t i = (int64_t)blockIdx.x * ENT_WG + threadIdx.x;
    if (i < cells)
        Q[i] = 0.0 + prior;
}

__global__ void __launch_bounds__(ENT_WG)
ent_scatter_kernel(const int32_t *__restrict__ ci, const int32_t *__restrict__ cj,
                   const int64_t *__restrict__ cv, int64_t nnz, int32_t n, double prior,
                   double *__restrict__ Q)
{
    const int64_t k = (int64_t)blockIdx.x * ENT_WG + threadIdx.x;
    if (k >= nnz)
        return;
    const int32_t i = ci[k], j = cj[k];
    if (i < 0 || i >= n || j < 0 || j >= n)     // (the host has checked; never out of bounds)
        return;
    Q[(int64_t)i * n + j] = (double)cv[k] + prior;
}

// one wave per row: 64 columns at a time, every lane adds them in column order (the lanes
// behind the row's end hold 0.0, which adds nothing), so all hold the sequential sum
__global__ void __launch_bounds__(ENT_WG)
ent_rownorm_kernel(double *__restrict__ Q, int32_t n)
{
    const int64_t row = (int64_t)blockIdx.x * (ENT_WG / EK_WAVE) + threadIdx.x / EK_WAVE;
    const int lane = threadIdx.x & (EK_WAVE - 1);
    if (row >= n)           // (whole waves leave: the shuffles below stay among full waves)
        return;
    double *q = Q + row * n;
    double w = 0.0;
    for (int32_t base = 0; base < n; base += EK_WAVE) {
        const double x = base + lane < n ? q[base + lane] : 0.0;
#pragma unroll 8
        for (int l = 0; l < EK_WAVE; ++l)
            w = w + __shfl(x, l, EK_WAVE);
    }
    const double inv = (w > 0.0) ? 1.0 / w : 0.0;
    for (int32_t j = lane; j < n; j += EK_WAVE)
        q[j] = inv * q[j];
}

extern "C" int ek_ent_kl_counts(int device, int32_t n, const double *P, int64_t nnz,
                                const int32_t *ci, const int32_t *cj, const int64_t *cv,
                                double prior, double *out, uint32_t *flags_out)
{
    int rc = EK_OK;
    if (!P || !out || !flags_out || nnz < 0 || (nnz > 0 && (!ci || !cj || !cv)) || !(prior >= 0.0))
        return ek_set_error(EK_EARG, "ek_ent_kl_counts: bad argument (arrays, nnz >= 0, "
                                     "prior >= 0)");
    if ((rc = ent_check_rows(n, n, "ek_ent_kl_counts")) != EK_OK)
        return rc;
    for (int64_t k = 0; k < nnz; ++k)
        if (ci[k] < 0 || ci[k] >= n || cj[k] < 0 || cj[k] >= n || cv[k] < 0)
            return ek_set_error(EK_EARG, "ek_ent_kl_counts: entry %lld (%d, %d: %lld) is not "
                                         "a count of a %d x %d matrix", (long long)k, ci[k],
                                cj[k], (long long)cv[k], n, n);
    if ((rc = ent_set_device(device)) != EK_OK)
        return rc;
    const int64_t cells = (int64_t)n * n;
    const size_t in_b = (size_t)cells * sizeof(double), out_b = (size_t)n * sizeof(double);
    const size_t nz = (size_t)(nnz > 0 ? nnz : 1);
    if ((rc = ek_mi_check_memory(2 * in_b + out_b + nz * 16 + 256, "ek_ent_kl_counts")) != EK_OK)
        return rc;
    double *d_P = nullptr, *d_Q = nullptr, *d_out = nullptr;
    int32_t *d_ci = nullptr, *d_cj = nullptr;
    int64_t *d_cv = nullptr;
    uint32_t *d_flags = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float ms = 0.f;
    ENT_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    for (hipEvent_t &e : ev)
        ENT_HIP(ek_event_create(&e));
    ENT_HIP(ek_dev_malloc((void **)&d_P, in_b));
    ENT_HIP(ek_dev_malloc((void **)&d_Q, in_b));
    ENT_HIP(ek_dev_malloc((void **)&d_out, out_b));
    ENT_HIP(ek_dev_malloc((void **)&d_ci, nz * sizeof(int32_t)));
    ENT_HIP(ek_dev_malloc((void **)&d_cj, nz * sizeof(int32_t)));
    ENT_HIP(ek_dev_malloc((void **)&d_cv, nz * sizeof(int64_t)));
    ENT_HIP(ek_dev_malloc((void **)&d_flags, sizeof(uint32_t)));
    ENT_HIP(hipEventRecord(ev[0], s));
    ENT_HIP(hipMemcpyAsync(d_P, P, in_b, hipMemcpyHostToDevice, s));
    if (nnz > 0) {
        ENT_HIP(hipMemcpyAsync(d_ci, ci, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, s));
        ENT_HIP(hipMemcpyAsync(d_cj, cj, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, s));
        ENT_HIP(hipMemcpyAsync(d_cv, cv, (size_t)nnz * sizeof(int64_t), hipMemcpyHostToDevice, s));
    }
    ENT_HIP(hipMemsetAsync(d_flags, 0, sizeof(uint32_t), s));
    ENT_HIP(hipEventRecord(ev[1], s));
    hipLaunchKernelGGL(ent_fill_kernel, dim3((unsigned)((cells + ENT_WG - 1) / ENT_WG)),
                       dim3(ENT_WG), 0, s, d_Q, cells, prior);
    if (nnz > 0)
        hipLaunchKernelGGL(ent_scatter_kernel, dim3((unsigned)((nnz + ENT_WG - 1) / ENT_WG)),
                           dim3(ENT_WG), 0, s, d_ci, d_cj, d_cv, nnz, n, prior, d_Q);
    hipLaunchKernelGGL(ent_rownorm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(ENT_WG), 0, s,
                       d_Q, n);
    ENT_HIP(hipEventRecord(ev[2], s));
    ent_launch_kl(d_P, d_Q, n, n, 0, d_out, nullptr, d_flags, s);
    ENT_HIP(hipEventRecord(ev[3], s));
    ENT_HIP(hipGetLastError());
    ENT_HIP(hipMemcpyAsync(out, d_out, out_b, hipMemcpyDeviceToHost, s));
    ENT_HIP(hipMemcpyAsync(flags_out, d_flags, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ENT_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < 3; ++q) {
        ENT_HIP(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
        ent_ms[q] = ms;
    }
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_P);
    (void)ek_dev_free(d_Q);
    (void)ek_dev_free(d_out);
    (void)ek_dev_free(d_ci);
    (void)ek_dev_free(d_cj);
    (void)ek_dev_free(d_cv);
    (void)ek_dev_free(d_flags);
    for (hipEvent_t e : ev)
        if (e)
            (void)ek_event_destroy(e);
    if (s)
        (void)ek_stream_destroy(s);
    return rc;
}

extern "C" int ek_ent_last_timing(double *ms_out)
{
    if (!ms_out)
        return ek_set_error(EK_EARG, "ek_ent_last_timing: null argument");
    for (int i = 0; i < 3; ++i)
        ms_out[i] = ent_ms[i];
    return EK_OK;
}

// ---- state counts -------------------------------------------------------------------------
// the frames this wave takes: chunk c = blockIdx.y, + gridDim.y, ..; in it every fourth frame
template <int NS>
__global__ void __launch_bounds__(ENT_WG)
ent_sc_reg_kernel(const uint8_t *__restrict__ codes, int64_t frames, int32_t F,
                  unsigned long long *__restrict__ counts)
{
    const int lane = threadIdx.x & (EK_WAVE - 1), w = threadIdx.x / EK_WAVE;
    const int64_t f = (int64_t)blockIdx.x * EK_WAVE + lane;
    if (f >= F)             // (no barrier or shuffle below)
        return;
    uint32_t c[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k)
        c[k] = 0;
    const int64_t chunks = (frames + ENT_SC_CHUNK - 1) / ENT_SC_CHUNK;
    for (int64_t ch = blockIdx.y; ch < chunks; ch += gridDim.y) {
        const int64_t te = (ch + 1) * (int64_t)ENT_SC_CHUNK, t1 = te < frames ? te : frames;
        int64_t t = ch * (int64_t)ENT_SC_CHUNK + w;
        for (; t + 12 < t1; t += 16) {          // four loads in flight
            uint32_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                v[u] = codes[(t + 4 * u) * F + f];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < NS; ++k)
                    c[k] += v[u] == (uint32_t)k ? 1u : 0u;
        }
        for (; t < t1; t += 4) {
            const uint32_t v = codes[t * F + f];
#pragma unroll
            for (int k = 0; k < NS; ++k)
                c[k] += v == (uint32_t)k ? 1u : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < NS; ++k)
        if (c[k])
            atomicAdd(&counts[f * NS + k], (unsigned long long)c[k]);
}

__global__ void __launch_bounds__(ENT_WG)
ent_sc_lds_kernel(const uint8_t *__restrict__ codes, int64_t frames, int32_t F, int32_t n_states,
                  unsigned long long *__restrict__ counts)
{
    extern __shared__ uint32_t h[];             // [n_states][64], sized by the launch
    const int lane = threadIdx.x & (EK_WAVE - 1), w = threadIdx.x / EK_WAVE;
    const int64_t f = (int64_t)blockIdx.x * EK_WAVE + lane;
    const int cells = n_states * EK_WAVE;       // n_states <= MI_MAX_STATES: the host checks
    for (int i = threadIdx.x; i < cells; i += ENT_WG)
        h[i] = 0;
    __syncthreads();
    if (f < F) {
        const int64_t chunks = (frames + ENT_SC_CHUNK - 1) / ENT_SC_CHUNK;
        for (int64_t ch = blockIdx.y; ch < chunks; ch += gridDim.y) {
            const int64_t te = (ch + 1) * (int64_t)ENT_SC_CHUNK, t1 = te < frames ? te : frames;
            for (int64_t t = ch * (int64_t)ENT_SC_CHUNK + w; t < t1; t += 4) {
                const int v = codes[t * F + f];
                if (v < n_states)
                    atomicAdd(&h[v * EK_WAVE + lane], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += ENT_WG) {
        const int64_t ff = (int64_t)blockIdx.x * EK_WAVE + (i & (EK_WAVE - 1));
        if (ff < F && h[i])
            atomicAdd(&counts[ff * n_states + i / EK_WAVE], (unsigned long long)h[i]);
    }
}

struct ek_ent_state_counts {
    int device;
    int32_t F, n_states;
    unsigned long long *d_counts;
    hipStream_t s;
    double ms[2];           // the last add's upload, its kernel
};

extern "C" int ek_ent_state_counts_open(int device, int32_t F, int32_t n_states,
                                        ek_ent_state_counts **out)
{
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "ek_ent_state_counts_open: null argument");
    *out = nullptr;
    if ((rc = ek_mi_check_shape(F, F, n_states, n_states, "ek_ent_state_counts_open")) != EK_OK ||
        (rc = ent_set_device(device)) != EK_OK)
        return rc;
    const size_t bytes = (size_t)F * n_states * sizeof(unsigned long long);
    if ((rc = ek_mi_check_memory(bytes, "ek_ent_state_counts_open")) != EK_OK)
        return rc;
    ek_ent_state_counts *h = new (std::nothrow) ek_ent_state_counts();
    if (!h)
        return ek_set_error(EK_ENOMEM, "ek_ent_state_counts_open: out of host memory");
    h->device = device;
    h->F = F;
    h->n_states = n_states;
    ENT_HIP(ek_stream_create_flags(&h->s, hipStreamNonBlocking));
    ENT_HIP(ek_dev_malloc((void **)&h->d_counts, bytes));
    ENT_HIP(hipMemsetAsync(h->d_counts, 0, bytes, h->s));
    ENT_HIP(hipStreamSynchronize(h->s));
    *out = h;
    return EK_OK;
done:
    (void)ek_dev_free(h->d_counts);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    delete h;
    return rc;
}

extern "C" int ek_ent_state_counts_add(ek_ent_state_counts *h, const uint8_t *codes,
                                       int64_t frames)
{
    int rc = EK_OK;
    if (!h || frames < 0 || (frames > 0 && !codes) || frames >= ((int64_t)1 << 31) - 64)
        return ek_set_error(EK_EARG, "ek_ent_state_counts_add: bad argument (0 <= frames < "
                                     "2^31 - 64)");
    if (frames == 0)
        return EK_OK;
    if ((rc = ent_set_device(h->device)) != EK_OK)
        return rc;
    const size_t raw_b = (size_t)frames * h->F;
    if ((rc = ek_mi_check_memory(raw_b, "ek_ent_state_counts_add")) != EK_OK)
        return rc;
    uint8_t *d_codes = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float ms = 0.f;
    const int64_t chunks = (frames + ENT_SC_CHUNK - 1) / ENT_SC_CHUNK;
    const dim3 grid((unsigned)((h->F + EK_WAVE - 1) / EK_WAVE),
                    (unsigned)(chunks < ENT_SC_MAX_GRID_Y ? chunks : ENT_SC_MAX_GRID_Y)),
        wg(ENT_WG);
    for (hipEvent_t &e : ev)
        ENT_HIP(ek_event_create(&e));
    ENT_HIP(ek_dev_malloc((void **)&d_codes, raw_b));
    ENT_HIP(hipEventRecord(ev[0], h->s));
    ENT_HIP(hipMemcpyAsync(d_codes, codes, raw_b, hipMemcpyHostToDevice, h->s));
    ENT_HIP(hipEventRecord(ev[1], h->s));
    switch (h->n_states) {
    case 1:
        hipLaunchKernelGGL(ent_sc_reg_kernel<1>, grid, wg, 0, h->s, d_codes, frames, h->F,
                           h->d_counts);
        break;
    case 2:
        hipLaunchKernelGGL(ent_sc_reg_kernel<2>, grid, wg, 0, h->s, d_codes, frames, h->F,
                           h->d_counts);
        break;
    case 3:
        hipLaunchKernelGGL(ent_sc_reg_kernel<3>, grid, wg, 0, h->s, d_codes, frames, h->F,
                           h->d_counts);
        break;
    case ENT_SC_REG:
        hipLaunchKernelGGL(ent_sc_reg_kernel<ENT_SC_REG>, grid, wg, 0, h->s, d_codes, frames,
                           h->F, h->d_counts);
        break;
    default:
        hipLaunchKernelGGL(ent_sc_lds_kernel, grid, wg,
                           (size_t)h->n_states * EK_WAVE * sizeof(uint32_t), h->s, d_codes,
                           frames, h->F, h->n_states, h->d_counts);
    }
    ENT_HIP(hipEventRecord(ev[2], h->s));
    ENT_HIP(hipGetLastError());
    ENT_HIP(hipStreamSynchronize(h->s));
    for (int q = 0; q < 2; ++q) {
        ENT_HIP(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
        h->ms[q] = ms;
    }
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_codes);
    for (hipEvent_t e : ev)
        if (e)
            (void)ek_event_destroy(e);
    return rc;
}

extern "C" int ek_ent_state_counts_read(ek_ent_state_counts *h, uint64_t *counts_out)
{
    int rc = EK_OK;
    if (!h || !counts_out)
        return ek_set_error(EK_EARG, "ek_ent_state_counts_read: null argument");
    if ((rc = ent_set_device(h->device)) != EK_OK)
        return rc;
    ENT_HIP(hipMemcpyAsync(counts_out, h->d_counts,
                           (size_t)h->F * h->n_states * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, h->s));
    ENT_HIP(hipStreamSynchronize(h->s));
done:
    return rc;
}

extern "C" int ek_ent_state_counts_last_timing(ek_ent_state_counts *h, double *ms_out)
{
    if (!h || !ms_out)
        return ek_set_error(EK_EARG, "ek_ent_state_counts_last_timing: null argument");
    ms_out[0] = h->ms[0];
    ms_out[1] = h->ms[1];
    return EK_OK;
}

extern "C" int ek_ent_state_counts_close(ek_ent_state_counts *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(h->d_counts);
    (void)ek_stream_destroy(h->s);
    delete h;
    return EK_OK;
}
