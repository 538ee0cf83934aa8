// ek_wmi.hip -- joint probabilities and mutual information of discrete features whose
// frames carry float64 weights.
//
// Replaces the arithmetic of the reference's weighted_mi
// (enspara/info_theory/mutual_info.py:78-178).
//
//   P[i][j][u][v] = sum over frames t of w_t [f_ti == u] [f_tj == v]
//
// is the product (diag(w) OneHot)^T OneHot with (F S) rows and columns and the frames
// as the summed index, in float64 on v_mfma_f64_16x16x4_f64.  No one-hot array exists
// in memory:
//   pack     ek_mi's: the uploaded codes [frames][F] uint8 -> feature-major [F][frames
//            padded to 64 with MI_PAD]; the weights are padded with zeros
//   product  a workgroup owns 64 rows x 64 columns and one chunk of frames, each of
//            its four waves 2 x 2 tiles of 16 x 16.  Row r of the product is (feature
//            r / S, state r % S).  Lane l gives the MFMA row (A) and column (B) l & 15
//            and summed index l >> 4: per step of 32 frames it loads the 8 codes of
//            frames t + 8 (l >> 4) .. + 7 of its rows' and columns' features and their
//            8 weights, and for m = 0 .. 7 makes A = (code == u ? w : 0.0), B = (code
//            == v ? 1.0 : 0.0) in registers.  The partial tile goes to part[chunk].
//   reduce   P = part[0]; P = P + part[c] for c = 1, 2, ..: one lane per cell, into the
//            [F][F][S][S] layout
//   info     one lane per feature pair, the reference's operations in float64, terms
//            added u outer, v inner; the marginal P_x[i][u] is the cell P[i][i][u][u],
//            which is sum_t w_t [f_ti == u] by the same tree
// The summation tree of a cell is therefore fixed by the number of frames alone: within
// a chunk the frames 32 s + 8 g + m, added g = 0 .. 3 inside one MFMA (the hardware's
// order), MFMAs m = 0 .. 7 then steps s in sequence onto one accumulator; then the
// chunks in ascending order.  No atomics: two runs give the same bits.
// C/D lane map (as in ek_lu.hip): column l & 15, row (l >> 4) + 4 register.
#include "ek_common.h"
#include "ek_mi_launch.h"

#include <math.h>

extern int ek_set_error(int code, const char *fmt, ...);

#define WMI_HIP(call)                                                          \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define WMI_WG 256
#define WMI_BLOCK 64            // rows / columns of a workgroup: 2 x 2 waves of 32 x 32
#define WMI_CHUNK 2048          // frames of a chunk, at least (info_theory.WMI_CHUNK)
#define WMI_MAX_CHUNKS 64       // ... and at most this many chunks: longer input, longer chunks

static double wmi_ms[4];        // upload + pack, product, reduce, information: the last run's

// frames of one chunk for `frames` frames: WMI_CHUNK, or what makes WMI_MAX_CHUNKS chunks,
// in whole steps of 64
static int64_t wmi_chunk(int64_t frames)
{
    int64_t c = (frames + WMI_MAX_CHUNKS - 1) / WMI_MAX_CHUNKS;
    c = (c + 63) / 64 * 64;
    return c < WMI_CHUNK ? WMI_CHUNK : c;
}

__device__ __forceinline__ uint32_t wmi_byte(uint2 c, int m)
{
    return ((m < 4 ? c.x >> (8 * m) : c.y >> (8 * (m - 4))) & 0xffu);
}

// grid: x column blocks, y row blocks, z chunks.  Rows and columns past the product's
// edge read the last one and are not written.
__global__ void __launch_bounds__(WMI_WG)
wmi_product_kernel(const uint8_t *__restrict__ codes, const double *__restrict__ w, int64_t tpad,
                   int64_t chunk, int32_t S, int32_t M, double *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, l = lane & 15;
    const int32_t r0 = (int32_t)blockIdx.y * WMI_BLOCK + (wave >> 1) * 32;
    const int32_t c0 = (int32_t)blockIdx.x * WMI_BLOCK + (wave & 1) * 32;
    const int64_t t0 = (int64_t)blockIdx.z * chunk;
    const int64_t t1 = (t0 + chunk < tpad) ? t0 + chunk : tpad;

    const uint8_t *pa[2], *pb[2];
    uint32_t ua[2], ub[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int32_t r = r0 + 16 * q + l;
        r = (r < M) ? r : M - 1;
        pa[q] = codes + (size_t)(r / S) * tpad + 8 * g;
        ua[q] = (uint32_t)(r % S);
        int32_t c = c0 + 16 * q + l;
        c = (c < M) ? c : M - 1;
        pb[q] = codes + (size_t)(c / S) * tpad + 8 * g;
        ub[q] = (uint32_t)(c % S);
    }
    typedef double wmi_v4d __attribute__((ext_vector_type(4)));
    wmi_v4d acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
            acc[a][b] = wmi_v4d{0.0, 0.0, 0.0, 0.0};

    for (int64_t t = t0; t < t1; t += 32) {
        uint2 ca[2], cb[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            ca[q] = *reinterpret_cast<const uint2 *>(pa[q] + t);
            cb[q] = *reinterpret_cast<const uint2 *>(pb[q] + t);
        }
        double wv[8];
#pragma unroll
        for (int m = 0; m < 8; ++m)
            wv[m] = w[t + 8 * g + m];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            double a[2], b[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                a[q] = (wmi_byte(ca[q], m) == ua[q]) ? wv[m] : 0.0;
                b[q] = (wmi_byte(cb[q], m) == ub[q]) ? 1.0 : 0.0;
            }
#pragma unroll
            for (int qa = 0; qa < 2; ++qa)
#pragma unroll
                for (int qb = 0; qb < 2; ++qb)
                    acc[qa][qb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[qa], b[qb], acc[qa][qb],
                                                                       0, 0, 0);
        }
    }

    double *out = part + (size_t)blockIdx.z * M * M;
#pragma unroll
    for (int qa = 0; qa < 2; ++qa)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb) {
            const int32_t c = c0 + 16 * qb + l;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int32_t r = r0 + 16 * qa + g + 4 * k;
                if (r < M && c < M)
                    out[(size_t)r * M + c] = acc[qa][qb][k];
            }
        }
}

// P[i][j][u][v] = part[0][r][c] + part[1][r][c] + .. in that order, r = i S + u, c = j S + v
__global__ void __launch_bounds__(WMI_WG)
wmi_reduce_kernel(const double *__restrict__ part, int32_t chunks, int32_t F, int32_t S,
                  double *__restrict__ P)
{
    const size_t M = (size_t)F * S;
    const size_t cell = (size_t)blockIdx.x * WMI_WG + threadIdx.x;
    if (cell >= M * M)
        return;
    double sum = part[cell];
    for (int32_t c = 1; c < chunks; ++c)
        sum = sum + part[(size_t)c * M * M + cell];
    const size_t r = cell / M, col = cell % M;
    const size_t i = r / S, u = r % S, j = col / S, v = col % S;
    P[((i * F + j) * S + u) * S + v] = sum;
}

// mutual_info.py:155-168: P / (P_x P_y) where P_x P_y != 0, its log where that is not 0,
// times P; the terms of a pair added u outer, v inner
__global__ void __launch_bounds__(WMI_WG)
wmi_info_kernel(const double *__restrict__ P, int32_t F, int32_t S, double *__restrict__ mi)
{
    const int64_t p = (int64_t)blockIdx.x * WMI_WG + threadIdx.x;
    if (p >= (int64_t)F * F)
        return;
    const size_t i = (size_t)(p / F), j = (size_t)(p % F), s = (size_t)S;
    const double *pij = P + (size_t)p * s * s;
    const double *pii = P + (i * F + i) * s * s, *pjj = P + (j * F + j) * s * s;
    double acc = 0.0;
    for (size_t u = 0; u < s; ++u) {
        const double px = pii[u * s + u];
        for (size_t v = 0; v < s; ++v) {
            const double pm = px * pjj[v * s + v];
            const double pxy = pij[u * s + v];
            if (pm == 0.0 || pxy == 0.0)
                continue;
            acc = acc + pxy * log(pxy / pm);
        }
    }
    mi[p] = acc;
}

extern "C" int ek_wmi_run(int device, const uint8_t *codes, const double *weights,
                          int64_t frames, int32_t F, int32_t S, double *P_out, double *mi_out)
{
    int rc = EK_OK;
    if (!codes || !weights || frames < 1 || frames >= ((int64_t)1 << 31) - 64 ||
        (!P_out && !mi_out))
        return ek_set_error(EK_EARG, "ek_wmi_run: bad argument (1 <= frames < 2^31 - 64, an "
                                     "output)");
    rc = ek_mi_check_shape(F, F, S, S, "ek_wmi_run");
    if (rc != EK_OK)
        return rc;
    if ((int64_t)F * S > 65535 * (int64_t)WMI_BLOCK)
        return ek_set_error(EK_EARG, "ek_wmi_run: features x states is too large");
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess)
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
    }
    const int64_t tpad = ek_mi_tpad(frames);
    const int64_t chunk = wmi_chunk(frames);
    const int32_t chunks = (int32_t)((tpad + chunk - 1) / chunk);
    const int32_t M = F * S;
    const size_t cells = (size_t)M * M;
    const size_t raw_b = (size_t)frames * F, code_b = (size_t)F * tpad;
    const size_t w_b = (size_t)tpad * sizeof(double);
    const size_t part_b = (size_t)chunks * cells * sizeof(double), P_b = cells * sizeof(double);
    const size_t mi_b = (size_t)F * F * sizeof(double);
    rc = ek_mi_check_memory(raw_b + code_b + w_b + part_b + P_b + mi_b, "ek_wmi_run");
    if (rc != EK_OK)
        return rc;

    uint8_t *d_raw = nullptr, *d_codes = nullptr;
    double *d_w = nullptr, *d_part = nullptr, *d_P = nullptr, *d_mi = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float ms = 0.f;
    const unsigned blocks = (unsigned)((M + WMI_BLOCK - 1) / WMI_BLOCK);
    WMI_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    for (hipEvent_t &e : ev)
        WMI_HIP(ek_event_create(&e));
    WMI_HIP(ek_dev_malloc((void **)&d_raw, raw_b));
    WMI_HIP(ek_dev_malloc((void **)&d_codes, code_b));
    WMI_HIP(ek_dev_malloc((void **)&d_w, w_b));
    WMI_HIP(ek_dev_malloc((void **)&d_part, part_b));
    WMI_HIP(ek_dev_malloc((void **)&d_P, P_b));
    WMI_HIP(ek_dev_malloc((void **)&d_mi, mi_b));
    WMI_HIP(hipEventRecord(ev[0], s));
    WMI_HIP(hipMemcpyAsync(d_raw, codes, raw_b, hipMemcpyHostToDevice, s));
    WMI_HIP(hipMemsetAsync(d_w, 0, w_b, s));
    WMI_HIP(hipMemcpyAsync(d_w, weights, (size_t)frames * sizeof(double), hipMemcpyHostToDevice,
                           s));
    ek_mi_launch_pack(d_raw, frames, F, tpad, d_codes, s);
    WMI_HIP(hipEventRecord(ev[1], s));
    hipLaunchKernelGGL(wmi_product_kernel, dim3(blocks, blocks, (unsigned)chunks), dim3(WMI_WG),
                       0, s, d_codes, d_w, tpad, chunk, S, M, d_part);
    WMI_HIP(hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(wmi_reduce_kernel, dim3((unsigned)((cells + WMI_WG - 1) / WMI_WG)),
                       dim3(WMI_WG), 0, s, d_part, chunks, F, S, d_P);
    WMI_HIP(hipEventRecord(ev[3], s));
    if (mi_out)
        hipLaunchKernelGGL(wmi_info_kernel,
                           dim3((unsigned)(((size_t)F * F + WMI_WG - 1) / WMI_WG)), dim3(WMI_WG),
                           0, s, d_P, F, S, d_mi);
    WMI_HIP(hipEventRecord(ev[4], s));
    WMI_HIP(hipGetLastError());
    if (P_out)
        WMI_HIP(hipMemcpyAsync(P_out, d_P, P_b, hipMemcpyDeviceToHost, s));
    if (mi_out)
        WMI_HIP(hipMemcpyAsync(mi_out, d_mi, mi_b, hipMemcpyDeviceToHost, s));
    WMI_HIP(hipStreamSynchronize(s));
    for (int q = 0; q < 4; ++q) {
        WMI_HIP(hipEventElapsedTime(&ms, ev[q], ev[q + 1]));
        wmi_ms[q] = ms;
    }
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_raw);
    (void)ek_dev_free(d_codes);
    (void)ek_dev_free(d_w);
    (void)ek_dev_free(d_part);
    (void)ek_dev_free(d_P);
    (void)ek_dev_free(d_mi);
    for (hipEvent_t e : ev)
        if (e)
            (void)ek_event_destroy(e);
    if (s)
        (void)ek_stream_destroy(s);
    return rc;
}

extern "C" int ek_wmi_last_timing(double *ms_out)
{
    if (!ms_out)
        return ek_set_error(EK_EARG, "ek_wmi_last_timing: null argument");
    for (int i = 0; i < 4; ++i)
        ms_out[i] = wmi_ms[i];
    return EK_OK;
}
