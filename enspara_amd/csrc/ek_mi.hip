// ek_mi.hip -- joint counts and mutual information of discrete features on the
// device.
//
// Replaces the reference's enspara/info_theory/libinfo.pyx (matrix_bincount2d
// :50-74, bincount2d :30-45) and the arithmetic of mutual_info.mutual_information
// (mutual_info.py:290-327).
//
//   jc[i][j][u][v] = sum over frames t of [X[t][i] == u] [Y[t][j] == v]
//
// is the product OneHot(X)^T OneHot(Y) of two 0/1 byte matrices with
// (Fx n_x) rows, (Fy n_y) columns and the frames as the summed index: exact
// integers on v_mfma_i32_16x16x64_i8.  No one-hot array exists in memory:
//   pack     the uploaded codes [frames][F] uint8 -> feature-major [F][frames
//            padded to 64 with MI_PAD], so that 16 consecutive frames of one
//            feature are one 16-byte load
//   count    a workgroup owns 128 rows x 128 columns and one chunk of MI_CHUNK
//            frames, each of its four waves 4 x 4 tiles of 16 x 16; row r of the
//            product is (feature r / n_x, state r % n_x), so a lane makes operand
//            bytes by comparing the 16 codes it loaded with its row's state; the
//            fragments are shared through the LDS, each serves 8 MFMAs; the partial
//            tile goes into jc with atomicAdd (integers: any order, any split gives
//            the same counts)
//   info     one lane per feature pair, float64, the reference's operations in
//            the reference's order
// Operand lane map: lane l holds row (A) / column (B) l & 15 of the tile and 16
// of the 64 summed indices.  WHICH 16 does not matter here: A and B take the same
// frames in the same lane group and byte, and the sum over frames has no order.
// C/D: column l & 15, row 4 (l >> 4) + register.
#include "ek_common.h"
#include "ek_mi_launch.h"

#include <new>

extern int ek_set_error(int code, const char *fmt, ...);

#define MI_HIP(call)                                                           \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define MI_WG 256
#define MI_TW 4                 // tiles of 16 per wave and side
// (MI_BLOCK, MI_CHUNK, MI_PAD and the limits: ek_mi_launch.h)

typedef int mi_v4i __attribute__((ext_vector_type(4)));

struct ek_mi {
    int device;
    int32_t fx, fy, nx, ny;
    size_t cells;               // fx fy nx ny
    uint64_t n_obs;             // frames counted so far
    uint32_t *jc;               // [fx][fy][nx][ny] on the device
    hipStream_t s;
    hipEvent_t ev[4];           // add: start, packed, counted; information: with ev[0]
    double ms[3];               // upload + pack, count, information (the last of each)
};

// ---- pack --------------------------------------------------------------------------------
// in [frames][F] -> out [F][tpad], MI_PAD behind the last frame; a workgroup turns a
// tile of 64 frames x 64 features over in the LDS
__global__ void __launch_bounds__(MI_WG)
mi_pack_kernel(const uint8_t *__restrict__ in, int64_t frames, int32_t F, int64_t tpad,
               uint8_t *__restrict__ out)
{
    __shared__ uint8_t tile[64][65];
    const int64_t t0 = (int64_t)blockIdx.x * 64;
    const int32_t f0 = (int32_t)blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += MI_WG / 64) {
        const int64_t t = t0 + i;
        const int32_t f = f0 + tx;
        tile[i][tx] = (t < frames && f < F) ? in[(size_t)t * F + f] : (uint8_t)MI_PAD;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += MI_WG / 64) {
        const int32_t f = f0 + i;
        if (f < F)      // (t0 + tx < tpad: tpad is a multiple of 64)
            out[(size_t)f * tpad + t0 + tx] = tile[tx][i];
    }
}

// ---- count -------------------------------------------------------------------------------
// the four bytes of w that equal the byte repeated in pat -> 0x01, the others 0x00
// (x | 0x80) - 1 borrows from no neighbouring byte and has bit 7 clear only where the
// low seven bits of x are zero
__device__ __forceinline__ uint32_t mi_eq_bytes(uint32_t w, uint32_t pat)
{
    const uint32_t x = w ^ pat;
    const uint32_t t = ((x | 0x80808080u) - 0x01010101u) | x;
    return (~t & 0x80808080u) >> 7;
}

__device__ __forceinline__ mi_v4i mi_onehot(uint4 w, uint32_t pat)
{
    mi_v4i o;
    o.x = (int)mi_eq_bytes(w.x, pat);
    o.y = (int)mi_eq_bytes(w.y, pat);
    o.z = (int)mi_eq_bytes(w.z, pat);
    o.w = (int)mi_eq_bytes(w.w, pat);
    return o;
}

// grid: x column blocks, y row blocks, z frame chunks (chunk0 + z).  A workgroup owns 128
// rows x 128 columns (8 A and 8 B fragments per 64 frames) and one chunk; wave w makes the
// A and B fragments 2w, 2w + 1 from the codes it loaded a step ahead, puts them into the
// LDS lane-linear (16-byte writes and reads without bank conflicts) and reads the 4 + 4
// its own 4 x 4 tiles need: 4 fragments made per 16 MFMAs.  Two buffers, one barrier per
// step: a wave writes buffer k & 1 of step k only after the barrier of step k - 1, behind
// which every wave has read step k - 2.  Rows and columns past the product's edge read the
// last one and are not written.  (The second launch bound keeps the 64 accumulator
// registers in the one file the operands are in: without it the compiler splits them off
// and moves 84 registers per step between the two.)
__global__ void __launch_bounds__(MI_WG, 2)
mi_count_kernel(const uint8_t *__restrict__ cx, const uint8_t *__restrict__ cy, int64_t tpad,
                int32_t fy, int32_t nx, int32_t ny, int32_t M, int32_t N, int64_t chunk0,
                uint32_t *__restrict__ jc)
{
    __shared__ mi_v4i frag[2][16][64];      // [buffer][A tiles 0 .. 7, B tiles 0 .. 7][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t R0 = (int32_t)blockIdx.y * MI_BLOCK, C0 = (int32_t)blockIdx.x * MI_BLOCK;
    const int32_t r0 = R0 + (wave >> 1) * (16 * MI_TW), c0 = C0 + (wave & 1) * (16 * MI_TW);
    const int64_t t0 = (chunk0 + blockIdx.z) * MI_CHUNK;
    const int64_t t1 = (t0 + MI_CHUNK < tpad) ? t0 + MI_CHUNK : tpad;
    const int g = lane >> 4, l = lane & 15;

    // the fragments this wave makes: A tiles and B tiles 2 wave, 2 wave + 1 of the block
    const uint8_t *pa[2], *pb[2];
    uint32_t ua[2], ub[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int32_t r = R0 + 16 * (2 * wave + q) + l;
        r = (r < M) ? r : M - 1;
        pa[q] = cx + (size_t)(r / nx) * tpad + 16 * g;
        ua[q] = (uint32_t)(r % nx) * 0x01010101u;
        int32_t c = C0 + 16 * (2 * wave + q) + l;
        c = (c < N) ? c : N - 1;
        pb[q] = cy + (size_t)(c / ny) * tpad + 16 * g;
        ub[q] = (uint32_t)(c % ny) * 0x01010101u;
    }
    mi_v4i acc[MI_TW][MI_TW];
#pragma unroll
    for (int m = 0; m < MI_TW; ++m)
#pragma unroll
        for (int n = 0; n < MI_TW; ++n)
            acc[m][n] = mi_v4i{0, 0, 0, 0};

    uint4 wa[2], wb[2];     // the codes of the next step, loaded a step ahead
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        wa[q] = *reinterpret_cast<const uint4 *>(pa[q] + t0);
        wb[q] = *reinterpret_cast<const uint4 *>(pb[q] + t0);
    }
    int buf = 0;
    for (int64_t t = t0; t < t1; t += 64, buf ^= 1) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            frag[buf][2 * wave + q][lane] = mi_onehot(wa[q], ua[q]);
            frag[buf][8 + 2 * wave + q][lane] = mi_onehot(wb[q], ub[q]);
        }
        const int64_t tn = (t + 64 < t1) ? t + 64 : t;      // (the last step loads its own again)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            wa[q] = *reinterpret_cast<const uint4 *>(pa[q] + tn);
            wb[q] = *reinterpret_cast<const uint4 *>(pb[q] + tn);
        }
        __syncthreads();
        mi_v4i a[MI_TW], b[MI_TW];
#pragma unroll
        for (int m = 0; m < MI_TW; ++m) {
            a[m] = frag[buf][MI_TW * (wave >> 1) + m][lane];
            b[m] = frag[buf][8 + MI_TW * (wave & 1) + m][lane];
        }
#pragma unroll
        for (int m = 0; m < MI_TW; ++m)
#pragma unroll
            for (int n = 0; n < MI_TW; ++n)
                acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], b[n], acc[m][n], 0, 0, 0);
    }

    if (r0 >= M || c0 >= N)
        return;
#pragma unroll
    for (int m = 0; m < MI_TW; ++m)
#pragma unroll
        for (int n = 0; n < MI_TW; ++n) {
            const int32_t c = c0 + 16 * n + l;
            if (c >= N)
                continue;
            const size_t j = (size_t)(c / ny), v = (size_t)(c % ny);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int32_t r = r0 + 16 * m + 4 * g + k;
                const int cnt = acc[m][n][k];
                if (r < M && cnt != 0) {
                    const size_t i = (size_t)(r / nx), u = (size_t)(r % nx);
                    atomicAdd(&jc[((i * fy + j) * nx + u) * ny + v], (uint32_t)cnt);
                }
            }
        }
}

// ---- information ---------------------------------------------------------------------------
// one lane per feature pair; col [pairs][ny] scratch for the pair's column sums.
// mutual_info.py:290-327: marginals as exact integer sums, P = count / n_obs in float64,
// terms with a zero P skipped, P_xy * log(P_xy / (P_x * P_y)) added u outer, v inner.
// A pair without observations gives 0 (the reference divides by nothing there and
// reads memory it never wrote).
__global__ void __launch_bounds__(MI_WG)
mi_info_kernel(const uint32_t *__restrict__ jc, int64_t pairs, int32_t nx, int32_t ny,
               uint32_t *__restrict__ col, double *__restrict__ mi)
{
    const int64_t p = (int64_t)blockIdx.x * MI_WG + threadIdx.x;
    if (p >= pairs)
        return;
    const uint32_t *c = jc + (size_t)p * nx * ny;
    uint32_t *cs = col + (size_t)p * ny;
    unsigned long long n_obs = 0;
    for (int32_t v = 0; v < ny; ++v)
        cs[v] = 0;
    for (int32_t u = 0; u < nx; ++u)
        for (int32_t v = 0; v < ny; ++v) {
            const uint32_t x = c[(size_t)u * ny + v];
            cs[v] += x;
            n_obs += x;
        }
    double acc = 0.0;
    if (n_obs != 0) {
        const double dn = (double)n_obs;
        for (int32_t u = 0; u < nx; ++u) {
            unsigned long long row = 0;
            for (int32_t v = 0; v < ny; ++v)
                row += c[(size_t)u * ny + v];
            if (row == 0)
                continue;
            const double px = (double)row / dn;
            for (int32_t v = 0; v < ny; ++v) {
                const uint32_t x = c[(size_t)u * ny + v];
                if (x == 0 || cs[v] == 0)
                    continue;
                const double pxy = (double)x / dn;
                const double py = (double)cs[v] / dn;
                acc = acc + pxy * log(pxy / (px * py));
            }
        }
    }
    mi[p] = acc;
}

// ---- launches (ek_mi_launch.h) -----------------------------------------------------------------
void ek_mi_launch_pack(const uint8_t *in, int64_t frames, int32_t F, int64_t tpad, uint8_t *out,
                       hipStream_t s)
{
    hipLaunchKernelGGL(mi_pack_kernel, dim3((unsigned)(tpad / 64), (F + 63) / 64), dim3(MI_WG),
                       0, s, in, frames, F, tpad, out);
}

void ek_mi_launch_count(const uint8_t *cx, const uint8_t *cy, int64_t tpad, int32_t fx,
                        int32_t fy, int32_t nx, int32_t ny, uint32_t *jc, hipStream_t s)
{
    const int32_t M = fx * nx, N = fy * ny;
    const int64_t chunks = (tpad + MI_CHUNK - 1) / MI_CHUNK;
    for (int64_t z0 = 0; z0 < chunks; z0 += MI_MAX_GRID_Z) {
        const int64_t nz = (chunks - z0 < MI_MAX_GRID_Z) ? chunks - z0 : MI_MAX_GRID_Z;
        hipLaunchKernelGGL(mi_count_kernel,
                           dim3((N + MI_BLOCK - 1) / MI_BLOCK, (M + MI_BLOCK - 1) / MI_BLOCK,
                                (unsigned)nz),
                           dim3(MI_WG), 0, s, cx, cy, tpad, fy, nx, ny, M, N, z0, jc);
    }
}

void ek_mi_launch_info(const uint32_t *jc, int64_t pairs, int32_t nx, int32_t ny, uint32_t *col,
                       double *mi, hipStream_t s)
{
    hipLaunchKernelGGL(mi_info_kernel, dim3((unsigned)((pairs + MI_WG - 1) / MI_WG)),
                       dim3(MI_WG), 0, s, jc, pairs, nx, ny, col, mi);
}

// ---- host ------------------------------------------------------------------------------------
int ek_mi_check_memory(size_t bytes, const char *who)
{
    size_t free_b = 0, total_b = 0;
    hipError_t e = hipMemGetInfo(&free_b, &total_b);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "%s: hipMemGetInfo: %s", who, hipGetErrorString(e));
    const size_t slack = (size_t)256 << 20;
    if (bytes + slack > free_b)
        return ek_set_error(EK_ENOMEM, "%s: %zu MiB of device memory are needed, %zu MiB are "
                                       "free", who, bytes >> 20, free_b >> 20);
    return EK_OK;
}

int ek_mi_check_shape(int32_t fx, int32_t fy, int32_t nx, int32_t ny, const char *who)
{
    if (fx < 1 || fy < 1 || nx < 1 || ny < 1 || nx > MI_MAX_STATES || ny > MI_MAX_STATES)
        return ek_set_error(EK_EARG, "%s: bad argument (features >= 1, 1 <= states <= %d)",
                            who, MI_MAX_STATES);
    if (fx > MI_MAX_FEATURES || fy > MI_MAX_FEATURES)
        return ek_set_error(EK_EARG, "%s: at most %d features a side", who, MI_MAX_FEATURES);
    if ((int64_t)fx * nx > INT32_MAX - MI_BLOCK || (int64_t)fy * ny > INT32_MAX - MI_BLOCK ||
        ((int64_t)fx * nx + MI_BLOCK - 1) / MI_BLOCK > MI_MAX_GRID_Z)
        return ek_set_error(EK_EARG, "%s: features x states is too large", who);
    return EK_OK;
}

static int mi_bind(ek_mi *h, const char *who)
{
    if (!h)
        return ek_set_error(EK_EARG, "%s: null handle", who);
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", h->device, hipGetErrorString(e));
    return EK_OK;
}

extern "C" int ek_mi_close(ek_mi *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(h->jc);
    for (hipEvent_t e : h->ev)
        if (e)
            (void)ek_event_destroy(e);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    delete h;
    return EK_OK;
}

extern "C" int ek_mi_open(int device, int32_t fx, int32_t fy, int32_t nx, int32_t ny,
                          ek_mi **out)
{
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "ek_mi_open: null output");
    *out = nullptr;
    rc = ek_mi_check_shape(fx, fy, nx, ny, "ek_mi_open");
    if (rc != EK_OK)
        return rc;
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess)
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device,
                                hipGetErrorString(e0));
    }
    ek_mi *h = new (std::nothrow) ek_mi();
    if (!h)
        return ek_set_error(EK_ENOMEM, "ek_mi_open: out of host memory");
    h->device = device;
    h->fx = fx;
    h->fy = fy;
    h->nx = nx;
    h->ny = ny;
    h->cells = (size_t)fx * fy * nx * ny;
    rc = ek_mi_check_memory(h->cells * sizeof(uint32_t), "ek_mi_open");
    if (rc != EK_OK)
        goto done;
    MI_HIP(ek_stream_create_flags(&h->s, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev)
        MI_HIP(ek_event_create(&e));
    MI_HIP(ek_dev_malloc((void **)&h->jc, h->cells * sizeof(uint32_t)));
    MI_HIP(hipMemsetAsync(h->jc, 0, h->cells * sizeof(uint32_t), h->s));
    MI_HIP(hipStreamSynchronize(h->s));
    *out = h;
    return EK_OK;
done:
    ek_mi_close(h);
    return rc;
}

extern "C" int ek_mi_add(ek_mi *h, const uint8_t *X, const uint8_t *Y, int64_t frames)
{
    int rc = mi_bind(h, "ek_mi_add");
    if (rc != EK_OK)
        return rc;
    if (!X || frames < 0 || frames >= ((int64_t)1 << 31) - 64)
        return ek_set_error(EK_EARG, "ek_mi_add: bad argument (0 <= frames < 2^31 - 64)");
    if (!Y && (h->fx != h->fy || h->nx != h->ny))
        return ek_set_error(EK_EARG, "ek_mi_add: X against itself needs a square handle");
    if (h->n_obs + (uint64_t)frames >= ((uint64_t)1 << 32))
        return ek_set_error(EK_EARG, "ek_mi_add: %llu + %lld observations do not fit the "
                                     "counts (2^32)", (unsigned long long)h->n_obs,
                            (long long)frames);
    if (frames == 0)
        return EK_OK;

    const int64_t tpad = ek_mi_tpad(frames);
    const int32_t fmax = h->fx > h->fy ? h->fx : h->fy;
    const size_t raw_b = (size_t)frames * fmax;
    const size_t cx_b = (size_t)h->fx * tpad, cy_b = Y ? (size_t)h->fy * tpad : 0;
    uint8_t *d_raw = nullptr, *d_cx = nullptr, *d_cy = nullptr;
    float ms = 0.f;

    rc = ek_mi_check_memory(raw_b + cx_b + cy_b, "ek_mi_add");
    if (rc != EK_OK)
        return rc;
    MI_HIP(ek_dev_malloc((void **)&d_raw, raw_b));
    MI_HIP(ek_dev_malloc((void **)&d_cx, cx_b));
    if (Y)
        MI_HIP(ek_dev_malloc((void **)&d_cy, cy_b));
    MI_HIP(hipEventRecord(h->ev[0], h->s));
    MI_HIP(hipMemcpyAsync(d_raw, X, (size_t)frames * h->fx, hipMemcpyHostToDevice, h->s));
    ek_mi_launch_pack(d_raw, frames, h->fx, tpad, d_cx, h->s);
    if (Y) {
        MI_HIP(hipMemcpyAsync(d_raw, Y, (size_t)frames * h->fy, hipMemcpyHostToDevice, h->s));
        ek_mi_launch_pack(d_raw, frames, h->fy, tpad, d_cy, h->s);
    }
    MI_HIP(hipEventRecord(h->ev[1], h->s));
    ek_mi_launch_count(d_cx, Y ? d_cy : d_cx, tpad, h->fx, h->fy, h->nx, h->ny, h->jc, h->s);
    MI_HIP(hipEventRecord(h->ev[2], h->s));
    MI_HIP(hipGetLastError());
    MI_HIP(hipStreamSynchronize(h->s));
    h->n_obs += (uint64_t)frames;
    MI_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms[0] = ms;
    MI_HIP(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
    h->ms[1] = ms;
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_raw);
    (void)ek_dev_free(d_cx);
    (void)ek_dev_free(d_cy);
    return rc;
}

extern "C" int ek_mi_load_counts(ek_mi *h, const uint32_t *jc, uint64_t n_obs)
{
    int rc = mi_bind(h, "ek_mi_load_counts");
    if (rc != EK_OK)
        return rc;
    if (!jc || n_obs >= ((uint64_t)1 << 32))
        return ek_set_error(EK_EARG, "ek_mi_load_counts: null counts, or 2^32 observations "
                                     "or more");
    MI_HIP(hipMemcpyAsync(h->jc, jc, h->cells * sizeof(uint32_t), hipMemcpyHostToDevice,
                          h->s));
    MI_HIP(hipStreamSynchronize(h->s));
    h->n_obs = n_obs;   // (the fullest pair, the caller's word: what ek_mi_add adds to)
done:
    return rc;
}

extern "C" int ek_mi_counts(ek_mi *h, uint32_t *jc_out)
{
    int rc = mi_bind(h, "ek_mi_counts");
    if (rc != EK_OK)
        return rc;
    if (!jc_out)
        return ek_set_error(EK_EARG, "ek_mi_counts: null output");
    MI_HIP(hipMemcpyAsync(jc_out, h->jc, h->cells * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          h->s));
    MI_HIP(hipStreamSynchronize(h->s));
done:
    return rc;
}

extern "C" int ek_mi_information(ek_mi *h, double *mi_out)
{
    int rc = mi_bind(h, "ek_mi_information");
    if (rc != EK_OK)
        return rc;
    if (!mi_out)
        return ek_set_error(EK_EARG, "ek_mi_information: null output");
    const int64_t pairs = (int64_t)h->fx * h->fy;
    uint32_t *d_col = nullptr;
    double *d_mi = nullptr;
    float ms = 0.f;
    rc = ek_mi_check_memory((size_t)pairs * (h->ny * sizeof(uint32_t) + sizeof(double)),
                         "ek_mi_information");
    if (rc != EK_OK)
        return rc;
    MI_HIP(ek_dev_malloc((void **)&d_col, (size_t)pairs * h->ny * sizeof(uint32_t)));
    MI_HIP(ek_dev_malloc((void **)&d_mi, (size_t)pairs * sizeof(double)));
    MI_HIP(hipEventRecord(h->ev[0], h->s));
    ek_mi_launch_info(h->jc, pairs, h->nx, h->ny, d_col, d_mi, h->s);
    MI_HIP(hipEventRecord(h->ev[3], h->s));
    MI_HIP(hipGetLastError());
    MI_HIP(hipMemcpyAsync(mi_out, d_mi, (size_t)pairs * sizeof(double), hipMemcpyDeviceToHost,
                          h->s));
    MI_HIP(hipStreamSynchronize(h->s));
    MI_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[3]));
    h->ms[2] = ms;
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_col);
    (void)ek_dev_free(d_mi);
    return rc;
}

extern "C" int ek_mi_last_timing(ek_mi *h, double *ms_out)
{
    if (!h || !ms_out)
        return ek_set_error(EK_EARG, "ek_mi_last_timing: null argument");
    for (int i = 0; i < 3; ++i)
        ms_out[i] = h->ms[i];
    return EK_OK;
}
