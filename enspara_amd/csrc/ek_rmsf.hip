// ek_rmsf.hip -- superposition on a reference structure and the weighted sums of
// squared deviations behind an RMSF, on the device.
//
// Replaces the reference's enspara/geometry/rmsf.py (md.Trajectory.superpose, the
// population-weighted mean square deviation per atom, its mean per residue).  The
// contract is DESIGN.md 4o; tests/_numpy_rmsf.py restates step 3 operation for
// operation.
//
// One workgroup owns one TILE of RMSF_TILE frames (absolute frame indices: tile k is
// frames [32 k, 32 k + 32) of everything the handle has seen) and walks it frame by
// frame, its lanes across the atoms:
//   0. the frame into LDS, one coalesced read (atoms <= RMSF_LDS_ATOMS; beyond, the
//      steps below read global memory: the selection twice more, every atom once);
//   1. FIT.  centroid of the selection: per lane the float64 sum of its atoms k = lane,
//      lane + T, .. in that order, then a fixed butterfly over the lanes and (T = 256)
//      the four waves in order; the centred coordinates rounded to float32; S and Gx
//      as float64 sums of the exact products, same tree, S then rounded to float32;
//      lambda by ek_msd_lambda_from_S.  (Not ek_prepare.hip's one-lane-per-frame
//      sequential sum: with a workgroup per frame that is a serial chain of n_sel
//      dependent float64 adds.  The tree depends on the atom counts alone.)
//   2. ROTATION.  ek_superpose_from_S, in every lane (they all hold the same sums).
//   3. APPLY.  aligned = float32(fma(R_i2, z, fma(R_i1, y, R_i0 * x)) + c_ref,i), (x, y,
//      z) = float64(coordinate) - centroid; d^2 = (dx * dx + dy * dy) + dz * dz from
//      float64(aligned) - float64(reference), nothing fused; acc_a = acc_a + w_f * d^2,
//      frames of the tile in order, starting from 0.0 -- or from the carried partial
//      where an earlier launch ended inside the tile.  The accumulators live in LDS
//      (or, beyond RMSF_LDS_ATOMS, in the tile's row of the partials, read and
//      written by the one lane that owns the atom).
// A second kernel adds the complete tiles' partials to the totals, tile by tile in
// order, and keeps an incomplete last tile as the carry.  No atomics anywhere: the
// bits depend on the frames and their absolute indices alone.
//
// T = 64 (one wave per tile) up to RMSF_WAVE_ATOMS atoms, 256 beyond: chosen by
// tools/rmsf_timing.py's shapes ("Measured").
#include "ek_common.h"
#include "ek_qcp.h"
#include "ek_superpose.h"

#include <math.h>
#include <new>
#include <string.h>

extern int ek_set_error(int code, const char *fmt, ...);
int ek_mi_check_memory(size_t bytes, const char *who);

#define RMSF_HIP(call)                                                         \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define RMSF_TILE 32                // frames per partial (geometry.rmsf.TILE)
#define RMSF_LDS_ATOMS 3072         // frame + accumulators in LDS: 20 B per atom (geometry.rmsf.LDS_ATOMS)
#define RMSF_WAVE_ATOMS 512         // one wave per tile up to here (geometry.rmsf.WAVE_ATOMS)
#define RMSF_NRED 10                // S (9) and Gx
#define RMSF_MAX_CHUNK ((int64_t)1 << 24)

struct ek_rmsf {
    int device;
    int32_t atoms, n_sel, n_groups, n_idx;
    int32_t *sel;               // [n_sel]
    float *yc;                  // [n_sel][3] the reference's selection, centred, float32
    float *ref;                 // [atoms][3]
    double Gy, cref[3];
    double *total, *carry;      // [atoms]
    int32_t *goff, *gidx;       // host copies of the groups
    int64_t n_seen;             // frames of all runs so far
    hipStream_t s;
    hipEvent_t ev[4];
    double ms[3];               // upload, kernels, download: the last run's sums
};

struct RmsfArgs {
    const float *xyz;           // [nf][atoms][3]
    const double *w;            // [nf] or null: no sums
    int64_t nf, f_abs0, ref_local;
    int32_t atoms, n_sel;
    const int32_t *sel;
    const float *yc, *ref;
    double Gy, cref[3];
    float *aligned;             // [nf][atoms][3] or null
    double *rot;                // [nf][9] or null
    float *rmsd;                // [nf] or null
    uint32_t *flags;            // [nf]
    double *partial;            // [tiles of the launch][atoms]
    const double *carry;        // [atoms]: where the first tile starts from, if inside it
};

// every lane leaves with the sum of all T lanes' v[0 .. N): xor butterfly over the
// wave (a + b == b + a, so the lanes agree bit for bit), then the waves in order
template <int T, int N>
__device__ __forceinline__ void rmsf_reduce(double (&v)[N], double *scratch)
{
#pragma unroll
    for (int off = 1; off < EK_WAVE; off <<= 1)
#pragma unroll
        for (int j = 0; j < N; ++j)
            v[j] = v[j] + __shfl_xor(v[j], off);
    if (T > EK_WAVE) {
        const int lane = threadIdx.x & (EK_WAVE - 1), wave = threadIdx.x / EK_WAVE;
        if (lane == 0)
#pragma unroll
            for (int j = 0; j < N; ++j)
                scratch[wave * N + j] = v[j];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < N; ++j) {
            double s = scratch[j];
            for (int w = 1; w < T / EK_WAVE; ++w)
                s = s + scratch[w * N + j];
            v[j] = s;
        }
        __syncthreads();        // the scratch is free again
    }
}

template <int T, bool LDSF>
__global__ void __launch_bounds__(T) rmsf_tile_kernel(const RmsfArgs a)
{
    extern __shared__ double smem[];
    const int tid = threadIdx.x, A = a.atoms, nsel = a.n_sel;
    // LDS: [accumulators: A doubles, LDSF only][scratch: 4 * RMSF_NRED doubles][frame: 3 A floats, LDSF only]
    double *scratch = smem + (LDSF ? A : 0);
    float *fr = (float *)(scratch + (T / EK_WAVE) * RMSF_NRED);
    double *acc = LDSF ? smem : a.partial + (size_t)blockIdx.x * A;

    const int64_t tile = a.f_abs0 / RMSF_TILE + blockIdx.x;
    int64_t lo = tile * RMSF_TILE - a.f_abs0, hi = lo + RMSF_TILE;
    const bool resumed = lo < 0;        // an earlier launch ended inside this tile
    lo = resumed ? 0 : lo;
    hi = (hi > a.nf) ? a.nf : hi;
    if (a.w)
        for (int i = tid; i < A; i += T)
            acc[i] = resumed ? a.carry[i] : 0.0;

    for (int64_t f = lo; f < hi; ++f) {
        const float *X = a.xyz + (size_t)f * 3 * (size_t)A;
        if (LDSF) {
            __syncthreads();    // the last frame's readers are done
#pragma unroll 4
            for (int i = tid; i < 3 * A; i += T)
                fr[i] = X[i];
            __syncthreads();
        }
        const float *P = LDSF ? fr : X;
        double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
        double c[3] = {0.0, 0.0, 0.0}, cr[3] = {0.0, 0.0, 0.0};
        const bool is_ref = (f == a.ref_local);     // its own bits, deviation exactly 0
        if (!is_ref) {
            for (int k = tid; k < nsel; k += T) {
                const float *p = P + 3 * (size_t)a.sel[k];
                c[0] = c[0] + (double)p[0];
                c[1] = c[1] + (double)p[1];
                c[2] = c[2] + (double)p[2];
            }
            rmsf_reduce<T, 3>(c, scratch);
            c[0] = c[0] / (double)nsel;
            c[1] = c[1] / (double)nsel;
            c[2] = c[2] / (double)nsel;
            double v[RMSF_NRED];
#pragma unroll
            for (int j = 0; j < RMSF_NRED; ++j)
                v[j] = 0.0;
            for (int k = tid; k < nsel; k += T) {
                const float *p = P + 3 * (size_t)a.sel[k];
                const float *y = a.yc + 3 * (size_t)k;
                const double x0 = (double)(float)((double)p[0] - c[0]);
                const double x1 = (double)(float)((double)p[1] - c[1]);
                const double x2 = (double)(float)((double)p[2] - c[2]);
                const double y0 = (double)y[0], y1 = (double)y[1], y2 = (double)y[2];
                v[0] = v[0] + x0 * y0;
                v[1] = v[1] + x0 * y1;
                v[2] = v[2] + x0 * y2;
                v[3] = v[3] + x1 * y0;
                v[4] = v[4] + x1 * y1;
                v[5] = v[5] + x1 * y2;
                v[6] = v[6] + x2 * y0;
                v[7] = v[7] + x2 * y1;
                v[8] = v[8] + x2 * y2;
                v[9] = v[9] + ((x0 * x0 + x1 * x1) + x2 * x2);
            }
            rmsf_reduce<T, RMSF_NRED>(v, scratch);
            float S[9];
#pragma unroll
            for (int j = 0; j < 9; ++j)
                S[j] = (float)v[j];
            double lam;
            const double msd = ek_msd_lambda_from_S(S, v[9], a.Gy, nsel, &lam);
            const int bad = ek_superpose_from_S(S, v[9], a.Gy, lam, R);
            cr[0] = a.cref[0];
            cr[1] = a.cref[1];
            cr[2] = a.cref[2];
            if (tid == 0) {
                a.flags[f] = (uint32_t)bad;
                if (a.rmsd)
                    a.rmsd[f] = __builtin_sqrtf((float)msd);
            }
        } else if (tid == 0) {
            a.flags[f] = 0u;
            if (a.rmsd)
                a.rmsd[f] = 0.0f;
        }
        if (a.rot && tid < 9)
            a.rot[(size_t)f * 9 + tid] = (tid == 0)   ? R[0]
                                         : (tid == 1) ? R[1]
                                         : (tid == 2) ? R[2]
                                         : (tid == 3) ? R[3]
                                         : (tid == 4) ? R[4]
                                         : (tid == 5) ? R[5]
                                         : (tid == 6) ? R[6]
                                         : (tid == 7) ? R[7]
                                                      : R[8];
        const double wf = a.w ? a.w[f] : 0.0;
        float *O = a.aligned ? a.aligned + (size_t)f * 3 * (size_t)A : nullptr;
        for (int i = tid; i < A; i += T) {
            const float p0 = P[3 * (size_t)i], p1 = P[3 * (size_t)i + 1], p2 = P[3 * (size_t)i + 2];
            float o0 = p0, o1 = p1, o2 = p2;
            if (!is_ref) {
                const double x = (double)p0 - c[0], y = (double)p1 - c[1], z = (double)p2 - c[2];
                o0 = (float)(__builtin_fma(R[2], z, __builtin_fma(R[1], y, R[0] * x)) + cr[0]);
                o1 = (float)(__builtin_fma(R[5], z, __builtin_fma(R[4], y, R[3] * x)) + cr[1]);
                o2 = (float)(__builtin_fma(R[8], z, __builtin_fma(R[7], y, R[6] * x)) + cr[2]);
            }
            if (O) {
                O[3 * (size_t)i] = o0;
                O[3 * (size_t)i + 1] = o1;
                O[3 * (size_t)i + 2] = o2;
            }
            if (a.w) {
                const float *q = a.ref + 3 * (size_t)i;
                const double dx = (double)o0 - (double)q[0];
                const double dy = (double)o1 - (double)q[1];
                const double dz = (double)o2 - (double)q[2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                acc[i] = acc[i] + wf * d2;
            }
        }
    }
    if (LDSF && a.w) {
        double *out = a.partial + (size_t)blockIdx.x * A;
        for (int i = tid; i < A; i += T)    // (each lane reads back what it wrote)
            out[i] = acc[i];
    }
}

// totals += the complete tiles' partials, in order; an incomplete last tile is the carry
__global__ void __launch_bounds__(EK_BLOCK)
rmsf_fold_kernel(const double *__restrict__ partial, int64_t n_tiles, int32_t last_complete,
                 int32_t atoms, double *__restrict__ total, double *__restrict__ carry)
{
    const int i = blockIdx.x * EK_BLOCK + threadIdx.x;
    if (i >= atoms)
        return;
    const int64_t n_full = last_complete ? n_tiles : n_tiles - 1;
    double t = total[i];
    for (int64_t k = 0; k < n_full; ++k)
        t = t + partial[(size_t)k * atoms + i];
    total[i] = t;
    if (!last_complete)
        carry[i] = partial[(size_t)(n_tiles - 1) * atoms + i];
}

static int rmsf_bind(ek_rmsf *h, const char *who)
{
    if (!h)
        return ek_set_error(EK_EARG, "%s: null handle", who);
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", h->device, hipGetErrorString(e));
    return EK_OK;
}

extern "C" int ek_rmsf_close(ek_rmsf *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(h->sel);
    (void)ek_dev_free(h->yc);
    (void)ek_dev_free(h->ref);
    (void)ek_dev_free(h->total);
    (void)ek_dev_free(h->carry);
    for (hipEvent_t e : h->ev)
        if (e)
            (void)ek_event_destroy(e);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    delete[] h->goff;
    delete[] h->gidx;
    delete h;
    return EK_OK;
}

extern "C" int ek_rmsf_open(int device, int32_t atoms, int32_t n_sel, const int32_t *sel,
                            const float *reference, int32_t n_groups,
                            const int32_t *group_offsets, const int32_t *group_atoms,
                            ek_rmsf **out)
{
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "ek_rmsf_open: null output");
    *out = nullptr;
    if (!sel || !reference || atoms < 3 || n_sel < 3 || n_sel > atoms || n_groups < 0 ||
        (n_groups > 0 && (!group_offsets || !group_atoms)))
        return ek_set_error(EK_EARG, "ek_rmsf_open: bad argument (3 <= n_sel <= atoms)");
    for (int32_t k = 0; k < n_sel; ++k)
        if (sel[k] < 0 || sel[k] >= atoms)
            return ek_set_error(EK_EARG, "ek_rmsf_open: selected atom %d is not in [0, %d)",
                                sel[k], atoms);
    for (size_t q = 0; q < 3 * (size_t)atoms; ++q)
        if (!isfinite(reference[q]))
            return ek_set_error(EK_EARG, "ek_rmsf_open: reference coordinate %zu is not finite", q);
    int32_t n_idx = 0;
    if (n_groups > 0) {
        if (group_offsets[0] != 0)
            return ek_set_error(EK_EARG, "ek_rmsf_open: group offsets start at 0");
        for (int32_t g = 0; g < n_groups; ++g)
            if (group_offsets[g + 1] <= group_offsets[g])
                return ek_set_error(EK_EARG, "ek_rmsf_open: group %d is empty", g);
        n_idx = group_offsets[n_groups];
        for (int32_t q = 0; q < n_idx; ++q)
            if (group_atoms[q] < 0 || group_atoms[q] >= atoms)
                return ek_set_error(EK_EARG, "ek_rmsf_open: group atom %d is not in [0, %d)",
                                    group_atoms[q], atoms);
    }
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess)
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
    }
    ek_rmsf *h = new (std::nothrow) ek_rmsf();
    float *yc = new (std::nothrow) float[3 * (size_t)n_sel];
    if (h) {
        h->goff = new (std::nothrow) int32_t[(size_t)n_groups + 1];
        h->gidx = new (std::nothrow) int32_t[(size_t)n_idx + 1];
    }
    if (!h || !yc || !h->goff || !h->gidx) {
        if (h) {
            delete[] h->goff;
            delete[] h->gidx;
        }
        delete h;
        delete[] yc;
        return ek_set_error(EK_ENOMEM, "ek_rmsf_open: out of host memory");
    }
    h->device = device;
    h->atoms = atoms;
    h->n_sel = n_sel;
    h->n_groups = n_groups;
    h->n_idx = n_idx;
    h->goff[0] = 0;
    if (n_groups > 0) {
        memcpy(h->goff, group_offsets, ((size_t)n_groups + 1) * sizeof(int32_t));
        memcpy(h->gidx, group_atoms, (size_t)n_idx * sizeof(int32_t));
    }
    {
        // the reference's selection: centroid as float64 sums in listed order, centred
        // coordinates rounded to float32, Gy the float64 sum of their exact squares
        double c[3] = {0.0, 0.0, 0.0};
        for (int32_t k = 0; k < n_sel; ++k)
            for (int d = 0; d < 3; ++d)
                c[d] = c[d] + (double)reference[3 * (size_t)sel[k] + d];
        double G = 0.0;
        for (int d = 0; d < 3; ++d)
            h->cref[d] = c[d] / (double)n_sel;
        for (int32_t k = 0; k < n_sel; ++k) {
            double y[3];
            for (int d = 0; d < 3; ++d) {
                yc[3 * (size_t)k + d] = (float)((double)reference[3 * (size_t)sel[k] + d] - h->cref[d]);
                y[d] = (double)yc[3 * (size_t)k + d];
            }
            G = G + ((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
        }
        h->Gy = G;
    }
    RMSF_HIP(ek_stream_create_flags(&h->s, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev)
        RMSF_HIP(ek_event_create(&e));
    RMSF_HIP(ek_dev_malloc((void **)&h->sel, (size_t)n_sel * sizeof(int32_t)));
    RMSF_HIP(ek_dev_malloc((void **)&h->yc, 3 * (size_t)n_sel * sizeof(float)));
    RMSF_HIP(ek_dev_malloc((void **)&h->ref, 3 * (size_t)atoms * sizeof(float)));
    RMSF_HIP(ek_dev_malloc((void **)&h->total, (size_t)atoms * sizeof(double)));
    RMSF_HIP(ek_dev_malloc((void **)&h->carry, (size_t)atoms * sizeof(double)));
    RMSF_HIP(hipMemcpyAsync(h->sel, sel, (size_t)n_sel * sizeof(int32_t), hipMemcpyHostToDevice,
                            h->s));
    RMSF_HIP(hipMemcpyAsync(h->yc, yc, 3 * (size_t)n_sel * sizeof(float), hipMemcpyHostToDevice,
                            h->s));
    RMSF_HIP(hipMemcpyAsync(h->ref, reference, 3 * (size_t)atoms * sizeof(float),
                            hipMemcpyHostToDevice, h->s));
    RMSF_HIP(hipMemsetAsync(h->total, 0, (size_t)atoms * sizeof(double), h->s));
    RMSF_HIP(hipMemsetAsync(h->carry, 0, (size_t)atoms * sizeof(double), h->s));
    RMSF_HIP(hipStreamSynchronize(h->s));
    delete[] yc;
    *out = h;
    return EK_OK;
done:
    delete[] yc;
    ek_rmsf_close(h);
    return rc;
}

template <int T, bool LDSF>
static void rmsf_launch(const RmsfArgs &a, unsigned tiles, hipStream_t s)
{
    const size_t lds = (size_t)(T / EK_WAVE) * RMSF_NRED * sizeof(double) +
                       (LDSF ? (size_t)a.atoms * (sizeof(double) + 3 * sizeof(float)) : 0);
    hipLaunchKernelGGL((rmsf_tile_kernel<T, LDSF>), dim3(tiles), dim3(T), lds, s, a);
}

extern "C" int ek_rmsf_run(ek_rmsf *h, const float *xyz, int64_t frames, const double *weights,
                           int64_t ref_index, int64_t chunk_frames, float *aligned_out,
                           double *rotations_out, float *rmsd_out, uint32_t *flags_out)
{
    int rc = rmsf_bind(h, "ek_rmsf_run");
    if (rc != EK_OK)
        return rc;
    if (!xyz || !flags_out || frames < 0 || chunk_frames < 0 || ref_index >= frames)
        return ek_set_error(EK_EARG, "ek_rmsf_run: bad argument");
    h->ms[0] = h->ms[1] = h->ms[2] = 0.0;
    if (frames == 0)
        return EK_OK;
    const int32_t A = h->atoms;
    const size_t per_frame = (size_t)A * 3 * sizeof(float) * (aligned_out ? 2 : 1) +
                             9 * sizeof(double) + sizeof(float) + sizeof(uint32_t) +
                             sizeof(double) + (size_t)A * sizeof(double) / RMSF_TILE + 1;
    int64_t chunk = chunk_frames;
    if (chunk == 0) {
        size_t free_b = 0, total_b = 0;
        hipError_t e = hipMemGetInfo(&free_b, &total_b);
        if (e != hipSuccess)
            return ek_set_error(EK_EHIP, "ek_rmsf_run: hipMemGetInfo: %s", hipGetErrorString(e));
        chunk = (int64_t)(free_b / 2 / per_frame);
        if (chunk < 1)
            return ek_set_error(EK_ENOMEM, "ek_rmsf_run: one frame of %d atoms does not fit "
                                           "%zu MiB of free device memory", A, free_b >> 20);
    }
    if (chunk > RMSF_MAX_CHUNK)
        chunk = RMSF_MAX_CHUNK;
    if (chunk > frames)
        chunk = frames;
    // (a chunk may start inside a tile and end inside another: two tiles more than it fills)
    const int64_t max_tiles = chunk / RMSF_TILE + 2;
    rc = ek_mi_check_memory((size_t)chunk * per_frame + (size_t)max_tiles * A * sizeof(double),
                            "ek_rmsf_run");
    if (rc != EK_OK)
        return rc;

    float *d_xyz = nullptr, *d_al = nullptr, *d_rmsd = nullptr;
    double *d_w = nullptr, *d_rot = nullptr, *d_part = nullptr;
    uint32_t *d_flags = nullptr;
    RMSF_HIP(ek_dev_malloc((void **)&d_xyz, (size_t)chunk * A * 3 * sizeof(float)));
    RMSF_HIP(ek_dev_malloc((void **)&d_flags, (size_t)chunk * sizeof(uint32_t)));
    if (weights) {
        RMSF_HIP(ek_dev_malloc((void **)&d_w, (size_t)chunk * sizeof(double)));
        RMSF_HIP(ek_dev_malloc((void **)&d_part, (size_t)max_tiles * A * sizeof(double)));
    }
    if (aligned_out)
        RMSF_HIP(ek_dev_malloc((void **)&d_al, (size_t)chunk * A * 3 * sizeof(float)));
    if (rotations_out)
        RMSF_HIP(ek_dev_malloc((void **)&d_rot, (size_t)chunk * 9 * sizeof(double)));
    if (rmsd_out)
        RMSF_HIP(ek_dev_malloc((void **)&d_rmsd, (size_t)chunk * sizeof(float)));
    for (int64_t f0 = 0; f0 < frames; f0 += chunk) {
        const int64_t nf = (frames - f0 < chunk) ? frames - f0 : chunk;
        const int64_t abs0 = h->n_seen, abs1 = abs0 + nf;
        const int64_t tiles = (abs1 + RMSF_TILE - 1) / RMSF_TILE - abs0 / RMSF_TILE;
        float ms = 0.f;
        RmsfArgs a;
        a.xyz = d_xyz;
        a.w = d_w;
        a.nf = nf;
        a.f_abs0 = abs0;
        a.ref_local = (ref_index >= f0 && ref_index < f0 + nf) ? ref_index - f0 : -1;
        a.atoms = A;
        a.n_sel = h->n_sel;
        a.sel = h->sel;
        a.yc = h->yc;
        a.ref = h->ref;
        a.Gy = h->Gy;
        for (int d = 0; d < 3; ++d)
            a.cref[d] = h->cref[d];
        a.aligned = d_al;
        a.rot = d_rot;
        a.rmsd = d_rmsd;
        a.flags = d_flags;
        a.partial = d_part;
        a.carry = h->carry;
        RMSF_HIP(hipEventRecord(h->ev[0], h->s));
        RMSF_HIP(hipMemcpyAsync(d_xyz, xyz + (size_t)f0 * A * 3, (size_t)nf * A * 3 * sizeof(float),
                                hipMemcpyHostToDevice, h->s));
        if (weights)
            RMSF_HIP(hipMemcpyAsync(d_w, weights + f0, (size_t)nf * sizeof(double),
                                    hipMemcpyHostToDevice, h->s));
        RMSF_HIP(hipEventRecord(h->ev[1], h->s));
        if (A > RMSF_LDS_ATOMS)
            rmsf_launch<EK_BLOCK, false>(a, (unsigned)tiles, h->s);
        else if (A > RMSF_WAVE_ATOMS)
            rmsf_launch<EK_BLOCK, true>(a, (unsigned)tiles, h->s);
        else
            rmsf_launch<EK_WAVE, true>(a, (unsigned)tiles, h->s);
        if (weights)
            hipLaunchKernelGGL(rmsf_fold_kernel, dim3((unsigned)((A + EK_BLOCK - 1) / EK_BLOCK)),
                               dim3(EK_BLOCK), 0, h->s, d_part, tiles,
                               (int32_t)(abs1 % RMSF_TILE == 0), A, h->total, h->carry);
        RMSF_HIP(hipEventRecord(h->ev[2], h->s));
        RMSF_HIP(hipGetLastError());
        RMSF_HIP(hipMemcpyAsync(flags_out + f0, d_flags, (size_t)nf * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, h->s));
        if (aligned_out)
            RMSF_HIP(hipMemcpyAsync(aligned_out + (size_t)f0 * A * 3, d_al,
                                    (size_t)nf * A * 3 * sizeof(float), hipMemcpyDeviceToHost,
                                    h->s));
        if (rotations_out)
            RMSF_HIP(hipMemcpyAsync(rotations_out + (size_t)f0 * 9, d_rot,
                                    (size_t)nf * 9 * sizeof(double), hipMemcpyDeviceToHost, h->s));
        if (rmsd_out)
            RMSF_HIP(hipMemcpyAsync(rmsd_out + f0, d_rmsd, (size_t)nf * sizeof(float),
                                    hipMemcpyDeviceToHost, h->s));
        RMSF_HIP(hipEventRecord(h->ev[3], h->s));
        RMSF_HIP(hipStreamSynchronize(h->s));
        if (weights)
            h->n_seen = abs1;
        for (int q = 0; q < 3; ++q) {
            RMSF_HIP(hipEventElapsedTime(&ms, h->ev[q], h->ev[q + 1]));
            h->ms[q] += ms;
        }
    }
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_xyz);
    (void)ek_dev_free(d_flags);
    (void)ek_dev_free(d_w);
    (void)ek_dev_free(d_part);
    (void)ek_dev_free(d_al);
    (void)ek_dev_free(d_rot);
    (void)ek_dev_free(d_rmsd);
    return rc;
}

extern "C" int ek_rmsf_fetch(ek_rmsf *h, double *atom_sums_out, double *group_sums_out)
{
    int rc = rmsf_bind(h, "ek_rmsf_fetch");
    if (rc != EK_OK)
        return rc;
    if (group_sums_out && h->n_groups == 0)
        return ek_set_error(EK_EARG, "ek_rmsf_fetch: the handle has no groups");
    const int32_t A = h->atoms;
    double *t = new (std::nothrow) double[2 * (size_t)A];
    if (!t)
        return ek_set_error(EK_ENOMEM, "ek_rmsf_fetch: out of host memory");
    RMSF_HIP(hipMemcpyAsync(t, h->total, (size_t)A * sizeof(double), hipMemcpyDeviceToHost, h->s));
    RMSF_HIP(hipMemcpyAsync(t + A, h->carry, (size_t)A * sizeof(double), hipMemcpyDeviceToHost,
                            h->s));
    RMSF_HIP(hipStreamSynchronize(h->s));
    // the incomplete last tile is one more partial, added last
    if (h->n_seen % RMSF_TILE != 0)
        for (int32_t i = 0; i < A; ++i)
            t[i] = t[i] + t[A + i];
    if (atom_sums_out)
        memcpy(atom_sums_out, t, (size_t)A * sizeof(double));
    if (group_sums_out)
        for (int32_t g = 0; g < h->n_groups; ++g) {
            double s = 0.0;
            for (int32_t q = h->goff[g]; q < h->goff[g + 1]; ++q)
                s = s + t[h->gidx[q]];
            group_sums_out[g] = s / (double)(h->goff[g + 1] - h->goff[g]);
        }
done:
    delete[] t;
    return rc;
}

extern "C" int ek_rmsf_last_timing(ek_rmsf *h, double *ms_out)
{
    if (!h || !ms_out)
        return ek_set_error(EK_EARG, "ek_rmsf_last_timing: null argument");
    for (int i = 0; i < 3; ++i)
        ms_out[i] = h->ms[i];
    return EK_OK;
}
