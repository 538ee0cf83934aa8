// ek_sasa.hip -- Shrake-Rupley solvent-accessible surface area on the device.
//
// Replaces mdtraj.shrake_rupley(mode='atom') as the reference's
// enspara/info_theory/exposons.py calls it, and condense_sidechain_sasas (:178-217).
//
// The contract, float32, nothing fused:
//   R_i      = radius_i + probe (the caller's, float32)
//   p        = (R_i * s_k) + x_i per component, s_k the k-th sphere point
//   blocked  iff for some j != i: (dx*dx + dy*dy) + dz*dz < R_j * R_j, d = p - x_j
//   count_i  = the points that are not blocked
//   area_i   = ((c * R_i) * R_i) * float(count_i), c = float(4 pi / n)
//   group    = 0.0f + the areas of its atoms, in the order they are listed
// count_i is an integer: which neighbours are tried, and in which order, is free.
//
//   count    one workgroup per (atom i, frame).  The frame's atoms are scanned in
//            batches of SASA_SCAN; the ones that can block a point of i at all
//            (r_ij < R_i + R_j + SASA_MARGIN, see below) are compacted into the LDS
//            by wave ballots.  Lane l owns the points l, l + 256, ..: for each it
//            walks the batch's list until one neighbour blocks it, starting with the
//            neighbour that blocked its previous point (neighbouring points of the
//            spiral are mostly buried by the same atom).  A bit per point keeps what
//            earlier batches blocked, so a frame of any size takes SASA_SCAN * 16
//            bytes of LDS.
//   groups   one lane per (frame, group), the sequential float32 sum.
//
// SASA_MARGIN.  j is left out only if no point of i can come out blocked by it in
// the arithmetic above.  With |x| <= SASA_MAX_COORD = 128 nm and R <= SASA_MAX_R = 4
// nm every component of p is below 256 in magnitude, so rounding p costs at most
// 2^-17 nm per component (half an ulp there; the product R_i * s_k adds 2^-24 * 4),
// 1.4e-5 nm as a vector; d, the squares, their sum and R_j * R_j each round by
// 2^-24 relative, together less than 1e-6 nm at these radii; the cull's own r_ij
// (from x_i - x_j in float32) is off by less than 1e-6 nm for r_ij < 10 nm.  A
// point's distance to x_j is at least r_ij - R_i, so j cannot block once r_ij >=
// R_i + R_j + 1.6e-5 nm.  SASA_MARGIN = 2^-13 nm = 1.2e-4 nm is seven times that.
#include "ek_common.h"

#include <math.h>
#include <new>

extern int ek_set_error(int code, const char *fmt, ...);
int ek_mi_check_memory(size_t bytes, const char *who);

#define SASA_HIP(call)                                                         \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define SASA_WG 256
#define SASA_SCAN 2048              // atoms of one batch: 32 KiB of LDS
#define SASA_MAX_POINTS 4096        // 16 per lane: one bit each (geometry.sasa.MAX_POINTS)
#define SASA_MAX_FRAMES 32768       // of one launch: grid.y
#define SASA_MARGIN 0x1p-13f        // nm, see above
#define SASA_MAX_COORD 128.0f       // nm (geometry.sasa.MAX_COORD)
#define SASA_MAX_R 4.0f             // nm, radius + probe (geometry.sasa.MAX_R)

struct ek_sasa {
    int device;
    int32_t atoms, n_points, n_groups, n_idx;
    float c;                    // float(4 pi / n_points)
    float *R, *R2;              // [atoms] radius + probe, and its square
    float *sp;                  // [3][n_points] sphere points, x then y then z
    int32_t *goff, *gidx;       // groups: [n_groups + 1] offsets into [n_idx] atom indices
    hipStream_t s;
    hipEvent_t ev[4];
    double ms[3];               // upload, count kernel, group kernel: the last run's sums
};

__global__ void __launch_bounds__(SASA_WG)
sasa_count_kernel(const float *__restrict__ xyz, int32_t atoms, const float *__restrict__ R,
                  const float *__restrict__ R2, const float *__restrict__ sp, int32_t n, float c,
                  int32_t *__restrict__ counts, float *__restrict__ areas)
{
    __shared__ float4 nb[SASA_SCAN];
    __shared__ int n_nb;
    __shared__ int wave_count[SASA_WG / EK_WAVE];
    const int tid = threadIdx.x, lane = tid & (EK_WAVE - 1), wave = tid / EK_WAVE;
    const int32_t i = (int32_t)blockIdx.x;
    const float *X = xyz + (size_t)blockIdx.y * atoms * 3;
    const float xi = X[3 * (size_t)i], yi = X[3 * (size_t)i + 1], zi = X[3 * (size_t)i + 2];
    const float Ri = R[i];
    const int per_lane = (n + SASA_WG - 1) / SASA_WG;       // <= 16
    uint32_t blocked = 0;       // bit b: point tid + 256 b is blocked
    int hint = 0;

    for (int32_t base = 0; base < atoms; base += SASA_SCAN) {
        const int32_t end = (atoms - base < SASA_SCAN) ? atoms : base + SASA_SCAN;
        if (tid == 0)
            n_nb = 0;
        __syncthreads();
        for (int32_t j0 = base; j0 < end; j0 += SASA_WG) {
            const int32_t j = j0 + tid;
            bool keep = false;
            float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < end && j != i) {
                e.x = X[3 * (size_t)j];
                e.y = X[3 * (size_t)j + 1];
                e.z = X[3 * (size_t)j + 2];
                e.w = R2[j];
                const float dx = xi - e.x, dy = yi - e.y, dz = zi - e.z;
                const float cut = (Ri + R[j]) + SASA_MARGIN;
                keep = (dx * dx + dy * dy) + dz * dz < cut * cut;
            }
            const unsigned long long m = __ballot(keep);
            int slot = 0;
            if (lane == 0 && m != 0)
                slot = atomicAdd(&n_nb, __popcll(m));
            slot = __shfl(slot, 0);
            if (keep)       // (at most end - base <= SASA_SCAN entries a batch)
                nb[slot + __popcll(m & (((unsigned long long)1 << lane) - 1))] = e;
        }
        __syncthreads();
        const int cnt = n_nb;
        for (int b = 0; b < per_lane && cnt > 0; ++b) {
            const int k = tid + SASA_WG * b;
            if (k >= n || ((blocked >> b) & 1u))
                continue;
            const float px = (Ri * sp[k]) + xi;
            const float py = (Ri * sp[(size_t)n + k]) + yi;
            const float pz = (Ri * sp[2 * (size_t)n + k]) + zi;
            bool hit = false;
            if (hint < cnt) {
                const float4 q = nb[hint];
                const float dx = px - q.x, dy = py - q.y, dz = pz - q.z;
                hit = (dx * dx + dy * dy) + dz * dz < q.w;
            }
            for (int j = 0; j < cnt && !hit; ++j) {
                const float4 q = nb[j];
                const float dx = px - q.x, dy = py - q.y, dz = pz - q.z;
                if ((dx * dx + dy * dy) + dz * dz < q.w) {
                    hit = true;
                    hint = j;
                }
            }
            if (hit)
                blocked |= 1u << b;
        }
        __syncthreads();        // the next batch overwrites the list
    }

    int free_pts = 0;
    for (int b = 0; b < per_lane; ++b) {
        const int k = tid + SASA_WG * b;
        free_pts += __popcll(__ballot(k < n && !((blocked >> b) & 1u)));
    }
    if (lane == 0)
        wave_count[wave] = free_pts;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int w = 0; w < SASA_WG / EK_WAVE; ++w)
            total += wave_count[w];
        const size_t o = (size_t)blockIdx.y * atoms + i;
        counts[o] = total;
        areas[o] = ((c * Ri) * Ri) * (float)total;
    }
}

__global__ void __launch_bounds__(SASA_WG)
sasa_group_kernel(const float *__restrict__ areas, int32_t atoms, int64_t frames,
                  const int32_t *__restrict__ goff, const int32_t *__restrict__ gidx,
                  int32_t n_groups, float *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * SASA_WG + threadIdx.x;
    if (t >= frames * n_groups)
        return;
    const int64_t f = t / n_groups;
    const int32_t g = (int32_t)(t % n_groups);
    const float *a = areas + (size_t)f * atoms;
    float sum = 0.0f;
    for (int32_t q = goff[g]; q < goff[g + 1]; ++q)
        sum = sum + a[gidx[q]];
    out[t] = sum;
}

static int sasa_bind(ek_sasa *h, const char *who)
{
    if (!h)
        return ek_set_error(EK_EARG, "%s: null handle", who);
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", h->device, hipGetErrorString(e));
    return EK_OK;
}

extern "C" int ek_sasa_close(ek_sasa *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(h->R);
    (void)ek_dev_free(h->R2);
    (void)ek_dev_free(h->sp);
    (void)ek_dev_free(h->goff);
    (void)ek_dev_free(h->gidx);
    for (hipEvent_t e : h->ev)
        if (e)
            (void)ek_event_destroy(e);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    delete h;
    return EK_OK;
}

extern "C" int ek_sasa_open(int device, int32_t atoms, const float *R, int32_t n_points,
                            const float *points, int32_t n_groups, const int32_t *group_offsets,
                            const int32_t *group_atoms, ek_sasa **out)
{
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "ek_sasa_open: null output");
    *out = nullptr;
    if (!R || !points || atoms < 1 || n_points < 1 || n_points > SASA_MAX_POINTS ||
        n_groups < 0 || (n_groups > 0 && (!group_offsets || !group_atoms)))
        return ek_set_error(EK_EARG, "ek_sasa_open: bad argument (atoms >= 1, 1 <= n_points <= "
                                     "%d)", SASA_MAX_POINTS);
    for (int32_t i = 0; i < atoms; ++i)
        if (!(R[i] > 0.0f && R[i] <= SASA_MAX_R))
            return ek_set_error(EK_EARG, "ek_sasa_open: radius + probe of atom %d is not in "
                                         "(0, %g] nm", i, (double)SASA_MAX_R);
    int32_t n_idx = 0;
    if (n_groups > 0) {
        if (group_offsets[0] != 0)
            return ek_set_error(EK_EARG, "ek_sasa_open: group offsets start at 0");
        for (int32_t g = 0; g < n_groups; ++g)
            if (group_offsets[g + 1] <= group_offsets[g])
                return ek_set_error(EK_EARG, "ek_sasa_open: group %d is empty", g);
        n_idx = group_offsets[n_groups];
        for (int32_t q = 0; q < n_idx; ++q)
            if (group_atoms[q] < 0 || group_atoms[q] >= atoms)
                return ek_set_error(EK_EARG, "ek_sasa_open: group atom %d is not in [0, %d)",
                                    group_atoms[q], atoms);
    }
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess)
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
    }
    ek_sasa *h = new (std::nothrow) ek_sasa();
    float *tmp = new (std::nothrow) float[(size_t)atoms + 3 * (size_t)n_points];
    if (!h || !tmp) {
        delete h;
        delete[] tmp;
        return ek_set_error(EK_ENOMEM, "ek_sasa_open: out of host memory");
    }
    h->device = device;
    h->atoms = atoms;
    h->n_points = n_points;
    h->n_groups = n_groups;
    h->n_idx = n_idx;
    h->c = (float)(4.0 * M_PI / (double)n_points);
    for (int32_t i = 0; i < atoms; ++i)
        tmp[i] = R[i] * R[i];
    for (int32_t k = 0; k < n_points; ++k)
        for (int d = 0; d < 3; ++d)
            tmp[(size_t)atoms + (size_t)d * n_points + k] = points[3 * (size_t)k + d];
    SASA_HIP(ek_stream_create_flags(&h->s, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev)
        SASA_HIP(ek_event_create(&e));
    SASA_HIP(ek_dev_malloc((void **)&h->R, (size_t)atoms * sizeof(float)));
    SASA_HIP(ek_dev_malloc((void **)&h->R2, (size_t)atoms * sizeof(float)));
    SASA_HIP(ek_dev_malloc((void **)&h->sp, 3 * (size_t)n_points * sizeof(float)));
    SASA_HIP(hipMemcpyAsync(h->R, R, (size_t)atoms * sizeof(float), hipMemcpyHostToDevice, h->s));
    SASA_HIP(hipMemcpyAsync(h->R2, tmp, (size_t)atoms * sizeof(float), hipMemcpyHostToDevice,
                            h->s));
    SASA_HIP(hipMemcpyAsync(h->sp, tmp + atoms, 3 * (size_t)n_points * sizeof(float),
                            hipMemcpyHostToDevice, h->s));
    if (n_groups > 0) {
        SASA_HIP(ek_dev_malloc((void **)&h->goff, ((size_t)n_groups + 1) * sizeof(int32_t)));
        SASA_HIP(ek_dev_malloc((void **)&h->gidx, (size_t)n_idx * sizeof(int32_t)));
        SASA_HIP(hipMemcpyAsync(h->goff, group_offsets, ((size_t)n_groups + 1) * sizeof(int32_t),
                                hipMemcpyHostToDevice, h->s));
        SASA_HIP(hipMemcpyAsync(h->gidx, group_atoms, (size_t)n_idx * sizeof(int32_t),
                                hipMemcpyHostToDevice, h->s));
    }
    SASA_HIP(hipStreamSynchronize(h->s));
    delete[] tmp;
    *out = h;
    return EK_OK;
done:
    delete[] tmp;
    ek_sasa_close(h);
    return rc;
}

extern "C" int ek_sasa_run(ek_sasa *h, const float *xyz, int64_t frames, int64_t chunk_frames,
                           int32_t *counts_out, float *areas_out, float *groups_out)
{
    int rc = sasa_bind(h, "ek_sasa_run");
    if (rc != EK_OK)
        return rc;
    if (!xyz || frames < 0 || chunk_frames < 0)
        return ek_set_error(EK_EARG, "ek_sasa_run: bad argument");
    if (groups_out && h->n_groups == 0)
        return ek_set_error(EK_EARG, "ek_sasa_run: the handle has no groups");
    h->ms[0] = h->ms[1] = h->ms[2] = 0.0;
    if (frames == 0)
        return EK_OK;
    // (the host part of the contract: finite coordinates within SASA_MAX_COORD)
    for (size_t q = 0, nq = (size_t)frames * h->atoms * 3; q < nq; ++q)
        if (!(fabsf(xyz[q]) <= SASA_MAX_COORD))
            return ek_set_error(EK_EARG, "ek_sasa_run: coordinate %zu is not finite or beyond "
                                         "%g nm", q, (double)SASA_MAX_COORD);

    const size_t per_frame = (size_t)h->atoms * (3 * sizeof(float) + sizeof(int32_t) +
                                                 sizeof(float)) +
                             (size_t)h->n_groups * sizeof(float);
    int64_t chunk = chunk_frames;
    if (chunk == 0) {
        size_t free_b = 0, total_b = 0;
        hipError_t e = hipMemGetInfo(&free_b, &total_b);
        if (e != hipSuccess)
            return ek_set_error(EK_EHIP, "ek_sasa_run: hipMemGetInfo: %s", hipGetErrorString(e));
        chunk = (int64_t)(free_b / 2 / per_frame);
        if (chunk < 1)
            return ek_set_error(EK_ENOMEM, "ek_sasa_run: one frame of %d atoms does not fit "
                                           "%zu MiB of free device memory", h->atoms,
                                free_b >> 20);
    }
    if (chunk > SASA_MAX_FRAMES)
        chunk = SASA_MAX_FRAMES;
    if (chunk > frames)
        chunk = frames;
    rc = ek_mi_check_memory((size_t)chunk * per_frame, "ek_sasa_run");
    if (rc != EK_OK)
        return rc;

    float *d_xyz = nullptr, *d_areas = nullptr, *d_groups = nullptr;
    int32_t *d_counts = nullptr;
    SASA_HIP(ek_dev_malloc((void **)&d_xyz, (size_t)chunk * h->atoms * 3 * sizeof(float)));
    SASA_HIP(ek_dev_malloc((void **)&d_counts, (size_t)chunk * h->atoms * sizeof(int32_t)));
    SASA_HIP(ek_dev_malloc((void **)&d_areas, (size_t)chunk * h->atoms * sizeof(float)));
    if (groups_out)
        SASA_HIP(ek_dev_malloc((void **)&d_groups, (size_t)chunk * h->n_groups * sizeof(float)));
    for (int64_t f0 = 0; f0 < frames; f0 += chunk) {
        const int64_t nf = (frames - f0 < chunk) ? frames - f0 : chunk;
        const size_t cells = (size_t)nf * h->atoms;
        float ms = 0.f;
        SASA_HIP(hipEventRecord(h->ev[0], h->s));
        SASA_HIP(hipMemcpyAsync(d_xyz, xyz + (size_t)f0 * h->atoms * 3, cells * 3 * sizeof(float),
                                hipMemcpyHostToDevice, h->s));
        SASA_HIP(hipEventRecord(h->ev[1], h->s));
        hipLaunchKernelGGL(sasa_count_kernel, dim3((unsigned)h->atoms, (unsigned)nf),
                           dim3(SASA_WG), 0, h->s, d_xyz, h->atoms, h->R, h->R2, h->sp,
                           h->n_points, h->c, d_counts, d_areas);
        SASA_HIP(hipEventRecord(h->ev[2], h->s));
        if (groups_out)
            hipLaunchKernelGGL(sasa_group_kernel,
                               dim3((unsigned)(((size_t)nf * h->n_groups + SASA_WG - 1) / SASA_WG)),
                               dim3(SASA_WG), 0, h->s, d_areas, h->atoms, nf, h->goff, h->gidx,
                               h->n_groups, d_groups);
        SASA_HIP(hipEventRecord(h->ev[3], h->s));
        SASA_HIP(hipGetLastError());
        if (counts_out)
            SASA_HIP(hipMemcpyAsync(counts_out + (size_t)f0 * h->atoms, d_counts,
                                    cells * sizeof(int32_t), hipMemcpyDeviceToHost, h->s));
        if (areas_out)
            SASA_HIP(hipMemcpyAsync(areas_out + (size_t)f0 * h->atoms, d_areas,
                                    cells * sizeof(float), hipMemcpyDeviceToHost, h->s));
        if (groups_out)
            SASA_HIP(hipMemcpyAsync(groups_out + (size_t)f0 * h->n_groups, d_groups,
                                    (size_t)nf * h->n_groups * sizeof(float),
                                    hipMemcpyDeviceToHost, h->s));
        SASA_HIP(hipStreamSynchronize(h->s));
        for (int q = 0; q < 3; ++q) {
            SASA_HIP(hipEventElapsedTime(&ms, h->ev[q], h->ev[q + 1]));
            h->ms[q] += ms;
        }
    }
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_xyz);
    (void)ek_dev_free(d_counts);
    (void)ek_dev_free(d_areas);
    (void)ek_dev_free(d_groups);
    return rc;
}

extern "C" int ek_sasa_last_timing(ek_sasa *h, double *ms_out)
{
    if (!h || !ms_out)
        return ek_set_error(EK_EARG, "ek_sasa_last_timing: null argument");
    for (int i = 0; i < 3; ++i)
        ms_out[i] = h->ms[i];
    return EK_OK;
}
