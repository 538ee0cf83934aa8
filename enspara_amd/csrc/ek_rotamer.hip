// ek_rotamer.hip -- dihedral angles from coordinates and buffered rotamer states from
// angles on the device.
//
// Replaces the reference's enspara/geometry/rotamer.py: dihedral_angles (mdtraj's
// formula and the transforms behind it), _rotamers, is_buffered_transition, get_gates.
//
// _rotamers is a state machine along time: frame t keeps the current basin unless the
// angle has left the basin's gates, then the basin becomes digitize(angle).  So frame t
// is a map basin -> basin that is the identity on some basins and one constant on the
// others, and maps compose associatively.  With at most 8 basins a map is one 32-bit
// word, four bits per start basin.
//   map     lane = one dihedral, grid.y = one chunk of ROT_CHUNK frames: the chunk's
//           composed map (chunk 0 starts from frame 0's constant)
//   carry   lane = one dihedral: the basin each chunk starts in
//   emit    as map, from the known start: the states, uint8 [frames][n]
// Lanes run across the dihedrals, so a wave's load of one frame is 64 consecutive
// dwords.  The angle of a frame comes either from the angle array or straight from the
// coordinates (the fused entry): the same device functions, the same bits.
#include "ek_common.h"

#include <new>

extern int ek_set_error(int code, const char *fmt, ...);

#define RT_HIP(call)                                                           \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define RT_WG 256
#define ROT_CHUNK 256           // frames of one lane's scan (enspara_amd.geometry.rotamer.SCAN_CHUNK)
#define ROT_MAX_FRAMES ((int64_t)1 << 27)
#define ROT_MAX_BASINS 8
#define RT_MAX_GRID_Y 65535
#define RT_IDENTITY 0x76543210u

// one kind of dihedral: boundaries hb[0 .. nb], the gates of each basin (get_gates)
struct rt_kind {
    int32_t nb;
    float shift;
    double hb[ROT_MAX_BASINS + 1];
    double lower[ROT_MAX_BASINS];
    double upper[ROT_MAX_BASINS];
};

// ---- a frame's map ---------------------------------------------------------------------------
// a = raw - shift in float32, + 360 where negative; compared in float64.  d = digitize(a),
// hb[d] <= a < hb[d + 1], an a of exactly 360 in the last basin; bit s of T = the angle is
// a buffered transition out of basin s (is_buffered_transition, both ends closed).
__device__ __forceinline__ void rt_frame(float raw, const rt_kind &K, uint32_t &T, uint32_t &d)
{
    float a32 = raw - K.shift;
    if (a32 < 0.f)
        a32 = a32 + 360.f;
    const double a = (double)a32;
    d = 0;
    T = 0;
#pragma unroll
    for (int s = 0; s < ROT_MAX_BASINS; ++s) {
        if (s >= K.nb)
            continue;
        if (s >= 1 && a >= K.hb[s])
            d += 1;
        const double lo = K.lower[s], up = K.upper[s];
        bool tr = false;
        if (up < lo)
            tr = (up <= a && a <= lo);
        else if (up > lo)
            tr = !(lo <= a && a <= up);
        T |= (tr ? 1u : 0u) << s;
    }
}

// the map `m` followed by the frame (T, d)
__device__ __forceinline__ uint32_t rt_compose(uint32_t m, uint32_t T, uint32_t d)
{
    uint32_t o = 0;
#pragma unroll
    for (int s = 0; s < ROT_MAX_BASINS; ++s) {
        const uint32_t cur = (m >> (4 * s)) & 7u;
        o |= (((T >> cur) & 1u) ? d : cur) << (4 * s);
    }
    return o;
}

// ---- the dihedral of four atoms, in degrees within [0, 359.5] ----------------------------------
// b1 = x1 - x0, b2 = x2 - x1, b3 = x3 - x2, c1 = b2 x b3, c2 = b1 x b2,
// atan2((b1 . c1) |b2|, c1 . c2) in float32, nothing fused; then the reference's
// transforms: degrees, < 0 -> + 360, > 359.5 -> 359.5
__device__ __forceinline__ float rt_dot(float ax, float ay, float az, float bx, float by,
                                        float bz)
{
    return ax * bx + ay * by + az * bz;
}

__device__ __forceinline__ float rt_dihedral_deg(const float *__restrict__ x, int4 q)
{
    const float *p0 = x + 3 * (size_t)q.x, *p1 = x + 3 * (size_t)q.y;
    const float *p2 = x + 3 * (size_t)q.z, *p3 = x + 3 * (size_t)q.w;
    const float b1x = p1[0] - p0[0], b1y = p1[1] - p0[1], b1z = p1[2] - p0[2];
    const float b2x = p2[0] - p1[0], b2y = p2[1] - p1[1], b2z = p2[2] - p1[2];
    const float b3x = p3[0] - p2[0], b3y = p3[1] - p2[1], b3z = p3[2] - p2[2];
    const float c1x = b2y * b3z - b2z * b3y, c1y = b2z * b3x - b2x * b3z,
                c1z = b2x * b3y - b2y * b3x;
    const float c2x = b1y * b2z - b1z * b2y, c2y = b1z * b2x - b1x * b2z,
                c2z = b1x * b2y - b1y * b2x;
    const float y = rt_dot(b1x, b1y, b1z, c1x, c1y, c1z) * sqrtf(rt_dot(b2x, b2y, b2z, b2x, b2y, b2z));
    const float xx = rt_dot(c1x, c1y, c1z, c2x, c2y, c2z);
    float deg = atan2f(y, xx) * 57.29577951308232f;
    if (deg < 0.f)
        deg = deg + 360.f;
    if (deg > 359.5f)
        deg = 359.5f;
    return deg;
}

// where a frame's angle comes from: angles [frames][n], or xyz [frames][atoms][3] and the
// lane's four atoms
template <bool XYZ> struct rt_source {
    const float *base;
    int64_t stride;     // floats per frame
    int4 q;
    int32_t j;
    __device__ __forceinline__ float at(int64_t t) const
    {
        if (XYZ)
            return rt_dihedral_deg(base + (size_t)t * stride, q);
        return base[(size_t)t * stride + j];
    }
};

template <bool XYZ>
__device__ __forceinline__ rt_source<XYZ> rt_make_source(const float *angles, const float *xyz,
                                                         int32_t atoms, const int32_t *quads,
                                                         int32_t n, int32_t j)
{
    rt_source<XYZ> s;
    s.j = j;
    if (XYZ) {
        s.base = xyz;
        s.stride = (int64_t)atoms * 3;
        s.q = *reinterpret_cast<const int4 *>(quads + 4 * (size_t)j);
    } else {
        s.base = angles;
        s.stride = n;
        s.q = make_int4(0, 0, 0, 0);
    }
    return s;
}

// ---- kernels ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(RT_WG)
rt_angles_kernel(const float *__restrict__ xyz, int64_t frames, int32_t atoms,
                 const int32_t *__restrict__ quads, int32_t n, float *__restrict__ out)
{
    const int32_t j = (int32_t)(blockIdx.x * RT_WG + threadIdx.x);
    if (j >= n)
        return;
    const int4 q = *reinterpret_cast<const int4 *>(quads + 4 * (size_t)j);
    for (int64_t t = blockIdx.y; t < frames; t += gridDim.y)
        out[(size_t)t * n + j] = rt_dihedral_deg(xyz + (size_t)t * atoms * 3, q);
}

template <bool XYZ>
__global__ void __launch_bounds__(RT_WG)
rt_map_kernel(const float *__restrict__ angles, const float *__restrict__ xyz, int32_t atoms,
              const int32_t *__restrict__ quads, int64_t frames, int32_t n,
              const uint8_t *__restrict__ kind, const rt_kind *__restrict__ kinds,
              int64_t chunk0, uint32_t *__restrict__ maps)
{
    const int32_t j = (int32_t)(blockIdx.x * RT_WG + threadIdx.x);
    if (j >= n)
        return;
    const int64_t c = chunk0 + blockIdx.y;
    const rt_kind K = kinds[kind[j]];
    const rt_source<XYZ> src = rt_make_source<XYZ>(angles, xyz, atoms, quads, n, j);
    int64_t t = c * ROT_CHUNK;
    const int64_t t1 = (t + ROT_CHUNK < frames) ? t + ROT_CHUNK : frames;
    uint32_t m = RT_IDENTITY, T, d;
    if (c == 0) {       // frame 0: the basin the angle lies in, whatever came before
        rt_frame(src.at(0), K, T, d);
        m = d * 0x11111111u;
        t = 1;
    }
#pragma unroll 4
    for (; t < t1; ++t) {
        rt_frame(src.at(t), K, T, d);
        m = rt_compose(m, T, d);
    }
    maps[(size_t)c * n + j] = m;
}

__global__ void __launch_bounds__(RT_WG)
rt_carry_kernel(const uint32_t *__restrict__ maps, int32_t n, int32_t chunks,
                uint8_t *__restrict__ start)
{
    const int32_t j = (int32_t)(blockIdx.x * RT_WG + threadIdx.x);
    if (j >= n)
        return;
    uint32_t st = 0;
    for (int32_t c = 0; c < chunks; ++c) {
        start[(size_t)c * n + j] = (uint8_t)st;
        st = (maps[(size_t)c * n + j] >> (4 * st)) & 7u;
    }
}

template <bool XYZ>
__global__ void __launch_bounds__(RT_WG)
rt_emit_kernel(const float *__restrict__ angles, const float *__restrict__ xyz, int32_t atoms,
               const int32_t *__restrict__ quads, int64_t frames, int32_t n,
               const uint8_t *__restrict__ kind, const rt_kind *__restrict__ kinds,
               int64_t chunk0, const uint8_t *__restrict__ start,
               uint8_t *__restrict__ states, float *__restrict__ angles_out)
{
    const int32_t j = (int32_t)(blockIdx.x * RT_WG + threadIdx.x);
    if (j >= n)
        return;
    const int64_t c = chunk0 + blockIdx.y;
    const rt_kind K = kinds[kind[j]];
    const rt_source<XYZ> src = rt_make_source<XYZ>(angles, xyz, atoms, quads, n, j);
    int64_t t = c * ROT_CHUNK;
    const int64_t t1 = (t + ROT_CHUNK < frames) ? t + ROT_CHUNK : frames;
    uint32_t cur = start[(size_t)c * n + j], T, d;
#pragma unroll 4
    for (; t < t1; ++t) {
        const float a = src.at(t);
        rt_frame(a, K, T, d);
        if (t == 0 || ((T >> cur) & 1u))
            cur = d;
        states[(size_t)t * n + j] = (uint8_t)cur;
        if (XYZ && angles_out)
            angles_out[(size_t)t * n + j] = a;
    }
}

// ---- host ------------------------------------------------------------------------------------
static int rt_check_memory(size_t bytes, const char *who)
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

// the kinds' tables from the caller's arrays; EK_EARG where they break the contract
static int rt_make_kinds(const char *who, int32_t n, const uint8_t *kind, int32_t n_kinds,
                         const int32_t *n_basins, const double *hb, const float *shift,
                         double width, rt_kind *out)
{
    if (!kind || !n_basins || !hb || !shift || n_kinds < 1 || n_kinds > 255)
        return ek_set_error(EK_EARG, "%s: bad argument (1 <= kinds <= 255)", who);
    for (int32_t k = 0; k < n_kinds; ++k) {
        const int32_t nb = n_basins[k];
        const double *b = hb + (size_t)k * (ROT_MAX_BASINS + 1);
        if (nb < 1 || nb > ROT_MAX_BASINS)
            return ek_set_error(EK_EARG, "%s: kind %d has %d basins (1 .. %d)", who, k, nb,
                                ROT_MAX_BASINS);
        if (b[0] != 0.0 || b[nb] != 360.0)
            return ek_set_error(EK_EARG, "%s: the boundaries of kind %d do not run from 0 to "
                                         "360", who, k);
        for (int32_t s = 0; s < nb; ++s)
            if (!(b[s] < b[s + 1]))
                return ek_set_error(EK_EARG, "%s: the boundaries of kind %d do not increase",
                                    who, k);
        if (!(width >= 0.0 && width < 360.0 / nb))
            return ek_set_error(EK_EARG, "%s: buffer width %g outside [0, 360 / %d)", who,
                                width, nb);
        rt_kind &K = out[k];
        K = rt_kind();
        K.nb = nb;
        K.shift = shift[k];
        for (int32_t s = 0; s <= nb; ++s)
            K.hb[s] = b[s];
        for (int32_t s = 0; s < nb; ++s) {      // get_gates
            K.lower[s] = (b[s] == 0.0 ? 360.0 : b[s]) - width;
            K.upper[s] = (b[s + 1] == 360.0 ? 0.0 : b[s + 1]) + width;
        }
    }
    for (int32_t j = 0; j < n; ++j)
        if (kind[j] >= n_kinds)
            return ek_set_error(EK_EARG, "%s: dihedral %d is of kind %d of %d", who, j,
                                (int)kind[j], n_kinds);
    return EK_OK;
}

static int rt_check_quads(const char *who, const int32_t *quads, int32_t n, int32_t atoms)
{
    if (!quads)
        return ek_set_error(EK_EARG, "%s: null atom indices", who);
    for (size_t i = 0; i < (size_t)n * 4; ++i)
        if (quads[i] < 0 || quads[i] >= atoms)
            return ek_set_error(EK_EARG, "%s: atom index %d outside [0, %d)", who, quads[i],
                                atoms);
    return EK_OK;
}

// angles or xyz (+ quads) on the host -> states (and angles) on the host
static int rt_run(const char *who, int device, const float *angles, const float *xyz,
                  int64_t frames, int32_t atoms, const int32_t *quads, int32_t n,
                  const uint8_t *kind, int32_t n_kinds, const int32_t *n_basins,
                  const double *hb, const float *shift, double width, uint8_t *states_out,
                  float *angles_out, double *ms_out)
{
    int rc = EK_OK;
    const bool from_xyz = xyz != nullptr;
    if (frames < 0 || n < 1 || (from_xyz && atoms < 1) || (!states_out && !angles_out))
        return ek_set_error(EK_EARG, "%s: bad argument", who);
    const int64_t chunks = (frames + ROT_CHUNK - 1) / ROT_CHUNK;
    if (frames > ROT_MAX_FRAMES)
        return ek_set_error(EK_EARG, "%s: at most %lld frames", who, (long long)ROT_MAX_FRAMES);
    if (from_xyz) {
        rc = rt_check_quads(who, quads, n, atoms);
        if (rc != EK_OK)
            return rc;
    }
    rt_kind *kinds = nullptr;
    if (states_out) {
        kinds = new (std::nothrow) rt_kind[n_kinds > 0 ? n_kinds : 1];
        if (!kinds)
            return ek_set_error(EK_ENOMEM, "%s: out of host memory", who);
        rc = rt_make_kinds(who, n, kind, n_kinds, n_basins, hb, shift, width, kinds);
        if (rc != EK_OK) {
            delete[] kinds;
            return rc;
        }
    }
    if (ms_out)
        ms_out[0] = ms_out[1] = 0.0;
    if (frames == 0) {
        delete[] kinds;
        return EK_OK;
    }
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess) {
            delete[] kinds;
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
        }
    }
    const size_t cells = (size_t)frames * n;
    const size_t in_b = from_xyz ? (size_t)frames * atoms * 3 * sizeof(float)
                                 : cells * sizeof(float);
    const size_t ang_b = (from_xyz && angles_out) ? cells * sizeof(float) : 0;
    const size_t st_b = states_out ? cells : 0;
    const size_t map_b = states_out ? (size_t)chunks * n * (sizeof(uint32_t) + 1) : 0;
    const unsigned gx = (n + RT_WG - 1) / RT_WG;
    float *d_in = nullptr, *d_ang = nullptr;
    int32_t *d_quads = nullptr;
    uint8_t *d_kind = nullptr, *d_start = nullptr, *d_states = nullptr;
    rt_kind *d_kinds = nullptr;
    uint32_t *d_maps = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float ms = 0.f;

    rc = rt_check_memory(in_b + ang_b + st_b + map_b + (size_t)n * 20, who);
    if (rc != EK_OK)
        goto done;
    RT_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    for (hipEvent_t &e : ev)
        RT_HIP(ek_event_create(&e));
    RT_HIP(ek_dev_malloc((void **)&d_in, in_b));
    RT_HIP(hipMemcpyAsync(d_in, from_xyz ? xyz : angles, in_b, hipMemcpyHostToDevice, s));
    if (from_xyz) {
        RT_HIP(ek_dev_malloc((void **)&d_quads, (size_t)n * 4 * sizeof(int32_t)));
        RT_HIP(hipMemcpyAsync(d_quads, quads, (size_t)n * 4 * sizeof(int32_t),
                              hipMemcpyHostToDevice, s));
        if (angles_out)
            RT_HIP(ek_dev_malloc((void **)&d_ang, ang_b));
    }
    if (states_out) {
        RT_HIP(ek_dev_malloc((void **)&d_kind, (size_t)n));
        RT_HIP(ek_dev_malloc((void **)&d_kinds, (size_t)n_kinds * sizeof(rt_kind)));
        RT_HIP(ek_dev_malloc((void **)&d_maps, (size_t)chunks * n * sizeof(uint32_t)));
        RT_HIP(ek_dev_malloc((void **)&d_start, (size_t)chunks * n));
        RT_HIP(ek_dev_malloc((void **)&d_states, st_b));
        RT_HIP(hipMemcpyAsync(d_kind, kind, (size_t)n, hipMemcpyHostToDevice, s));
        RT_HIP(hipMemcpyAsync(d_kinds, kinds, (size_t)n_kinds * sizeof(rt_kind),
                              hipMemcpyHostToDevice, s));
    }
    RT_HIP(hipEventRecord(ev[0], s));
    if (!states_out) {
        const unsigned gy = (unsigned)(frames < RT_MAX_GRID_Y ? frames : RT_MAX_GRID_Y);
        hipLaunchKernelGGL(rt_angles_kernel, dim3(gx, gy), dim3(RT_WG), 0,
                           s, d_in, frames, atoms, d_quads, n, d_ang);
        RT_HIP(hipEventRecord(ev[1], s));
    } else {
        RT_HIP(hipEventRecord(ev[1], s));
        // (the grid's y is limited: the chunks in batches, every map before the carry)
        for (int64_t c0 = 0; c0 < chunks; c0 += RT_MAX_GRID_Y) {
            const dim3 grid(gx, (unsigned)(chunks - c0 < RT_MAX_GRID_Y ? chunks - c0
                                                                        : RT_MAX_GRID_Y));
            if (from_xyz)
                hipLaunchKernelGGL(rt_map_kernel<true>, grid, dim3(RT_WG), 0, s, nullptr, d_in,
                                   atoms, d_quads, frames, n, d_kind, d_kinds, c0, d_maps);
            else
                hipLaunchKernelGGL(rt_map_kernel<false>, grid, dim3(RT_WG), 0, s, d_in, nullptr,
                                   0, nullptr, frames, n, d_kind, d_kinds, c0, d_maps);
        }
        hipLaunchKernelGGL(rt_carry_kernel, dim3(gx), dim3(RT_WG), 0, s, d_maps, n,
                           (int32_t)chunks, d_start);
        for (int64_t c0 = 0; c0 < chunks; c0 += RT_MAX_GRID_Y) {
            const dim3 grid(gx, (unsigned)(chunks - c0 < RT_MAX_GRID_Y ? chunks - c0
                                                                        : RT_MAX_GRID_Y));
            if (from_xyz)
                hipLaunchKernelGGL(rt_emit_kernel<true>, grid, dim3(RT_WG), 0, s, nullptr, d_in,
                                   atoms, d_quads, frames, n, d_kind, d_kinds, c0, d_start,
                                   d_states, d_ang);
            else
                hipLaunchKernelGGL(rt_emit_kernel<false>, grid, dim3(RT_WG), 0, s, d_in, nullptr,
                                   0, nullptr, frames, n, d_kind, d_kinds, c0, d_start, d_states,
                                   nullptr);
        }
    }
    RT_HIP(hipEventRecord(ev[2], s));
    RT_HIP(hipGetLastError());
    if (states_out)
        RT_HIP(hipMemcpyAsync(states_out, d_states, st_b, hipMemcpyDeviceToHost, s));
    if (d_ang)
        RT_HIP(hipMemcpyAsync(angles_out, d_ang, ang_b, hipMemcpyDeviceToHost, s));
    RT_HIP(hipStreamSynchronize(s));
    if (ms_out) {
        RT_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        ms_out[0] = ms;
        RT_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
        ms_out[1] = ms;
    }
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_in);
    (void)ek_dev_free(d_ang);
    (void)ek_dev_free(d_quads);
    (void)ek_dev_free(d_kind);
    (void)ek_dev_free(d_kinds);
    (void)ek_dev_free(d_maps);
    (void)ek_dev_free(d_start);
    (void)ek_dev_free(d_states);
    for (hipEvent_t e : ev)
        if (e)
            (void)ek_event_destroy(e);
    if (s)
        (void)ek_stream_destroy(s);
    delete[] kinds;
    return rc;
}

extern "C" int ek_rotamer_states(int device, const float *angles, int64_t frames, int32_t n,
                                 const uint8_t *kind, int32_t n_kinds, const int32_t *n_basins,
                                 const double *hb, const float *shift, double width,
                                 uint8_t *states_out, double *ms_out)
{
    if (!angles || !states_out)
        return ek_set_error(EK_EARG, "ek_rotamer_states: null argument");
    return rt_run("ek_rotamer_states", device, angles, nullptr, frames, 0, nullptr, n, kind,
                  n_kinds, n_basins, hb, shift, width, states_out, nullptr, ms_out);
}

extern "C" int ek_dihedral_angles(int device, const float *xyz, int64_t frames, int32_t atoms,
                                  const int32_t *quads, int32_t n, float *angles_out,
                                  double *ms_out)
{
    if (!xyz || !angles_out)
        return ek_set_error(EK_EARG, "ek_dihedral_angles: null argument");
    return rt_run("ek_dihedral_angles", device, nullptr, xyz, frames, atoms, quads, n, nullptr, 0,
                  nullptr, nullptr, nullptr, 0.0, nullptr, angles_out, ms_out);
}

extern "C" int ek_dihedral_rotamers(int device, const float *xyz, int64_t frames, int32_t atoms,
                                    const int32_t *quads, int32_t n, const uint8_t *kind,
                                    int32_t n_kinds, const int32_t *n_basins, const double *hb,
                                    const float *shift, double width, uint8_t *states_out,
                                    float *angles_out, double *ms_out)
{
    if (!xyz || !states_out)
        return ek_set_error(EK_EARG, "ek_dihedral_rotamers: null argument");
    return rt_run("ek_dihedral_rotamers", device, nullptr, xyz, frames, atoms, quads, n, kind,
                  n_kinds, n_basins, hb, shift, width, states_out, angles_out, ms_out);
}
