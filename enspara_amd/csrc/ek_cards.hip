// ek_cards.hip -- CARDS on the device: transition statistics, order / disorder codes
// and the four mutual-information matrices of rotamer and disorder states.
//
// Replaces the reference's enspara/cards/disorder.py (transitions,
// traj_ord_disord_times, create_disorder_traj, assign_order_disorder) and the four
// mi_matrix calls of cards.py::cards_matrices.
//
// The codes of every trajectory stay on the device in ek_mi.hip's packed layout,
// [F][frames padded to 64 with MI_PAD], where 16 frames of one feature are one 16-byte
// load.  Both scans run along that axis: a wave owns one feature and one chunk of
// CARDS_CHUNK frames, in CARDS_STEPS 16-byte loads per lane: in the disorder kernel lane
// l takes the 16 frames at chunk + 16 (64 k + l), k = 0 .. CARDS_STEPS - 1 (a wave's load
// and store are 1024 contiguous bytes), in the stats kernel the 16 CARDS_STEPS frames in
// a row at chunk + 16 CARDS_STEPS l (one join across the wave instead of one per step).
//   stats     a lane turns its 16 codes into a 16-bit mask of transitions (X[t] !=
//             X[t + 1], t + 1 < frames); masks join into segments (n, first, last, the
//             sum of d (d + 1) / 2 over the gaps d between neighbours), an associative
//             join, first inside the lane, then across the lanes -> one segment per
//             chunk
//   combine   one lane per feature joins the chunks' segments in order -> stats [F][4],
//             and notes for every chunk the last transition before it and the first one
//             behind it (the carries of the disorder scan)
//   disorder  per frame the previous transition a <= t (prefix maximum over lanes, steps
//             and the chunk's carry) and the next one b > t (suffix minimum); D = 1
//             where both exist and lo <= b - a <= hi, integer compares only
//   matrices  ek_mi's count kernel on S-S, D-D and S-D, the D-S counts as the exact
//             integer transpose of S-D, ek_mi's information kernel on each of the four
#include "ek_common.h"
#include "ek_mi_launch.h"

#include <new>
#include <vector>

extern int ek_set_error(int code, const char *fmt, ...);

#define CD_HIP(call)                                                           \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define CD_WG 256
#define CARDS_CHUNK 2048        // frames of a wave (enspara_amd.cards.SCAN_CHUNK)
#define CARDS_STEPS (CARDS_CHUNK / 1024)
#define CARDS_MAX_FRAMES ((int64_t)1 << 26)    // so that s2 < 2^53 (and times fit an int)
#define CD_NONE 0x7fffffff      // no next transition

struct cd_traj {
    int64_t frames, tpad, chunks;
    uint8_t *S, *D;             // [F][tpad] rotamer / disorder codes
    int64_t *part;              // [F][chunks][4] the chunks' segments
    int32_t *carry;             // [F][chunks][2] last transition before, first behind
    int64_t *stats;             // [F][4]
};

struct ek_cards {
    int device;
    int32_t f, n;
    uint64_t n_obs;
    bool disordered, counted;
    std::vector<cd_traj> trajs;
    uint32_t *jc[4];            // S-S [f][f][n][n], D-D [f][f][2][2], S-D [f][f][n][2], D-S
    int64_t *lo, *hi;           // [f]
    hipStream_t s;
    hipEvent_t ev[8];
    double ms[8];
};

static size_t cd_cells(const ek_cards *h, int which)
{
    const size_t ff = (size_t)h->f * h->f;
    switch (which) {
    case 0: return ff * h->n * h->n;
    case 1: return ff * 4;
    default: return ff * h->n * 2;
    }
}

// ---- transitions of 16 frames ---------------------------------------------------------------
// bit k of the result: X[p + k] != X[p + k + 1] and p + k + 1 < frames.  p is a multiple
// of 16; at or past tpad nothing is read.
__device__ __forceinline__ uint32_t cd_nonzero_bytes(uint32_t x)
{
    const uint32_t t = (((x | 0x80808080u) - 0x01010101u) | x) & 0x80808080u;
    return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}

__device__ __forceinline__ uint32_t cd_transitions(const uint8_t *__restrict__ row, int32_t p,
                                                   int32_t tpad, int32_t frames)
{
    if (p >= tpad)
        return 0;
    const uint4 w = *reinterpret_cast<const uint4 *>(row + p);
    const uint32_t ahead = (p + 16 < tpad) ? row[p + 16] : (uint32_t)MI_PAD;
    const uint32_t dx = w.x ^ ((w.x >> 8) | (w.y << 24));
    const uint32_t dy = w.y ^ ((w.y >> 8) | (w.z << 24));
    const uint32_t dz = w.z ^ ((w.z >> 8) | (w.w << 24));
    const uint32_t dw = w.w ^ ((w.w >> 8) | (ahead << 24));
    const uint32_t m = cd_nonzero_bytes(dx) | (cd_nonzero_bytes(dy) << 4) |
                       (cd_nonzero_bytes(dz) << 8) | (cd_nonzero_bytes(dw) << 12);
    int32_t valid = frames - 1 - p;     // frames t of this lane with t + 1 < frames
    valid = valid < 0 ? 0 : (valid > 16 ? 16 : valid);
    return m & ((1u << valid) - 1u);
}

// ---- segments ---------------------------------------------------------------------------------
struct cd_seg {
    int32_t n, first, last;     // (a trajectory has fewer than 2^26 frames)
    long long s2;               // sum of d (d + 1) / 2 over the gaps inside
};

__device__ __forceinline__ cd_seg cd_join(cd_seg a, cd_seg b)
{
    if (a.n == 0)
        return b;
    if (b.n == 0)
        return a;
    const long long d = b.first - a.last;
    return cd_seg{a.n + b.n, a.first, b.last, a.s2 + b.s2 + d * (d + 1) / 2};
}

__device__ __forceinline__ cd_seg cd_seg_of_mask(uint32_t m, int32_t p)
{
    cd_seg s{0, 0, 0, 0};
    if (m == 0)
        return s;
    s.n = __popc(m);
    s.first = p + (__ffs((int)m) - 1);
    s.last = p + (31 - __clz((int)m));
    int prev = -1;
    for (uint32_t mm = m; mm; mm &= mm - 1) {
        const int k = __ffs((int)mm) - 1;
        if (prev >= 0) {
            const long long d = k - prev;
            s.s2 += d * (d + 1) / 2;
        }
        prev = k;
    }
    return s;
}

// wave w of the grid owns (feature w / chunks, chunk w % chunks)
__global__ void __launch_bounds__(CD_WG)
cd_stats_kernel(const uint8_t *__restrict__ codes, int32_t frames, int32_t tpad, int32_t F,
                int32_t chunks, int64_t *__restrict__ part)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (CD_WG / 64) + (threadIdx.x >> 6);
    if (w >= (int64_t)F * chunks)
        return;
    const int32_t f = (int32_t)(w / chunks), c = (int32_t)(w % chunks);
    const uint8_t *row = codes + (size_t)f * tpad;
    // (here a lane takes 16 CARDS_STEPS frames in a row, so that the wave joins only once)
    cd_seg acc{0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < CARDS_STEPS; ++k) {
        const int32_t p = c * CARDS_CHUNK + 16 * (CARDS_STEPS * lane + k);
        acc = cd_join(acc, cd_seg_of_mask(cd_transitions(row, p, tpad, frames), p));
    }
    for (int off = 1; off < 64; off <<= 1) {
        cd_seg o;
        o.n = __shfl_down(acc.n, off);
        o.first = __shfl_down(acc.first, off);
        o.last = __shfl_down(acc.last, off);
        o.s2 = __shfl_down(acc.s2, off);
        if (lane + off < 64)
            acc = cd_join(acc, o);      // (lane 0's becomes the wave's)
    }
    if (lane == 0) {
        int64_t *o = part + (size_t)w * 4;
        o[0] = acc.n;
        o[1] = acc.first;
        o[2] = acc.last;
        o[3] = acc.s2;
    }
}

// one lane per feature: the chunks in order.  stats = (n, first, last, s2) with s2 = the
// sum of w (w + 1) / 2 over the waiting times w = [first, gaps ...]; without a transition
// (0, -1, -1, 0).
__global__ void __launch_bounds__(CD_WG)
cd_combine_kernel(const int64_t *__restrict__ part, int32_t F, int32_t chunks,
                  int32_t *__restrict__ carry, int64_t *__restrict__ stats)
{
    const int32_t f = (int32_t)(blockIdx.x * CD_WG + threadIdx.x);
    if (f >= F)
        return;
    const int64_t *p = part + (size_t)f * chunks * 4;
    int32_t *cr = carry + (size_t)f * chunks * 2;
    cd_seg acc{0, 0, 0, 0};
    int32_t prev = -1;
    for (int32_t c = 0; c < chunks; ++c) {
        cr[2 * c] = prev;
        const cd_seg s{(int32_t)p[4 * c], (int32_t)p[4 * c + 1], (int32_t)p[4 * c + 2],
                       p[4 * c + 3]};
        if (s.n)
            prev = (int32_t)s.last;
        acc = cd_join(acc, s);
    }
    int32_t next = -1;
    for (int32_t c = chunks - 1; c >= 0; --c) {
        cr[2 * c + 1] = next;
        if (p[4 * c])
            next = (int32_t)p[4 * c + 1];
    }
    int64_t *o = stats + (size_t)f * 4;
    o[0] = acc.n;
    o[1] = acc.n ? acc.first : -1;
    o[2] = acc.n ? acc.last : -1;
    o[3] = acc.n ? acc.s2 + (long long)acc.first * (acc.first + 1) / 2 : 0;
}

// ---- disorder codes ------------------------------------------------------------------------------
// D[t] = 1 where transitions a <= t < b are neighbours and lo <= b - a <= hi; 0 elsewhere
// below `frames`, MI_PAD behind: the layout the count kernel reads.
__global__ void __launch_bounds__(CD_WG)
cd_disorder_kernel(const uint8_t *__restrict__ codes, int32_t frames, int32_t tpad, int32_t F,
                   int32_t chunks, const int32_t *__restrict__ carry,
                   const int64_t *__restrict__ lo, const int64_t *__restrict__ hi,
                   uint8_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (CD_WG / 64) + (threadIdx.x >> 6);
    if (w >= (int64_t)F * chunks)
        return;
    const int32_t f = (int32_t)(w / chunks), c = (int32_t)(w % chunks);
    const uint8_t *row = codes + (size_t)f * tpad;
    const int64_t lo_f = lo[f], hi_f = hi[f];
    const int32_t prev_c = carry[(size_t)w * 2];
    int32_t next_c = carry[(size_t)w * 2 + 1];
    next_c = next_c < 0 ? CD_NONE : next_c;

    uint32_t m[CARDS_STEPS];
    int32_t before[CARDS_STEPS], behind[CARDS_STEPS];   // of the lanes below / above, this step
    int32_t step_last[CARDS_STEPS], step_first[CARDS_STEPS];
#pragma unroll
    for (int k = 0; k < CARDS_STEPS; ++k) {
        const int32_t p = c * CARDS_CHUNK + 16 * (64 * k + lane);
        m[k] = cd_transitions(row, p, tpad, frames);
        int32_t v = m[k] ? p + (31 - __clz((int)m[k])) : -1;
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t o = __shfl_up(v, off);
            if (lane >= off)
                v = v > o ? v : o;
        }
        step_last[k] = __shfl(v, 63);
        const int32_t b = __shfl_up(v, 1);
        before[k] = lane ? b : -1;
        v = m[k] ? p + (__ffs((int)m[k]) - 1) : CD_NONE;
        for (int off = 1; off < 64; off <<= 1) {
            const int32_t o = __shfl_down(v, off);
            if (lane + off < 64)
                v = v < o ? v : o;
        }
        step_first[k] = __shfl(v, 0);
        const int32_t a = __shfl_down(v, 1);
        behind[k] = lane < 63 ? a : CD_NONE;
    }
    // the carries into each step: from the steps before it and the chunk's own
    int32_t prev_in[CARDS_STEPS], next_in[CARDS_STEPS];
    int32_t run = prev_c;
#pragma unroll
    for (int k = 0; k < CARDS_STEPS; ++k) {
        prev_in[k] = run;
        run = step_last[k] > run ? step_last[k] : run;
    }
    run = next_c;
#pragma unroll
    for (int k = CARDS_STEPS - 1; k >= 0; --k) {
        next_in[k] = run;
        run = step_first[k] < run ? step_first[k] : run;
    }
#pragma unroll
    for (int k = 0; k < CARDS_STEPS; ++k) {
        const int32_t p = c * CARDS_CHUNK + 16 * (64 * k + lane);
        if (p >= tpad)
            continue;
        const int32_t prev_l = before[k] > prev_in[k] ? before[k] : prev_in[k];
        const int32_t next_l = behind[k] < next_in[k] ? behind[k] : next_in[k];
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int32_t t = p + j;
            const uint32_t pm = m[k] & ((2u << j) - 1u);
            const int32_t a = pm ? p + (31 - __clz((int)pm)) : prev_l;
            const uint32_t nm = m[k] >> (j + 1);
            const int32_t b = nm ? t + __ffs((int)nm) : next_l;
            const int64_t span = (int64_t)b - a;
            uint32_t code = (a >= 0 && b != CD_NONE && span >= lo_f && span <= hi_f) ? 1u : 0u;
            code = t < frames ? code : (uint32_t)MI_PAD;
            o[j >> 2] |= code << (8 * (j & 3));
        }
        *reinterpret_cast<uint4 *>(out + (size_t)f * tpad + p) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// ---- unpack: codes [F][tpad] -> out [frames][F], through the LDS as the pack kernel does -------
__global__ void __launch_bounds__(CD_WG)
cd_unpack_kernel(const uint8_t *__restrict__ in, int64_t frames, int32_t F, int64_t tpad,
                 uint8_t *__restrict__ out)
{
    __shared__ uint8_t tile[64][65];
    const int64_t t0 = (int64_t)blockIdx.x * 64;
    const int32_t f0 = (int32_t)blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += CD_WG / 64) {
        const int32_t f = f0 + i;       // (t0 + tx < tpad: tpad is a multiple of 64)
        tile[i][tx] = (f < F) ? in[(size_t)f * tpad + t0 + tx] : (uint8_t)0;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += CD_WG / 64) {
        const int64_t t = t0 + i;
        const int32_t f = f0 + tx;
        if (t < frames && f < F)
            out[(size_t)t * F + f] = tile[tx][i];
    }
}

// ---- D-S counts from the S-D counts: ds[i][j][u][v] = sd[j][i][v][u] -------------------------
__global__ void __launch_bounds__(CD_WG)
cd_transpose_kernel(const uint32_t *__restrict__ sd, int32_t F, int32_t n, size_t cells,
                    uint32_t *__restrict__ ds)
{
    const size_t x = (size_t)blockIdx.x * CD_WG + threadIdx.x;
    if (x >= cells)
        return;
    const size_t v = x % n, u = (x / n) % 2, j = (x / n / 2) % F, i = x / n / 2 / F;
    ds[x] = sd[((j * F + i) * n + v) * 2 + u];
}

// ---- host ------------------------------------------------------------------------------------
static int cd_bind(ek_cards *h, const char *who)
{
    if (!h)
        return ek_set_error(EK_EARG, "%s: null handle", who);
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", h->device, hipGetErrorString(e));
    return EK_OK;
}

static void cd_free_traj(cd_traj &t)
{
    (void)ek_dev_free(t.S);
    (void)ek_dev_free(t.D);
    (void)ek_dev_free(t.part);
    (void)ek_dev_free(t.carry);
    (void)ek_dev_free(t.stats);
    t = cd_traj();
}

extern "C" int ek_cards_close(ek_cards *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    for (cd_traj &t : h->trajs)
        cd_free_traj(t);
    for (uint32_t *p : h->jc)
        (void)ek_dev_free(p);
    (void)ek_dev_free(h->lo);
    (void)ek_dev_free(h->hi);
    for (hipEvent_t e : h->ev)
        if (e)
            (void)ek_event_destroy(e);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    delete h;
    return EK_OK;
}

extern "C" int ek_cards_open(int device, int32_t f, int32_t n_states, ek_cards **out)
{
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "ek_cards_open: null output");
    *out = nullptr;
    rc = ek_mi_check_shape(f, f, n_states < 2 ? 2 : n_states, n_states < 2 ? 2 : n_states,
                           "ek_cards_open");
    if (rc != EK_OK)
        return rc;
    if (n_states < 1)
        return ek_set_error(EK_EARG, "ek_cards_open: bad argument (1 <= states <= %d)",
                            MI_MAX_STATES);
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess)
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device,
                                hipGetErrorString(e0));
    }
    ek_cards *h = new (std::nothrow) ek_cards();
    if (!h)
        return ek_set_error(EK_ENOMEM, "ek_cards_open: out of host memory");
    h->device = device;
    h->f = f;
    h->n = n_states;
    {
        size_t bytes = (size_t)f * 2 * sizeof(int64_t);
        for (int k = 0; k < 4; ++k)
            bytes += cd_cells(h, k) * sizeof(uint32_t);
        rc = ek_mi_check_memory(bytes, "ek_cards_open");
        if (rc != EK_OK)
            goto done;
    }
    CD_HIP(ek_stream_create_flags(&h->s, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev)
        CD_HIP(ek_event_create(&e));
    for (int k = 0; k < 4; ++k)
        CD_HIP(ek_dev_malloc((void **)&h->jc[k], cd_cells(h, k) * sizeof(uint32_t)));
    CD_HIP(ek_dev_malloc((void **)&h->lo, (size_t)f * sizeof(int64_t)));
    CD_HIP(ek_dev_malloc((void **)&h->hi, (size_t)f * sizeof(int64_t)));
    *out = h;
    return EK_OK;
done:
    ek_cards_close(h);
    return rc;
}

extern "C" int ek_cards_add(ek_cards *h, const uint8_t *X, int64_t frames)
{
    int rc = cd_bind(h, "ek_cards_add");
    if (rc != EK_OK)
        return rc;
    if (!X || frames < 1 || frames >= CARDS_MAX_FRAMES)
        return ek_set_error(EK_EARG, "ek_cards_add: bad argument (1 <= frames < 2^26)");
    if (h->n_obs + (uint64_t)frames >= ((uint64_t)1 << 32))
        return ek_set_error(EK_EARG, "ek_cards_add: %llu + %lld observations do not fit the "
                                     "counts (2^32)", (unsigned long long)h->n_obs,
                            (long long)frames);
    cd_traj t = cd_traj();
    t.frames = frames;
    t.tpad = ek_mi_tpad(frames);
    t.chunks = (t.tpad + CARDS_CHUNK - 1) / CARDS_CHUNK;
    const int64_t waves = (int64_t)h->f * t.chunks;
    if ((waves + 3) / 4 > INT32_MAX)
        return ek_set_error(EK_EARG, "ek_cards_add: features x frames is too large");
    const size_t raw_b = (size_t)frames * h->f, code_b = (size_t)h->f * t.tpad;
    const size_t part_b = (size_t)waves * 4 * sizeof(int64_t);
    const size_t carry_b = (size_t)waves * 2 * sizeof(int32_t);
    const size_t stats_b = (size_t)h->f * 4 * sizeof(int64_t);
    uint8_t *d_raw = nullptr;
    float ms = 0.f;

    rc = ek_mi_check_memory(raw_b + 2 * code_b + part_b + carry_b + stats_b, "ek_cards_add");
    if (rc != EK_OK)
        return rc;
    CD_HIP(ek_dev_malloc((void **)&d_raw, raw_b));
    CD_HIP(ek_dev_malloc((void **)&t.S, code_b));
    CD_HIP(ek_dev_malloc((void **)&t.D, code_b));
    CD_HIP(ek_dev_malloc((void **)&t.part, part_b));
    CD_HIP(ek_dev_malloc((void **)&t.carry, carry_b));
    CD_HIP(ek_dev_malloc((void **)&t.stats, stats_b));
    CD_HIP(hipEventRecord(h->ev[0], h->s));
    CD_HIP(hipMemcpyAsync(d_raw, X, raw_b, hipMemcpyHostToDevice, h->s));
    ek_mi_launch_pack(d_raw, frames, h->f, t.tpad, t.S, h->s);
    CD_HIP(hipEventRecord(h->ev[1], h->s));
    hipLaunchKernelGGL(cd_stats_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(CD_WG), 0, h->s,
                       t.S, (int32_t)frames, (int32_t)t.tpad, h->f, (int32_t)t.chunks, t.part);
    hipLaunchKernelGGL(cd_combine_kernel, dim3((h->f + CD_WG - 1) / CD_WG), dim3(CD_WG), 0,
                       h->s, t.part, h->f, (int32_t)t.chunks, t.carry, t.stats);
    CD_HIP(hipEventRecord(h->ev[2], h->s));
    CD_HIP(hipGetLastError());
    CD_HIP(hipStreamSynchronize(h->s));
    CD_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms[0] = ms;
    CD_HIP(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
    h->ms[1] = ms;
    (void)ek_dev_free(d_raw);
    h->trajs.push_back(t);
    h->n_obs += (uint64_t)frames;
    h->disordered = h->counted = false;
    return EK_OK;
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_raw);
    cd_free_traj(t);
    return rc;
}

extern "C" int ek_cards_stats(ek_cards *h, int64_t *stats_out)
{
    int rc = cd_bind(h, "ek_cards_stats");
    if (rc != EK_OK)
        return rc;
    if (!stats_out)
        return ek_set_error(EK_EARG, "ek_cards_stats: null output");
    const size_t per = (size_t)h->f * 4;
    for (size_t i = 0; i < h->trajs.size(); ++i)
        CD_HIP(hipMemcpyAsync(stats_out + i * per, h->trajs[i].stats, per * sizeof(int64_t),
                              hipMemcpyDeviceToHost, h->s));
    CD_HIP(hipStreamSynchronize(h->s));
done:
    return rc;
}

extern "C" int ek_cards_disorder(ek_cards *h, const int64_t *lo, const int64_t *hi)
{
    int rc = cd_bind(h, "ek_cards_disorder");
    if (rc != EK_OK)
        return rc;
    if (!lo || !hi)
        return ek_set_error(EK_EARG, "ek_cards_disorder: null argument");
    float ms = 0.f;
    CD_HIP(hipMemcpyAsync(h->lo, lo, (size_t)h->f * sizeof(int64_t), hipMemcpyHostToDevice,
                          h->s));
    CD_HIP(hipMemcpyAsync(h->hi, hi, (size_t)h->f * sizeof(int64_t), hipMemcpyHostToDevice,
                          h->s));
    CD_HIP(hipEventRecord(h->ev[0], h->s));
    for (const cd_traj &t : h->trajs) {
        const int64_t waves = (int64_t)h->f * t.chunks;
        hipLaunchKernelGGL(cd_disorder_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(CD_WG),
                           0, h->s, t.S, (int32_t)t.frames, (int32_t)t.tpad, h->f,
                           (int32_t)t.chunks, t.carry, h->lo, h->hi, t.D);
    }
    CD_HIP(hipEventRecord(h->ev[1], h->s));
    CD_HIP(hipGetLastError());
    CD_HIP(hipStreamSynchronize(h->s));
    CD_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms[2] = ms;
    h->disordered = true;
    h->counted = false;
done:
    return rc;
}

extern "C" int ek_cards_disorder_codes(ek_cards *h, int32_t traj, uint8_t *out)
{
    int rc = cd_bind(h, "ek_cards_disorder_codes");
    if (rc != EK_OK)
        return rc;
    if (!out || traj < 0 || (size_t)traj >= h->trajs.size())
        return ek_set_error(EK_EARG, "ek_cards_disorder_codes: bad argument (trajectory %d of "
                                     "%zu)", traj, h->trajs.size());
    if (!h->disordered)
        return ek_set_error(EK_ESTATE, "ek_cards_disorder_codes: ek_cards_disorder has not run "
                                       "since the last trajectory was added");
    const cd_traj &t = h->trajs[traj];
    const size_t raw_b = (size_t)t.frames * h->f;
    uint8_t *d_raw = nullptr;
    rc = ek_mi_check_memory(raw_b, "ek_cards_disorder_codes");
    if (rc != EK_OK)
        return rc;
    CD_HIP(ek_dev_malloc((void **)&d_raw, raw_b));
    hipLaunchKernelGGL(cd_unpack_kernel, dim3((unsigned)(t.tpad / 64), (h->f + 63) / 64),
                       dim3(CD_WG), 0, h->s, t.D, t.frames, h->f, t.tpad, d_raw);
    CD_HIP(hipGetLastError());
    CD_HIP(hipMemcpyAsync(out, d_raw, raw_b, hipMemcpyDeviceToHost, h->s));
    CD_HIP(hipStreamSynchronize(h->s));
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_raw);
    return rc;
}

extern "C" int ek_cards_matrices(ek_cards *h, double *mi_out)
{
    int rc = cd_bind(h, "ek_cards_matrices");
    if (rc != EK_OK)
        return rc;
    if (!mi_out)
        return ek_set_error(EK_EARG, "ek_cards_matrices: null output");
    if (!h->disordered || h->trajs.empty())
        return ek_set_error(EK_ESTATE, "ek_cards_matrices: no trajectory, or ek_cards_disorder "
                                       "has not run since the last one was added");
    const int64_t pairs = (int64_t)h->f * h->f;
    const int32_t nmax = h->n > 2 ? h->n : 2;
    const int32_t nx[4] = {h->n, 2, h->n, 2}, ny[4] = {h->n, 2, 2, h->n};
    uint32_t *d_col = nullptr;
    double *d_mi = nullptr;
    float ms = 0.f;
    rc = ek_mi_check_memory((size_t)pairs * (nmax * sizeof(uint32_t) + 4 * sizeof(double)),
                            "ek_cards_matrices");
    if (rc != EK_OK)
        return rc;
    CD_HIP(ek_dev_malloc((void **)&d_col, (size_t)pairs * nmax * sizeof(uint32_t)));
    CD_HIP(ek_dev_malloc((void **)&d_mi, (size_t)pairs * 4 * sizeof(double)));
    for (int k = 0; k < 3; ++k)
        CD_HIP(hipMemsetAsync(h->jc[k], 0, cd_cells(h, k) * sizeof(uint32_t), h->s));
    CD_HIP(hipEventRecord(h->ev[0], h->s));
    for (const cd_traj &t : h->trajs)
        ek_mi_launch_count(t.S, t.S, t.tpad, h->f, h->f, h->n, h->n, h->jc[0], h->s);
    CD_HIP(hipEventRecord(h->ev[1], h->s));
    for (const cd_traj &t : h->trajs)
        ek_mi_launch_count(t.D, t.D, t.tpad, h->f, h->f, 2, 2, h->jc[1], h->s);
    CD_HIP(hipEventRecord(h->ev[2], h->s));
    for (const cd_traj &t : h->trajs)
        ek_mi_launch_count(t.S, t.D, t.tpad, h->f, h->f, h->n, 2, h->jc[2], h->s);
    CD_HIP(hipEventRecord(h->ev[3], h->s));
    hipLaunchKernelGGL(cd_transpose_kernel,
                       dim3((unsigned)((cd_cells(h, 3) + CD_WG - 1) / CD_WG)), dim3(CD_WG), 0,
                       h->s, h->jc[2], h->f, h->n, cd_cells(h, 3), h->jc[3]);
    CD_HIP(hipEventRecord(h->ev[4], h->s));
    for (int k = 0; k < 4; ++k)     // (in stream order: the scratch columns are shared)
        ek_mi_launch_info(h->jc[k], pairs, nx[k], ny[k], d_col, d_mi + (size_t)k * pairs, h->s);
    CD_HIP(hipEventRecord(h->ev[5], h->s));
    CD_HIP(hipGetLastError());
    CD_HIP(hipMemcpyAsync(mi_out, d_mi, (size_t)pairs * 4 * sizeof(double),
                          hipMemcpyDeviceToHost, h->s));
    CD_HIP(hipStreamSynchronize(h->s));
    for (int k = 0; k < 5; ++k) {
        CD_HIP(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
        h->ms[3 + k] = ms;
    }
    h->counted = true;
done:
    (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_col);
    (void)ek_dev_free(d_mi);
    return rc;
}

extern "C" int ek_cards_counts(ek_cards *h, int32_t which, uint32_t *jc_out)
{
    int rc = cd_bind(h, "ek_cards_counts");
    if (rc != EK_OK)
        return rc;
    if (!jc_out || which < 0 || which > 3)
        return ek_set_error(EK_EARG, "ek_cards_counts: bad argument (which = 0 .. 3)");
    if (!h->counted)
        return ek_set_error(EK_ESTATE, "ek_cards_counts: ek_cards_matrices has not run");
    CD_HIP(hipMemcpyAsync(jc_out, h->jc[which], cd_cells(h, which) * sizeof(uint32_t),
                          hipMemcpyDeviceToHost, h->s));
    CD_HIP(hipStreamSynchronize(h->s));
done:
    return rc;
}

extern "C" int ek_cards_last_timing(ek_cards *h, double *ms_out)
{
    if (!h || !ms_out)
        return ek_set_error(EK_EARG, "ek_cards_last_timing: null argument");
    for (int i = 0; i < 8; ++i)
        ms_out[i] = h->ms[i];
    return EK_OK;
}

extern "C" int ek_cards_scan_chunk(void)
{
    return CARDS_CHUNK;
}
