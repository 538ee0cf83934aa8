// ek_view.hip -- the active view of a shard: select, build, scatter.
//
// A frame whose stored distance is at most theta cannot be changed by a center that
// is accepted at a distance of 2 theta or more (triangle inequality, DESIGN.md 4a
// "Active view"), so the rounds need not stream it.  The frames above theta are
// compacted, in ascending order of their position, into a second frame store that
// the unchanged round machinery runs on (ek_run_rounds); what it leaves is
// scattered back.  Nothing here computes a distance: coordinates, traces,
// distances and labels are bit copies.
//
//   select   per 1024 frames the count of dist > theta, an exclusive scan of the
//            counts by one workgroup, then every frame's rank = its workgroup's
//            offset + its rank inside: positions ascending, no atomics
//   build    one workgroup per 64 view frames: their frame-major rows
//            through LDS (as ek_prepare_kernel stages them) into the view's
//            quad copy (ek_view_build_kernel); no frame-major copy: the few rows
//            a round reads come from the shard's, through the selection
//            (ek_round_row); the frame-minor tiles only when a kernel that reads
//            them runs under the view (ek_view_tiles_kernel).
//            ek_view_gather_kernel is the earlier form, kept as the reference
//            of ek_view_layout_check
//   look     the policy's counts, theta from the control word on the device: one
//            launch over the store being streamed and, under a view, the shard's
//   scatter  distances and labels back; the centers accepted under the view get
//            their positions in the shard
#include <algorithm>
#include "ek_view.h"

#define EK_VIEW_FPT (EK_VIEW_SEL / EK_BLOCK)    // frames per thread, consecutive
static_assert(EK_VIEW_FPT == 4, "a thread reads its frames' distances as one float4");

// a frame is streamed unless its distance is known to be at most theta
static __device__ __forceinline__ bool ek_view_active(float d, float theta)
{
    return !(d <= theta);
}

static __device__ __forceinline__ unsigned ek_view_flags(const float *__restrict__ dist,
                                                         int64_t f0, int64_t n, float theta)
{
    unsigned m = 0;
    if (f0 + EK_VIEW_FPT <= n) {
        const float4 t = *(const float4 *)(dist + f0);
        m = (ek_view_active(t.x, theta) ? 1u : 0u) | (ek_view_active(t.y, theta) ? 2u : 0u) |
            (ek_view_active(t.z, theta) ? 4u : 0u) | (ek_view_active(t.w, theta) ? 8u : 0u);
    } else {
        for (int q = 0; q < EK_VIEW_FPT; ++q)
            if (f0 + q < n && ek_view_active(dist[f0 + q], theta))
                m |= 1u << q;
    }
    return m;
}

// exclusive prefix sum of v over the workgroup's threads, in thread order; *total =
// the workgroup's sum.  red: EK_BLOCK / EK_WAVE words of LDS.
static __device__ __forceinline__ unsigned ek_view_block_scan(unsigned v, unsigned *red,
                                                              unsigned *total)
{
    const int tid = threadIdx.x, lane = tid & (EK_WAVE - 1), wave = tid / EK_WAVE;
    unsigned inc = v;
#pragma unroll
    for (int off = 1; off < EK_WAVE; off <<= 1) {
        const unsigned o = (unsigned)__shfl_up((int)inc, off, EK_WAVE);
        if (lane >= off)
            inc += o;
    }
    if (lane == EK_WAVE - 1)
        red[wave] = inc;
    __syncthreads();
    unsigned before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < EK_BLOCK / EK_WAVE; ++w) {
        if (w < wave)
            before += red[w];
        sum += red[w];
    }
    __syncthreads();
    *total = sum;
    return before + inc - v;
}

__global__ void __launch_bounds__(EK_BLOCK)
ek_view_count_kernel(const float *__restrict__ dist, int64_t n, float theta,
                     uint32_t *__restrict__ blockcnt)
{
    __shared__ unsigned red[EK_BLOCK / EK_WAVE];
    const int64_t f0 = ((int64_t)blockIdx.x * EK_BLOCK + threadIdx.x) * EK_VIEW_FPT;
    const unsigned m = f0 < n ? ek_view_flags(dist, f0, n, theta) : 0u;
    unsigned total;
    (void)ek_view_block_scan((unsigned)__popc(m), red, &total);
    if (threadIdx.x == 0)
        blockcnt[blockIdx.x] = total;
}

// one workgroup: blockoff = exclusive scan of blockcnt[0 .. nblk), count[0] = the sum
__global__ void __launch_bounds__(EK_BLOCK)
ek_view_scan_kernel(const uint32_t *__restrict__ blockcnt, int nblk,
                    uint32_t *__restrict__ blockoff, uint32_t *__restrict__ count)
{
    __shared__ unsigned red[EK_BLOCK / EK_WAVE];
    const int per = (nblk + EK_BLOCK - 1) / EK_BLOCK;   // consecutive entries per thread
    const int lo = threadIdx.x * per, hi = lo + per < nblk ? lo + per : nblk;
    unsigned mine = 0;
    for (int b = lo; b < hi; ++b)
        mine += blockcnt[b];
    unsigned total;
    unsigned run = ek_view_block_scan(mine, red, &total);
    if (blockoff)
        for (int b = lo; b < hi; ++b) {
            blockoff[b] = run;
            run += blockcnt[b];
        }
    if (threadIdx.x == 0)
        count[0] = total;
}

__global__ void __launch_bounds__(EK_BLOCK)
ek_view_write_kernel(const float *__restrict__ dist, int64_t n, float theta,
                     const uint32_t *__restrict__ blockoff, uint32_t *__restrict__ act,
                     int64_t act_cap)
{
    __shared__ unsigned red[EK_BLOCK / EK_WAVE];
    const int64_t f0 = ((int64_t)blockIdx.x * EK_BLOCK + threadIdx.x) * EK_VIEW_FPT;
    const unsigned m = f0 < n ? ek_view_flags(dist, f0, n, theta) : 0u;
    unsigned total;
    unsigned p = blockoff[blockIdx.x] + ek_view_block_scan((unsigned)__popc(m), red, &total);
#pragma unroll
    for (int q = 0; q < EK_VIEW_FPT; ++q)
        if ((m >> q) & 1u) {
            if (p < act_cap)    // (more than fit: the caller sees it in the count)
                act[p] = (uint32_t)(f0 + q);
            ++p;
        }
}

void ek_launch_view_select(const float *dist, int64_t n, float theta, uint32_t *blockcnt,
                           uint32_t *blockoff, uint32_t *act, int64_t act_cap,
                           uint32_t *count, hipStream_t s)
{
    if (n <= 0) {
        (void)hipMemsetAsync(count, 0, sizeof(uint32_t), s);
        return;
    }
    const unsigned nblk = (unsigned)ek_view_sel_blocks(n);
    hipLaunchKernelGGL(ek_view_count_kernel, dim3(nblk), dim3(EK_BLOCK), 0, s, dist, n,
                       theta, blockcnt);
    hipLaunchKernelGGL(ek_view_scan_kernel, dim3(1), dim3(EK_BLOCK), 0, s, blockcnt,
                       (int)nblk, act ? blockoff : (uint32_t *)nullptr, count);
    if (act)
        hipLaunchKernelGGL(ek_view_write_kernel, dim3(nblk), dim3(EK_BLOCK), 0, s, dist, n,
                           theta, blockoff, act, act_cap);
}

// ---------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------
#define EK_VIEW_CH 16                   // atoms per staged chunk
#define EK_VIEW_ROWF (3 * EK_VIEW_CH + 1)   // LDS row stride in floats (odd: no conflicts)

__global__ void __launch_bounds__(EK_BLOCK)
ek_view_gather_kernel(const uint32_t *__restrict__ act, int64_t n_v, int A,
                      const float *__restrict__ aos, const double *__restrict__ G,
                      const float *__restrict__ dist, const int32_t *__restrict__ assign,
                      float *__restrict__ tiles_v, double *__restrict__ G_v,
                      float *__restrict__ dist_v, int32_t *__restrict__ assign_v)
{
    static_assert(EK_BLOCK == EK_TILE, "one workgroup per tile of the view");
    __shared__ float stage[EK_BLOCK * EK_VIEW_ROWF];
    __shared__ uint32_t src[EK_BLOCK];
    const int t = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * EK_TILE;
    const int64_t p = p0 + t;
    const bool live = p < n_v;
    const int rows_here = (int)((n_v - p0 < EK_TILE) ? (n_v - p0) : EK_TILE);
    const uint32_t f = live ? act[p] : 0u;
    src[t] = f;
    if (live) {
        G_v[p] = G[f];
        dist_v[p] = dist[f];
        assign_v[p] = assign[f];
    }
    __syncthreads();
    const size_t A3 = (size_t)3 * A;
    float *tile = tiles_v + (size_t)blockIdx.x * A3 * EK_TILE + t;
    for (int a0 = 0; a0 < A; a0 += EK_VIEW_CH) {
        const int w = 3 * ((A - a0 < EK_VIEW_CH) ? (A - a0) : EK_VIEW_CH);
        const int total = rows_here * w;
        // a frame's piece of the chunk is 12 * CH contiguous bytes of its row
        for (int i = t; i < total; i += EK_BLOCK) {
            const int r = i / w, j = i % w;
            stage[r * EK_VIEW_ROWF + j] = aos[(size_t)src[r] * A3 + 3 * a0 + j];
        }
        __syncthreads();
        // frame-minor: 1 KiB per (atom, axis) row of the tile; zeros in the slots
        // of padding
        const float *row = stage + t * EK_VIEW_ROWF;
        for (int j = 0; j < w; ++j)
            tile[(size_t)(3 * a0 + j) * EK_TILE] = live ? row[j] : 0.f;
        __syncthreads();
    }
}

void ek_launch_view_gather(const uint32_t *act, int64_t n_v, int A, const float *aos,
                           const double *G, const float *dist, const int32_t *assign,
                           float *tiles_v, double *G_v, float *dist_v, int32_t *assign_v,
                           hipStream_t s)
{
    if (n_v <= 0)
        return;
    const unsigned tiles = (unsigned)((n_v + EK_TILE - 1) / EK_TILE);
    hipLaunchKernelGGL(ek_view_gather_kernel, dim3(tiles), dim3(EK_BLOCK), 0, s, act, n_v, A,
                       aos, G, dist, assign, tiles_v, G_v, dist_v, assign_v);
}

// ---------------------------------------------------------------------------
// build: the gather of a rebuild.  From the staged rows the view's QUAD copy (the
// layout above ek_quad_tiles_kernel, ek_pass16.hip) instead of its frame-minor tiles:
// a rebuild then moves a frame twice (one read, one write), not five times.  Without
// a quad copy in the context (QUAD = false: rounds of 8 at most) the frame-minor
// tiles, as ek_view_gather_kernel writes them.
//
// A workgroup owns the 64 frames of one wave of a tile -- the quad copy keeps them
// together: slots 64 w .. 64 w + 63 of every (trip, coordinate) -- and stages them in
// chunks of 64 atoms: a row's piece is 768 contiguous bytes, six cache lines, where
// the 192 bytes of ek_view_gather_kernel share a line with the next chunk more often
// than not.  VEC = 4 (A % 4 == 0: every row and every chunk starts on 16 bytes): 16
// lanes per row, three 16-byte loads each, 16 rows per sweep of the workgroup; VEC =
// 1: 64 lanes per row, three 4-byte loads each, 4 rows per sweep.  No division: a
// thread's row and column are shifts of its id.
// ---------------------------------------------------------------------------
#define EK_VIEW_BROWS 64                        // frames per workgroup
#define EK_VIEW_BCH 64                          // atoms per staged chunk
#define EK_VIEW_BROWF (3 * EK_VIEW_BCH + 1)     // LDS row stride in floats (odd)
typedef float ek_view_v4f __attribute__((ext_vector_type(4)));

template <int VEC> struct EkViewVec;
template <> struct EkViewVec<4> { typedef ek_view_v4f T; };
template <> struct EkViewVec<1> { typedef float T; };

template <int VEC, bool QUAD>
__global__ void __launch_bounds__(EK_BLOCK)
ek_view_build_kernel(const uint32_t *__restrict__ act, int64_t n_v, int A,
                     const float *__restrict__ aos, const double *__restrict__ G,
                     const float *__restrict__ dist, const int32_t *__restrict__ assign,
                     float *__restrict__ out_v, double *__restrict__ G_v,
                     float *__restrict__ dist_v, int32_t *__restrict__ assign_v)
{
    static_assert(EK_BLOCK == 256 && EK_TILE == 256 && EK_WAVE == 64,
                  "four workgroups per tile of the view, one per wave of the pass");
    typedef typename EkViewVec<VEC>::T vec_t;
    constexpr int LPR = EK_VIEW_BCH / VEC;      // lanes per row: 3 * LPR elements of VEC floats
    constexpr int RPS = EK_BLOCK / LPR;         // rows per sweep
    constexpr int SWEEPS = EK_VIEW_BROWS / RPS;
    __shared__ float stage[EK_VIEW_BROWS * EK_VIEW_BROWF];
    __shared__ uint32_t src[EK_VIEW_BROWS];
    const int t = threadIdx.x;
    const size_t tile = blockIdx.x >> 2;
    const int qw = blockIdx.x & 3;              // the wave of the tile
    const int64_t p0 = (int64_t)tile * EK_TILE + EK_VIEW_BROWS * qw;
    const int rows_here =
        (int)(n_v - p0 >= EK_VIEW_BROWS ? EK_VIEW_BROWS : (n_v > p0 ? n_v - p0 : 0));
    if (t < EK_VIEW_BROWS) {
        const int64_t p = p0 + t;
        const uint32_t f = t < rows_here ? act[p] : 0u;
        src[t] = f;
        if (t < rows_here) {
            G_v[p] = G[f];
            dist_v[p] = dist[f];
            assign_v[p] = assign[f];
        }
    }
    __syncthreads();
    const size_t A3 = (size_t)3 * A;
    const int NQ = (A + 3) / 4;
    const int jl = t & (LPR - 1), r0 = t / LPR;
    // the quad copy's slot of this thread: atom e of a trip, frame f16 of a group; the
    // workgroup's four waves share the (trip, coordinate) rows of a chunk
    const int slot = t & 63, wv = t >> 6, qe = slot >> 4, qf = slot & 15;
    for (int a0 = 0; a0 < A; a0 += EK_VIEW_BCH) {
        const int w = 3 * ((A - a0 < EK_VIEW_BCH) ? (A - a0) : EK_VIEW_BCH);
        const int we = w / VEC;     // (VEC = 4: A - a0 is a multiple of 4, so is w)
        vec_t v[SWEEPS][3];
#pragma unroll
        for (int it = 0; it < SWEEPS; ++it) {
            const int r = r0 + it * RPS;
            const vec_t *s = (const vec_t *)(aos + (size_t)src[r] * A3 + 3 * a0);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int j = jl + m * LPR;
                if (r < rows_here && j < we)
                    v[it][m] = s[j];
            }
        }
#pragma unroll
        for (int it = 0; it < SWEEPS; ++it) {
            const int r = r0 + it * RPS;
            float *st = stage + r * EK_VIEW_BROWF;
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                const int j = jl + m * LPR;
                if (r < rows_here && j < we) {
                    if constexpr (VEC == 4) {
#pragma unroll
                        for (int x = 0; x < 4; ++x)
                            st[4 * j + x] = v[it][m][x];
                    } else {
                        st[j] = v[it][m];
                    }
                }
            }
        }
        __syncthreads();
        if constexpr (QUAD) {
            // slot 64 qw + slot of (trip q, coordinate k): frames 16 g + qf of this
            // wave's 64, atom 4 q + qe; zeros for the atoms past the last and the
            // frames of padding
            ek_view_v4f *dst = (ek_view_v4f *)out_v + tile * (size_t)NQ * 3 * EK_TILE +
                               EK_VIEW_BROWS * qw + slot;
            for (int qq = wv; qq < EK_VIEW_BCH / 4; qq += EK_BLOCK / EK_WAVE) {
                const int q = a0 / 4 + qq;
                if (q >= NQ)
                    break;
                const bool atom = 4 * q + qe < A;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    ek_view_v4f o;
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int fr = 16 * g + qf;
                        o[g] = (atom && fr < rows_here)
                                   ? stage[fr * EK_VIEW_BROWF + 3 * (4 * qq + qe) + k] : 0.f;
                    }
                    dst[(size_t)(q * 3 + k) * EK_TILE] = o;
                }
            }
        } else {
            // frame-minor: this wave's 256 bytes of every (atom, axis) row of the tile;
            // zeros in the slots of padding
            float *tp = out_v + tile * A3 * EK_TILE + EK_VIEW_BROWS * qw + slot;
            const float *row = stage + slot * EK_VIEW_BROWF;
            for (int j = wv; j < w; j += EK_BLOCK / EK_WAVE)
                tp[(size_t)(3 * a0 + j) * EK_TILE] = slot < rows_here ? row[j] : 0.f;
        }
        __syncthreads();
    }
}

void ek_launch_view_build(const uint32_t *act, int64_t n_v, int A, bool quad, const float *aos,
                          const double *G, const float *dist, const int32_t *assign,
                          float *out_v, double *G_v, float *dist_v, int32_t *assign_v,
                          hipStream_t s)
{
    if (n_v <= 0)
        return;
    const unsigned tiles = (unsigned)((n_v + EK_TILE - 1) / EK_TILE);
#define EK_VIEW_BUILD(VEC, QUAD)                                                          \
    hipLaunchKernelGGL((ek_view_build_kernel<VEC, QUAD>), dim3(4 * tiles), dim3(EK_BLOCK), 0, \
                       s, act, n_v, A, aos, G, dist, assign, out_v, G_v, dist_v, assign_v)
    if (A % 4 == 0) {
        if (quad)
            EK_VIEW_BUILD(4, true);
        else
            EK_VIEW_BUILD(4, false);
    } else {
        if (quad)
            EK_VIEW_BUILD(1, true);
        else
            EK_VIEW_BUILD(1, false);
    }
#undef EK_VIEW_BUILD
}

// the frame-minor tiles of a view from its quad copy (the inverse of
// ek_quad_tiles_kernel): a bit copy; the frames of padding are zeros there and here
__global__ void __launch_bounds__(EK_BLOCK)
ek_view_tiles_kernel(const float *__restrict__ qtiles, int A, int NQ,
                     float *__restrict__ tiles)
{
    const int l = threadIdx.x;
    const int w = l >> 6, e = (l >> 4) & 3, f16 = l & 15;
    const size_t tile = blockIdx.x;
    const ek_view_v4f *src = (const ek_view_v4f *)qtiles + tile * (size_t)NQ * 3 * EK_TILE + l;
    float *dst = tiles + tile * 3 * (size_t)A * EK_TILE + 64 * w + f16;
    for (int q = blockIdx.y; q < NQ; q += gridDim.y) {
        const int a = 4 * q + e;
        if (a >= A)
            continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const ek_view_v4f v = src[(size_t)(q * 3 + k) * EK_TILE];
#pragma unroll
            for (int g = 0; g < 4; ++g)
                dst[(size_t)(3 * a + k) * EK_TILE + 16 * g] = v[g];
        }
    }
}

void ek_launch_view_tiles(const float *qtiles, int64_t n_tiles, int A, float *tiles,
                          hipStream_t s)
{
    if (n_tiles <= 0)
        return;
    const int NQ = (A + 3) / 4;
    const unsigned gy = (unsigned)std::max<int64_t>(
        1, std::min<int64_t>(NQ, 2048 / std::max<int64_t>(n_tiles, 1)));
    hipLaunchKernelGGL(ek_view_tiles_kernel, dim3((unsigned)n_tiles, gy), dim3(EK_BLOCK), 0, s,
                       qtiles, A, NQ, tiles);
}

// ---------------------------------------------------------------------------
// look: how many frames a view built now would hold, for the policy.  theta from the
// maximum the batch left on the device (the host's formula and rounding, ek_api.hip);
// one atomic per workgroup, a count needs no order.  An estimate only: a view is
// always built from a theta the host computed.
//
// One grid counts both arrays: its first blocks(n) workgroups the store being streamed
// into mine[0], the rest (under a view) the shard's own distances into mine[1].  The
// words of the look before, `other`, were read by the host before it enqueued this
// one: they are zeroed here for the look after, so no look needs a fill of its own.
// ---------------------------------------------------------------------------
#define EK_VIEW_LOOK_SEL (8 * EK_VIEW_SEL)     // frames per workgroup of the look
static inline unsigned ek_view_look_blocks(int64_t n)
{
    return n > 0 ? (unsigned)((n + EK_VIEW_LOOK_SEL - 1) / EK_VIEW_LOOK_SEL) : 0u;
}

__global__ void __launch_bounds__(EK_BLOCK)
ek_view_look_kernel(const float *__restrict__ dist_a, int64_t n_a, unsigned blocks_a,
                    const float *__restrict__ dist_b, int64_t n_b,
                    const EkCtl *__restrict__ ctl, double rho, double rel, double abs_,
                    uint32_t *__restrict__ mine_cnt, uint32_t *__restrict__ other)
{
    __shared__ unsigned red[EK_BLOCK / EK_WAVE];
    if (blockIdx.x == 0 && threadIdx.x == 0)
        other[0] = other[1] = 0u;
    const bool second = blockIdx.x >= blocks_a;     // uniform
    const float *__restrict__ dist = second ? dist_b : dist_a;
    const int64_t n = second ? n_b : n_a;
    const int64_t blk = second ? blockIdx.x - blocks_a : blockIdx.x;
    uint32_t *count = mine_cnt + (second ? 1 : 0);
    const double th = (rho * (double)ctl->last_max - abs_) / (2.0 * (1.0 + rel));
    float theta = (float)th;
    if ((double)theta > th && theta > 0.f)      // (down; at or below zero nobody looks)
        theta = __uint_as_float(__float_as_uint(theta) - 1u);
    // (EK_VIEW_LOOK_SEL frames per workgroup: a thousand atomics on one word took
    // longer than the read)
    unsigned mine = 0;
#pragma unroll
    for (int q = 0; q < EK_VIEW_LOOK_SEL / EK_VIEW_SEL; ++q) {
        const int64_t f0 = ((blk * (EK_VIEW_LOOK_SEL / EK_VIEW_SEL) + q) * EK_BLOCK +
                            threadIdx.x) * EK_VIEW_FPT;
        mine += f0 < n ? (unsigned)__popc(ek_view_flags(dist, f0, n, theta)) : 0u;
    }
    unsigned total;
    (void)ek_view_block_scan(mine, red, &total);
    if (threadIdx.x == 0 && total)
        atomicAdd(count, total);
}

void ek_launch_view_look(const float *dist, int64_t n, const float *shard_dist,
                         int64_t shard_n, const EkCtl *ctl, double rho, double rel,
                         double abs_, uint32_t *count, int parity, hipStream_t s)
{
    if (!shard_dist)
        shard_n = 0;
    // (never an empty grid: the zeroing of the other parity's words is this launch's too)
    const unsigned blocks_a = std::max(1u, ek_view_look_blocks(n));
    hipLaunchKernelGGL(ek_view_look_kernel, dim3(blocks_a + ek_view_look_blocks(shard_n)),
                       dim3(EK_BLOCK), 0, s, dist, std::max<int64_t>(n, 0), blocks_a, shard_dist,
                       shard_n, ctl, rho, rel, abs_, count + 2 * (parity & 1),
                       count + 2 * ((parity & 1) ^ 1));
}

// words of a[0 .. n) and b[0 .. n) that differ, added to *count (ek_view_layout_check)
__global__ void __launch_bounds__(EK_BLOCK)
ek_view_diff_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, size_t n,
                    unsigned long long *__restrict__ count)
{
    unsigned mine = 0;
    for (size_t i = (size_t)blockIdx.x * EK_BLOCK + threadIdx.x; i < n;
         i += (size_t)gridDim.x * EK_BLOCK)
        mine += a[i] != b[i] ? 1u : 0u;
    if (mine)
        atomicAdd(count, (unsigned long long)mine);
}

void ek_launch_view_diff(const void *a, const void *b, size_t words,
                         unsigned long long *count, hipStream_t s)
{
    if (words == 0)
        return;
    const unsigned blocks =
        (unsigned)std::min<size_t>((words + EK_BLOCK - 1) / EK_BLOCK, (size_t)4096);
    hipLaunchKernelGGL(ek_view_diff_kernel, dim3(blocks), dim3(EK_BLOCK), 0, s,
                       (const uint32_t *)a, (const uint32_t *)b, words, count);
}

// ---------------------------------------------------------------------------
// scatter
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(EK_BLOCK)
ek_view_scatter_kernel(const uint32_t *__restrict__ act, int64_t n_v,
                       const float *__restrict__ dist_v,
                       const int32_t *__restrict__ assign_v, float *__restrict__ dist,
                       int32_t *__restrict__ assign, EkHist *__restrict__ hist,
                       int32_t label_lo, int32_t label_cap, const EkCtl *__restrict__ ctl,
                       int64_t goff)
{
    const int64_t p = (int64_t)blockIdx.x * EK_BLOCK + threadIdx.x;
    if (p < n_v) {
        const uint32_t f = act[p];
        dist[f] = dist_v[p];
        assign[f] = assign_v[p];
    }
    // the centers of this view (a few thousand at most): a stride over the grid
    int32_t hi = ctl->n_done;
    if (hi > label_cap)
        hi = label_cap;
    for (int64_t l = label_lo + p; l < hi; l += (int64_t)gridDim.x * EK_BLOCK) {
        const int64_t q = hist[l].gidx - goff;
        if (hist[l].set && q >= 0 && q < n_v)
            hist[l].gidx = goff + (int64_t)act[q];
    }
}

void ek_launch_view_scatter(const uint32_t *act, int64_t n_v, const float *dist_v,
                            const int32_t *assign_v, float *dist, int32_t *assign,
                            EkHist *hist, int32_t label_lo, int32_t label_cap,
                            const EkCtl *ctl, int64_t goff, hipStream_t s)
{
    if (n_v <= 0)
        return;
    hipLaunchKernelGGL(ek_view_scatter_kernel,
                       dim3((unsigned)((n_v + EK_BLOCK - 1) / EK_BLOCK)), dim3(EK_BLOCK), 0,
                       s, act, n_v, dist_v, assign_v, dist, assign, hist, label_lo,
                       label_cap, ctl, goff);
}
