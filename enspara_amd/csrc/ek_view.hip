// ek_view.hip -- the active view of a shard: select, gather, scatter.
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
//   gather   one workgroup per tile of 256 view frames: their frame-major rows
//            through LDS (as ek_prepare_kernel stages them) into the view's
//            frame-major copy and its frame-minor tile
//   scatter  distances and labels back; the centers accepted under the view get
//            their positions in the shard
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
                      float *__restrict__ aos_v, float *__restrict__ tiles_v,
                      double *__restrict__ G_v, float *__restrict__ dist_v,
                      int32_t *__restrict__ assign_v)
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
            const float v = aos[(size_t)src[r] * A3 + 3 * a0 + j];
            stage[r * EK_VIEW_ROWF + j] = v;
            aos_v[(size_t)(p0 + r) * A3 + 3 * a0 + j] = v;
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
                           float *aos_v, float *tiles_v, double *G_v, float *dist_v,
                           int32_t *assign_v, hipStream_t s)
{
    if (n_v <= 0)
        return;
    const unsigned tiles = (unsigned)((n_v + EK_TILE - 1) / EK_TILE);
    hipLaunchKernelGGL(ek_view_gather_kernel, dim3(tiles), dim3(EK_BLOCK), 0, s, act, n_v, A,
                       aos, G, dist, assign, aos_v, tiles_v, G_v, dist_v, assign_v);
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
