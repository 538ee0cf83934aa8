// ek_pockets.hip -- LIGSITE pocket detection on the device.
//
// Replaces the reference's enspara/geometry/pockets.py: a grid over every frame, the
// cells within probe + radius of an atom "touch", seven scans rank the others, the cells
// of rank >= min_rank are the pocket cells, contiguous ones form a pocket.
//
// The contract, float64, nothing fused:
//   cell     = double(origin) + double(i) * spacing per axis, flat (ix * ny + iy) * nz + iz
//   touches  iff for some atom (dx*dx + dy*dy) + dz*dz < cutoff * cutoff, d = cell - double(x)
//   rank     = over the directions (1,0,0) (0,1,0) (0,0,1) (1,1,1) (-1,1,1) (-1,-1,1)
//              (1,-1,1), the lines on which the cell does not touch and lies strictly
//              between the first and the last touching cell
//   quirk    a diagonal line whose first cell has x and y on their start faces and z >= 1
//            is not scanned: the reference enumerates a diagonal's lines from three faces
//            and misses the edge the three share
//   pockets  components of the cells with rank >= min_rank under 18-connectivity, labelled
//            by their smallest flat index
//
// One chunk of frames at a time, every stage one launch over the whole chunk (grid.y =
// frame), so the number of launches does not depend on the frames:
//   touch    a wave per (frame, atom), its lanes over the atom's box of cells, clipped to
//            the grid; plain byte stores of 1 (idempotent)
//   extent   a lane per (frame, direction, line): first and last touching position, 16
//            bits each, "none" = (POCK_NONE, 0).  A line is an arithmetic progression of
//            flat indices.  The lines of x and y are indexed (., iz) and those of a
//            diagonal (x' - y', z - y') with x', y' counted from the start faces, so that
//            neighbouring lanes read neighbouring z; position = the coordinate walked for
//            x, y, z and z for the diagonals
//   rank     a lane per cell: seven look-ups first < pos < last; writes the cell's parent
//            (itself, or -1 below min_rank) for the labelling
//   union    a lane per pocket cell: unite with the 9 of its 18 neighbours that have a
//            larger flat index.  Roots only ever get a smaller parent (atomicMin), so
//            find terminates and a component's root is its smallest index whatever the
//            order of the merges
//   flatten  parent = root
//   compact  count per 256 cells, one-workgroup scan of the counts, ordered write of
//            (cell, root): ascending by frame and flat index
#include "ek_common.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <new>

extern int ek_set_error(int code, const char *fmt, ...);
int ek_mi_check_memory(size_t bytes, const char *who);

#define POCK_TRY(call)                                                         \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess)                                                  \
            return ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,      \
                                hipGetErrorString(e_), __FILE__, __LINE__);    \
    } while (0)

#define POCK_WG 256
#define POCK_MAX_AXIS 2048                  // cells along an axis (geometry.pockets.MAX_AXIS)
#define POCK_MAX_CELLS (1 << 26)            // of one frame (geometry.pockets.MAX_CELLS)
#define POCK_MAX_CHUNK_CELLS ((int64_t)1 << 30)     // of one chunk: parents are int32
#define POCK_MAX_FRAMES 32768               // of one chunk: grid.y
#define POCK_NONE 0x7fffu                   // "first" of a line without a touching cell

struct PockFrame {
    double ox, oy, oz;          // double(origin)
    int32_t nx, ny, nz;
    int32_t cell_off;           // the frame's first cell within the chunk
    int64_t line_off;           // ... first line extent
};

struct ek_pockets {
    int device;
    int32_t atoms, min_rank;
    double spacing;
    double *cutoff, *cutoff2;   // [atoms] probe + radius, and its square
    hipStream_t s;
    hipEvent_t ev[5];
    double ms[4];               // upload, touch, extent + rank, label + compact
    // the last run's result (host)
    int64_t frames, total;
    int64_t *counts;            // [frames]
    int32_t *cells, *labels;    // [total]
};

// buffers of one chunk (or of a single-stage call)
struct PockDev {
    float *xyz = nullptr;
    PockFrame *fr = nullptr;
    uint8_t *touch = nullptr, *rank = nullptr;
    uint32_t *ext = nullptr;
    int32_t *parent = nullptr;
    int32_t *bcnt = nullptr, *boff = nullptr, *total = nullptr;
    int32_t *out = nullptr;     // [2][out_cap]: cells, then roots
    size_t out_cap = 0;
};

static void pock_dev_free(PockDev &d)
{
    (void)ek_dev_free(d.xyz);
    (void)ek_dev_free(d.fr);
    (void)ek_dev_free(d.touch);
    (void)ek_dev_free(d.rank);
    (void)ek_dev_free(d.ext);
    (void)ek_dev_free(d.parent);
    (void)ek_dev_free(d.bcnt);
    (void)ek_dev_free(d.boff);
    (void)ek_dev_free(d.total);
    (void)ek_dev_free(d.out);
    d = PockDev();
}

static inline __host__ __device__ int32_t pock_dir_lines(int nx, int ny, int nz, int dir)
{
    if (nx < 1 || ny < 1 || nz < 1)
        return 0;
    switch (dir) {
    case 0: return ny * nz;
    case 1: return nx * nz;
    case 2: return nx * ny;
    default: return (nx + ny - 1) * (ny + nz - 1);
    }
}

static inline __host__ __device__ int64_t pock_dir_off(int nx, int ny, int nz, int dir)
{
    int64_t o = 0;
    for (int d = 0; d < dir; ++d)
        o += pock_dir_lines(nx, ny, nz, d);
    return o;
}

// ---- touch ---------------------------------------------------------------------------
__global__ void __launch_bounds__(POCK_WG)
pock_touch_kernel(const float *__restrict__ xyz, int32_t atoms, const double *__restrict__ cutoff,
                  const double *__restrict__ cutoff2, double spacing,
                  const PockFrame *__restrict__ fr, uint8_t *__restrict__ touch)
{
    const int lane = threadIdx.x & (EK_WAVE - 1);
    const int32_t a = (int32_t)blockIdx.x * (POCK_WG / EK_WAVE) + (int32_t)(threadIdx.x / EK_WAVE);
    if (a >= atoms)
        return;
    const PockFrame F = fr[blockIdx.y];
    if (F.nx < 1 || F.ny < 1 || F.nz < 1)
        return;
    const float *X = xyz + ((size_t)blockIdx.y * atoms + a) * 3;
    const double x[3] = {(double)X[0], (double)X[1], (double)X[2]};
    const double o[3] = {F.ox, F.oy, F.oz};
    const int32_t n[3] = {F.nx, F.ny, F.nz};
    const double c = cutoff[a], c2 = cutoff2[a];
    // the cull: a cell within c of the atom along an axis has (x - c - o) / spacing < i <
    // (x + c - o) / spacing there; one cell more on either side covers the rounding, and
    // the clamp in float64 comes before the conversion, which then cannot overflow
    int32_t lo[3], b[3];
    for (int k = 0; k < 3; ++k) {
        const double l = fmax(floor((x[k] - c - o[k]) / spacing) - 1.0, 0.0);
        const double h = fmin(ceil((x[k] + c - o[k]) / spacing) + 1.0, (double)(n[k] - 1));
        if (!(l <= h))
            return;
        lo[k] = (int32_t)l;
        b[k] = (int32_t)h - lo[k] + 1;
    }
    uint8_t *T = touch + F.cell_off;
    const int32_t vol = b[0] * b[1] * b[2];        // <= the frame's cells <= 2^26
    for (int32_t k = lane; k < vol; k += EK_WAVE) {
        const int32_t iz = lo[2] + k % b[2];
        const int32_t iy = lo[1] + (k / b[2]) % b[1];
        const int32_t ix = lo[0] + k / (b[2] * b[1]);
        const double dx = (o[0] + (double)ix * spacing) - x[0];
        const double dy = (o[1] + (double)iy * spacing) - x[1];
        const double dz = (o[2] + (double)iz * spacing) - x[2];
        if ((dx * dx + dy * dy) + dz * dz < c2)
            T[((size_t)ix * n[1] + iy) * n[2] + iz] = 1;
    }
}

// ---- line extents --------------------------------------------------------------------
static inline __device__ void pock_diag_signs(int dir, int &sx, int &sy)
{
    sx = (dir == 3 || dir == 6) ? 1 : -1;
    sy = (dir == 3 || dir == 4) ? 1 : -1;
}

__global__ void __launch_bounds__(POCK_WG)
pock_extent_kernel(const PockFrame *__restrict__ fr, const uint8_t *__restrict__ touch,
                   uint32_t *__restrict__ ext)
{
    const PockFrame F = fr[blockIdx.y];
    const int dir = (int)blockIdx.z;
    const int32_t nx = F.nx, ny = F.ny, nz = F.nz;
    const int32_t t = (int32_t)blockIdx.x * POCK_WG + (int32_t)threadIdx.x;
    if (t >= pock_dir_lines(nx, ny, nz, dir))
        return;
    const uint8_t *T = touch + F.cell_off;
    // the line's cells are start + k * stride, k < n, at positions pos0 + k
    int32_t start, stride, n, pos0 = 0;
    if (dir == 0) {
        start = t;                      // (iy, iz)
        stride = ny * nz;
        n = nx;
    } else if (dir == 1) {
        start = (t / nz) * ny * nz + t % nz;    // (ix, iz)
        stride = nz;
        n = ny;
    } else if (dir == 2) {
        start = t * nz;                 // (ix, iy)
        stride = 1;
        n = nz;
    } else {
        int sx, sy;
        pock_diag_signs(dir, sx, sy);
        const int32_t W = ny + nz - 1;
        const int32_t p = t / W - (ny - 1), q = t % W - (ny - 1);   // x' - y', z - y'
        const int32_t t0 = max(0, max(-p, -q));
        const int32_t t1 = min(ny - 1, min(nx - 1 - p, nz - 1 - q));
        n = t1 - t0 + 1;                // (<= 0: no cell has this (p, q))
        if (t0 == 0 && p == 0 && q >= 1)
            n = 0;                      // the reference never scans these
        const int32_t xf = p + t0, yf = t0, z = q + t0;
        const int32_t x = sx > 0 ? xf : nx - 1 - xf, y = sy > 0 ? yf : ny - 1 - yf;
        start = (x * ny + y) * nz + z;
        stride = sx * ny * nz + sy * nz + 1;
        pos0 = z;
    }
    uint32_t first = POCK_NONE, last = 0;
    for (int32_t k = 0; k < n; ++k)
        if (T[start + k * stride]) {
            first = (uint32_t)(pos0 + k);
            break;
        }
    if (first != POCK_NONE)
        for (int32_t k = n - 1; k >= 0; --k)
            if (T[start + k * stride]) {
                last = (uint32_t)(pos0 + k);
                break;
            }
    ext[F.line_off + pock_dir_off(nx, ny, nz, dir) + t] = first | (last << 16);
}

// ---- rank ----------------------------------------------------------------------------
__global__ void __launch_bounds__(POCK_WG)
pock_rank_kernel(const PockFrame *__restrict__ fr, const uint8_t *__restrict__ touch,
                 const uint32_t *__restrict__ ext, int32_t min_rank,
                 uint8_t *__restrict__ rank_out, int32_t *__restrict__ parent_out)
{
    const PockFrame F = fr[blockIdx.y];
    const int32_t nx = F.nx, ny = F.ny, nz = F.nz;
    const int64_t c64 = (int64_t)blockIdx.x * POCK_WG + threadIdx.x;
    if (nx < 1 || ny < 1 || nz < 1 || c64 >= (int64_t)nx * ny * nz)
        return;
    const int32_t c = (int32_t)c64;
    const int32_t iz = c % nz, iy = (c / nz) % ny, ix = c / (nz * ny);
    int32_t r = 0;
    if (!touch[F.cell_off + c]) {
        const uint32_t *E = ext + F.line_off;
        int64_t off = 0;
        for (int dir = 0; dir < 7; ++dir) {
            int32_t line, pos;
            if (dir == 0) {
                line = iy * nz + iz;
                pos = ix;
            } else if (dir == 1) {
                line = ix * nz + iz;
                pos = iy;
            } else if (dir == 2) {
                line = ix * ny + iy;
                pos = iz;
            } else {
                int sx, sy;
                pock_diag_signs(dir, sx, sy);
                const int32_t xf = sx > 0 ? ix : nx - 1 - ix, yf = sy > 0 ? iy : ny - 1 - iy;
                line = (xf - yf + ny - 1) * (ny + nz - 1) + (iz - yf + ny - 1);
                pos = iz;
            }
            const uint32_t e = E[off + line];
            r += ((int32_t)(e & 0xffffu) < pos && pos < (int32_t)(e >> 16)) ? 1 : 0;
            off += pock_dir_lines(nx, ny, nz, dir);
        }
    }
    if (rank_out)
        rank_out[F.cell_off + c] = (uint8_t)r;
    if (parent_out)
        parent_out[F.cell_off + c] = (r >= min_rank) ? F.cell_off + c : -1;
}

// ---- label ---------------------------------------------------------------------------
__global__ void __launch_bounds__(POCK_WG)
pock_mask_kernel(const uint8_t *__restrict__ mask, int32_t cells, int32_t *__restrict__ parent)
{
    const int64_t c = (int64_t)blockIdx.x * POCK_WG + threadIdx.x;
    if (c < cells)
        parent[c] = mask[c] ? (int32_t)c : -1;
}

static inline __device__ int32_t pock_find(int32_t *parent, int32_t x)
{
    int32_t p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
    while (p != x) {        // (parents only decrease: this ends at a root)
        x = p;
        p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
    }
    return x;
}

static inline __device__ void pock_unite(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = pock_find(parent, a);
        b = pock_find(parent, b);
        if (a == b)
            return;
        if (a < b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        // the larger root goes under the smaller.  If a was no root any more (old != a)
        // it pointed at old: whichever of old and b the minimum kept, the other is still
        // to be united with it
        const int32_t old = atomicMin(&parent[a], b);
        if (old == a)
            return;
        a = old;
    }
}

__global__ void __launch_bounds__(POCK_WG)
pock_union_kernel(const PockFrame *__restrict__ fr, int32_t *__restrict__ parent)
{
    const PockFrame F = fr[blockIdx.y];
    const int32_t nx = F.nx, ny = F.ny, nz = F.nz;
    const int64_t c64 = (int64_t)blockIdx.x * POCK_WG + threadIdx.x;
    if (nx < 1 || ny < 1 || nz < 1 || c64 >= (int64_t)nx * ny * nz)
        return;
    const int32_t c = (int32_t)c64, g = F.cell_off + c;
    if (__atomic_load_n(&parent[g], __ATOMIC_RELAXED) < 0)
        return;
    const int32_t iz = c % nz, iy = (c / nz) % ny, ix = c / (nz * ny);
    // the 9 of the 18 face and edge neighbours with a larger flat index
    const int8_t nb[9][3] = {{0, 0, 1}, {0, 1, -1}, {0, 1, 0}, {0, 1, 1}, {1, -1, 0},
                             {1, 0, -1}, {1, 0, 0}, {1, 0, 1}, {1, 1, 0}};
    for (int k = 0; k < 9; ++k) {
        const int32_t x = ix + nb[k][0], y = iy + nb[k][1], z = iz + nb[k][2];
        if (x >= nx || y < 0 || y >= ny || z < 0 || z >= nz)
            continue;
        const int32_t h = F.cell_off + (x * ny + y) * nz + z;
        if (__atomic_load_n(&parent[h], __ATOMIC_RELAXED) >= 0)
            pock_unite(parent, g, h);
    }
}

__global__ void __launch_bounds__(POCK_WG)
pock_flatten_kernel(const PockFrame *__restrict__ fr, int32_t *__restrict__ parent)
{
    const PockFrame F = fr[blockIdx.y];
    const int64_t c64 = (int64_t)blockIdx.x * POCK_WG + threadIdx.x;
    if (F.nx < 1 || F.ny < 1 || F.nz < 1 || c64 >= (int64_t)F.nx * F.ny * F.nz)
        return;
    const int32_t g = F.cell_off + (int32_t)c64;
    if (__atomic_load_n(&parent[g], __ATOMIC_RELAXED) < 0)
        return;
    __atomic_store_n(&parent[g], pock_find(parent, g), __ATOMIC_RELAXED);
}

// ---- compact -------------------------------------------------------------------------
__global__ void __launch_bounds__(POCK_WG)
pock_count_kernel(const int32_t *__restrict__ parent, int32_t cells, int32_t *__restrict__ bcnt)
{
    __shared__ int32_t wc[POCK_WG / EK_WAVE];
    const int64_t g = (int64_t)blockIdx.x * POCK_WG + threadIdx.x;
    const bool keep = g < cells && parent[g] >= 0;
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & (EK_WAVE - 1)) == 0)
        wc[threadIdx.x / EK_WAVE] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t s = 0;
        for (int w = 0; w < POCK_WG / EK_WAVE; ++w)
            s += wc[w];
        bcnt[blockIdx.x] = s;
    }
}

#define POCK_SCAN_WG 1024
__global__ void __launch_bounds__(POCK_SCAN_WG)
pock_scan_kernel(const int32_t *__restrict__ bcnt, int32_t nb, int32_t *__restrict__ boff,
                 int32_t *__restrict__ total)
{
    __shared__ int32_t wsum[POCK_SCAN_WG / EK_WAVE];
    const int tid = threadIdx.x, lane = tid & (EK_WAVE - 1), wave = tid / EK_WAVE;
    int32_t carry = 0;
    for (int32_t base = 0; base < nb; base += POCK_SCAN_WG) {
        const int32_t i = base + tid;
        const int32_t v = (i < nb) ? bcnt[i] : 0;
        int32_t s = v;
        for (int d = 1; d < EK_WAVE; d <<= 1) {
            const int32_t u = __shfl_up(s, d);
            if (lane >= d)
                s += u;
        }
        if (lane == EK_WAVE - 1)
            wsum[wave] = s;
        __syncthreads();
        int32_t before = 0, all = 0;
        for (int w = 0; w < POCK_SCAN_WG / EK_WAVE; ++w) {
            const int32_t x = wsum[w];
            before += (w < wave) ? x : 0;
            all += x;
        }
        if (i < nb)
            boff[i] = carry + before + s - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0)
        *total = carry;
}

__global__ void __launch_bounds__(POCK_WG)
pock_write_kernel(const int32_t *__restrict__ parent, int32_t cells,
                  const int32_t *__restrict__ boff, int32_t *__restrict__ out_cell,
                  int32_t *__restrict__ out_root)
{
    __shared__ int32_t wc[POCK_WG / EK_WAVE];
    const int lane = threadIdx.x & (EK_WAVE - 1), wave = threadIdx.x / EK_WAVE;
    const int64_t g = (int64_t)blockIdx.x * POCK_WG + threadIdx.x;
    const int32_t root = (g < cells) ? parent[g] : -1;
    const unsigned long long m = __ballot(root >= 0);
    if (lane == 0)
        wc[wave] = __popcll(m);
    __syncthreads();
    if (root < 0)
        return;
    int32_t slot = boff[blockIdx.x];    // (the slots of a block are the ones it counted)
    for (int w = 0; w < wave; ++w)
        slot += wc[w];
    slot += __popcll(m & (((unsigned long long)1 << lane) - 1));
    out_cell[slot] = (int32_t)g;
    out_root[slot] = root;
}

// ---- host ----------------------------------------------------------------------------
struct PockShape {              // of a chunk
    int64_t cells, lines;
    int32_t max_cells, max_lines;   // the largest frame's cells, the longest list of lines
};

static int pock_check_dims(const int32_t *d, const char *who, int64_t frame)
{
    for (int k = 0; k < 3; ++k)
        if (d[k] < 0 || d[k] > POCK_MAX_AXIS)
            return ek_set_error(EK_EARG, "%s: frame %lld has %d cells along axis %d, more than "
                                         "%d", who, (long long)frame, d[k], k, POCK_MAX_AXIS);
    if ((int64_t)d[0] * d[1] * d[2] > POCK_MAX_CELLS)
        return ek_set_error(EK_EARG, "%s: frame %lld has %lld cells, more than %d", who,
                            (long long)frame, (long long)((int64_t)d[0] * d[1] * d[2]),
                            POCK_MAX_CELLS);
    return EK_OK;
}

static inline int64_t pock_frame_cells(const int32_t *d)
{
    return (int64_t)d[0] * d[1] * d[2];
}

static inline int64_t pock_frame_lines(const int32_t *d)
{
    return pock_dir_off(d[0], d[1], d[2], 7);
}

static inline unsigned pock_blocks(int64_t n)
{
    return (unsigned)((n + POCK_WG - 1) / POCK_WG);
}

// the frames' table of a chunk, and the chunk's shape
static void pock_fill_frames(PockFrame *fr, const float *origin, const int32_t *dims, int64_t nf,
                             PockShape *sh)
{
    *sh = PockShape();
    for (int64_t f = 0; f < nf; ++f) {
        const int32_t *d = dims + 3 * f;
        fr[f].ox = (double)origin[3 * f];
        fr[f].oy = (double)origin[3 * f + 1];
        fr[f].oz = (double)origin[3 * f + 2];
        fr[f].nx = d[0];
        fr[f].ny = d[1];
        fr[f].nz = d[2];
        fr[f].cell_off = (int32_t)sh->cells;
        fr[f].line_off = sh->lines;
        const int64_t c = pock_frame_cells(d);
        sh->cells += c;
        sh->lines += pock_frame_lines(d);
        if (c > sh->max_cells)
            sh->max_cells = (int32_t)c;
        for (int dir = 0; dir < 4; ++dir)       // (the four diagonals have as many)
            if (pock_dir_lines(d[0], d[1], d[2], dir) > sh->max_lines)
                sh->max_lines = pock_dir_lines(d[0], d[1], d[2], dir);
    }
}

static void pock_launch_rank(const PockDev &d, int64_t nf, const PockShape &sh, int32_t min_rank,
                             uint8_t *rank_out, int32_t *parent_out, hipStream_t s)
{
    hipLaunchKernelGGL(pock_extent_kernel, dim3(pock_blocks(sh.max_lines), (unsigned)nf, 7),
                       dim3(POCK_WG), 0, s, d.fr, d.touch, d.ext);
    hipLaunchKernelGGL(pock_rank_kernel, dim3(pock_blocks(sh.max_cells), (unsigned)nf),
                       dim3(POCK_WG), 0, s, d.fr, d.touch, d.ext, min_rank, rank_out, parent_out);
}

static void pock_launch_label(const PockDev &d, int64_t nf, const PockShape &sh, hipStream_t s)
{
    hipLaunchKernelGGL(pock_union_kernel, dim3(pock_blocks(sh.max_cells), (unsigned)nf),
                       dim3(POCK_WG), 0, s, d.fr, d.parent);
    hipLaunchKernelGGL(pock_flatten_kernel, dim3(pock_blocks(sh.max_cells), (unsigned)nf),
                       dim3(POCK_WG), 0, s, d.fr, d.parent);
}

static int pock_bind(ek_pockets *h, const char *who)
{
    if (!h)
        return ek_set_error(EK_EARG, "%s: null handle", who);
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", h->device, hipGetErrorString(e));
    return EK_OK;
}

static int pock_check_cutoffs(const double *cutoff, int32_t atoms, double spacing, const char *who)
{
    if (!cutoff || atoms < 1)
        return ek_set_error(EK_EARG, "%s: bad argument (atoms >= 1)", who);
    if (!(spacing > 0.0) || !isfinite(spacing))
        return ek_set_error(EK_EARG, "%s: the grid spacing must be positive and finite", who);
    for (int32_t i = 0; i < atoms; ++i)
        if (!(cutoff[i] > 0.0) || !isfinite(cutoff[i]))
            return ek_set_error(EK_EARG, "%s: probe + radius of atom %d is not positive and "
                                         "finite", who, i);
    return EK_OK;
}

static int pock_upload_cutoffs(const double *cutoff, int32_t atoms, double **d_c, double **d_c2,
                               hipStream_t s)
{
    double *sq = new (std::nothrow) double[(size_t)atoms];
    if (!sq)
        return ek_set_error(EK_ENOMEM, "ek_pockets: out of host memory");
    for (int32_t i = 0; i < atoms; ++i)
        sq[i] = cutoff[i] * cutoff[i];
    int rc = EK_OK;
    hipError_t e = ek_dev_malloc((void **)d_c, (size_t)atoms * sizeof(double));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)d_c2, (size_t)atoms * sizeof(double));
    if (e == hipSuccess)
        e = hipMemcpyAsync(*d_c, cutoff, (size_t)atoms * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(*d_c2, sq, (size_t)atoms * sizeof(double), hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    if (e != hipSuccess)
        rc = ek_set_error(EK_EHIP, "ek_pockets: uploading the cutoffs: %s", hipGetErrorString(e));
    delete[] sq;
    return rc;
}

static void pock_drop_result(ek_pockets *h)
{
    free(h->counts);
    free(h->cells);
    free(h->labels);
    h->counts = nullptr;
    h->cells = h->labels = nullptr;
    h->frames = h->total = 0;
}

extern "C" int ek_pockets_close(ek_pockets *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(h->cutoff);
    (void)ek_dev_free(h->cutoff2);
    for (hipEvent_t e : h->ev)
        if (e)
            (void)ek_event_destroy(e);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    pock_drop_result(h);
    delete h;
    return EK_OK;
}

static int pock_open(ek_pockets *h, const double *cutoff)
{
    POCK_TRY(ek_stream_create_flags(&h->s, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev)
        POCK_TRY(ek_event_create(&e));
    return pock_upload_cutoffs(cutoff, h->atoms, &h->cutoff, &h->cutoff2, h->s);
}

extern "C" int ek_pockets_open(int device, int32_t atoms, const double *cutoff, double spacing,
                               int32_t min_rank, ek_pockets **out)
{
    if (!out)
        return ek_set_error(EK_EARG, "ek_pockets_open: null output");
    *out = nullptr;
    int rc = pock_check_cutoffs(cutoff, atoms, spacing, "ek_pockets_open");
    if (rc != EK_OK)
        return rc;
    hipError_t e0 = hipSetDevice(device);
    if (e0 != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
    ek_pockets *h = new (std::nothrow) ek_pockets();
    if (!h)
        return ek_set_error(EK_ENOMEM, "ek_pockets_open: out of host memory");
    h->device = device;
    h->atoms = atoms;
    h->min_rank = min_rank;
    h->spacing = spacing;
    rc = pock_open(h, cutoff);
    if (rc != EK_OK) {
        ek_pockets_close(h);
        return rc;
    }
    *out = h;
    return EK_OK;
}

// device bytes of a chunk of nf frames with these cells and lines (the compacted pairs at
// their most: every cell a pocket cell)
static size_t pock_chunk_bytes(int32_t atoms, int64_t nf, int64_t cells, int64_t lines)
{
    return (size_t)nf * ((size_t)atoms * 3 * sizeof(float) + sizeof(PockFrame)) +
           (size_t)cells * (1 + sizeof(int32_t) + 2 * sizeof(int32_t)) +
           (size_t)lines * sizeof(uint32_t) + ((size_t)cells / POCK_WG + 1) * 2 * sizeof(int32_t);
}

static int pock_grow_out(PockDev &d, size_t n)
{
    if (n <= d.out_cap)
        return EK_OK;
    (void)ek_dev_free(d.out);
    d.out = nullptr;
    d.out_cap = 0;
    POCK_TRY(ek_dev_malloc((void **)&d.out, 2 * n * sizeof(int32_t)));
    d.out_cap = n;
    return EK_OK;
}

// one chunk: frames [f0, f0 + nf), whose table fr (host) and shape sh are filled
static int pock_run_chunk(ek_pockets *h, PockDev &d, const float *xyz, const PockFrame *fr,
                          int64_t f0, int64_t nf, const PockShape &sh, int32_t *host_out)
{
    hipStream_t s = h->s;
    int32_t total = 0;
    const unsigned nb = pock_blocks(sh.cells);
    POCK_TRY(hipEventRecord(h->ev[0], s));
    POCK_TRY(hipMemcpyAsync(d.xyz, xyz + (size_t)f0 * h->atoms * 3,
                            (size_t)nf * h->atoms * 3 * sizeof(float), hipMemcpyHostToDevice, s));
    POCK_TRY(hipMemcpyAsync(d.fr, fr, (size_t)nf * sizeof(PockFrame), hipMemcpyHostToDevice, s));
    POCK_TRY(hipMemsetAsync(d.touch, 0, (size_t)sh.cells, s));
    POCK_TRY(hipEventRecord(h->ev[1], s));
    hipLaunchKernelGGL(pock_touch_kernel,
                       dim3((unsigned)((h->atoms + POCK_WG / EK_WAVE - 1) / (POCK_WG / EK_WAVE)),
                            (unsigned)nf),
                       dim3(POCK_WG), 0, s, d.xyz, h->atoms, h->cutoff, h->cutoff2, h->spacing,
                       d.fr, d.touch);
    POCK_TRY(hipEventRecord(h->ev[2], s));
    pock_launch_rank(d, nf, sh, h->min_rank, nullptr, d.parent, s);
    POCK_TRY(hipEventRecord(h->ev[3], s));
    pock_launch_label(d, nf, sh, s);
    hipLaunchKernelGGL(pock_count_kernel, dim3(nb), dim3(POCK_WG), 0, s, d.parent,
                       (int32_t)sh.cells, d.bcnt);
    hipLaunchKernelGGL(pock_scan_kernel, dim3(1), dim3(POCK_SCAN_WG), 0, s, d.bcnt, (int32_t)nb,
                       d.boff, d.total);
    POCK_TRY(hipGetLastError());
    POCK_TRY(hipMemcpyAsync(&total, d.total, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    POCK_TRY(hipStreamSynchronize(s));
    if (total < 0 || (int64_t)total > sh.cells)
        return ek_set_error(EK_ESTATE, "ek_pockets_run: %d pocket cells of %lld cells", total,
                            (long long)sh.cells);
    if (total > 0) {
        int rc = pock_grow_out(d, (size_t)total);
        if (rc != EK_OK)
            return rc;
        hipLaunchKernelGGL(pock_write_kernel, dim3(nb), dim3(POCK_WG), 0, s, d.parent,
                           (int32_t)sh.cells, d.boff, d.out, d.out + d.out_cap);
    }
    POCK_TRY(hipEventRecord(h->ev[4], s));
    POCK_TRY(hipGetLastError());
    if (total > 0) {
        POCK_TRY(hipMemcpyAsync(host_out, d.out, (size_t)total * sizeof(int32_t),
                                hipMemcpyDeviceToHost, s));
        POCK_TRY(hipMemcpyAsync(host_out + total, d.out + d.out_cap,
                                (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    POCK_TRY(hipStreamSynchronize(s));
    for (int q = 0; q < 4; ++q) {
        float ms = 0.f;
        POCK_TRY(hipEventElapsedTime(&ms, h->ev[q], h->ev[q + 1]));
        h->ms[q] += ms;
    }
    // append to the result: chunk-wide indices -> the frames' own
    {
        const int64_t need = h->total + total;
        int32_t *nc = (int32_t *)realloc(h->cells, (size_t)(need ? need : 1) * sizeof(int32_t));
        if (nc)
            h->cells = nc;
        int32_t *nl = (int32_t *)realloc(h->labels, (size_t)(need ? need : 1) * sizeof(int32_t));
        if (nl)
            h->labels = nl;
        if (!nc || !nl)
            return ek_set_error(EK_ENOMEM, "ek_pockets_run: out of host memory");
    }
    int64_t q = 0;
    for (int64_t f = 0; f < nf; ++f) {
        const int64_t end = (f + 1 < nf) ? fr[f + 1].cell_off : sh.cells;
        int64_t n = 0;
        while (q < total && host_out[q] < end) {
            h->cells[h->total + q] = host_out[q] - fr[f].cell_off;
            h->labels[h->total + q] = host_out[total + q] - fr[f].cell_off;
            ++q;
            ++n;
        }
        h->counts[f0 + f] = n;
    }
    h->total += total;
    return EK_OK;
}

static int pock_run(ek_pockets *h, PockDev &d, const float *xyz, int64_t frames,
                    const float *origin, const int32_t *dims, int64_t chunk_frames,
                    PockFrame *fr, int64_t *chunk_end)
{
    // the chunks: [chunk_end[i - 1], chunk_end[i])
    size_t budget = 0;
    if (chunk_frames == 0) {
        size_t free_b = 0, total_b = 0;
        POCK_TRY(hipMemGetInfo(&free_b, &total_b));
        budget = free_b / 2;
    }
    int64_t n_chunks = 0, max_nf = 0, max_cells = 0, max_lines = 0;
    size_t max_bytes = 0;
    for (int64_t f0 = 0; f0 < frames;) {
        int64_t nf = 0, cells = 0, lines = 0;
        while (f0 + nf < frames && nf < POCK_MAX_FRAMES) {
            const int32_t *dd = dims + 3 * (f0 + nf);
            const int64_t c = cells + pock_frame_cells(dd), l = lines + pock_frame_lines(dd);
            if (chunk_frames > 0) {
                if (nf == chunk_frames)
                    break;
                if (c >= POCK_MAX_CHUNK_CELLS)
                    return ek_set_error(EK_EARG, "ek_pockets_run: %lld frames from frame %lld "
                                                 "hold 2^30 cells or more: use smaller chunks",
                                        (long long)chunk_frames, (long long)f0);
            } else if (nf > 0 && (c >= POCK_MAX_CHUNK_CELLS ||
                                  pock_chunk_bytes(h->atoms, nf + 1, c, l) > budget))
                break;
            cells = c;
            lines = l;
            ++nf;
        }
        const size_t bytes = pock_chunk_bytes(h->atoms, nf, cells, lines);
        max_bytes = bytes > max_bytes ? bytes : max_bytes;
        max_nf = nf > max_nf ? nf : max_nf;
        max_cells = cells > max_cells ? cells : max_cells;
        max_lines = lines > max_lines ? lines : max_lines;
        f0 += nf;
        chunk_end[n_chunks++] = f0;
    }
    int rc = ek_mi_check_memory(max_bytes, "ek_pockets_run");
    if (rc != EK_OK)
        return rc;
    int32_t *host_out = (int32_t *)malloc((size_t)(max_cells ? max_cells : 1) * 2 * sizeof(int32_t));
    if (!host_out)
        return ek_set_error(EK_ENOMEM, "ek_pockets_run: out of host memory");
    const size_t nbk = (size_t)max_cells / POCK_WG + 1;
    hipError_t e = ek_dev_malloc((void **)&d.xyz, (size_t)max_nf * h->atoms * 3 * sizeof(float));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&d.fr, (size_t)max_nf * sizeof(PockFrame));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&d.touch, (size_t)max_cells + 1);
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&d.parent, ((size_t)max_cells + 1) * sizeof(int32_t));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&d.ext, ((size_t)max_lines + 1) * sizeof(uint32_t));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&d.bcnt, nbk * sizeof(int32_t));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&d.boff, nbk * sizeof(int32_t));
    if (e == hipSuccess)
        e = ek_dev_malloc((void **)&d.total, sizeof(int32_t));
    if (e != hipSuccess)
        rc = ek_set_error(e == hipErrorOutOfMemory ? EK_ENOMEM : EK_EHIP,
                          "ek_pockets_run: ek_dev_malloc: %s", hipGetErrorString(e));
    for (int64_t i = 0, f0 = 0; rc == EK_OK && i < n_chunks; f0 = chunk_end[i++]) {
        const int64_t nf = chunk_end[i] - f0;
        PockShape sh;
        pock_fill_frames(fr, origin + 3 * f0, dims + 3 * f0, nf, &sh);
        if (sh.cells == 0) {
            for (int64_t f = 0; f < nf; ++f)
                h->counts[f0 + f] = 0;
            continue;
        }
        rc = pock_run_chunk(h, d, xyz, fr, f0, nf, sh, host_out);
    }
    free(host_out);
    return rc;
}

extern "C" int ek_pockets_run(ek_pockets *h, const float *xyz, int64_t frames, const float *origin,
                              const int32_t *dims, int64_t chunk_frames)
{
    int rc = pock_bind(h, "ek_pockets_run");
    if (rc != EK_OK)
        return rc;
    if (!xyz || !origin || !dims || frames < 0 || chunk_frames < 0 ||
        chunk_frames > POCK_MAX_FRAMES)
        return ek_set_error(EK_EARG, "ek_pockets_run: bad argument (0 <= chunk_frames <= %d)",
                            POCK_MAX_FRAMES);
    pock_drop_result(h);
    h->ms[0] = h->ms[1] = h->ms[2] = h->ms[3] = 0.0;
    if (frames == 0)
        return EK_OK;
    for (size_t q = 0, nq = (size_t)frames * h->atoms * 3; q < nq; ++q)
        if (!isfinite(xyz[q]))
            return ek_set_error(EK_EARG, "ek_pockets_run: coordinate %zu is not finite", q);
    for (int64_t f = 0; f < frames; ++f) {
        for (int k = 0; k < 3; ++k)
            if (!isfinite(origin[3 * f + k]))
                return ek_set_error(EK_EARG, "ek_pockets_run: the origin of frame %lld is not "
                                             "finite", (long long)f);
        rc = pock_check_dims(dims + 3 * f, "ek_pockets_run", f);
        if (rc != EK_OK)
            return rc;
    }
    h->counts = (int64_t *)calloc((size_t)frames, sizeof(int64_t));
    const int64_t cap = frames < POCK_MAX_FRAMES ? frames : POCK_MAX_FRAMES;
    PockFrame *fr = (PockFrame *)malloc((size_t)cap * sizeof(PockFrame));
    int64_t *chunk_end = (int64_t *)malloc((size_t)frames * sizeof(int64_t));
    if (!h->counts || !fr || !chunk_end)
        rc = ek_set_error(EK_ENOMEM, "ek_pockets_run: out of host memory");
    else {
        h->frames = frames;
        PockDev d;
        rc = pock_run(h, d, xyz, frames, origin, dims, chunk_frames, fr, chunk_end);
        (void)hipStreamSynchronize(h->s);
        pock_dev_free(d);
    }
    free(fr);
    free(chunk_end);
    if (rc != EK_OK)
        pock_drop_result(h);
    return rc;
}

extern "C" int ek_pockets_counts(ek_pockets *h, int64_t frames, int64_t *counts_out)
{
    if (!h || !counts_out)
        return ek_set_error(EK_EARG, "ek_pockets_counts: null argument");
    if (frames != h->frames)
        return ek_set_error(EK_ESTATE, "ek_pockets_counts: the last run had %lld frames, not "
                                       "%lld", (long long)h->frames, (long long)frames);
    for (int64_t f = 0; f < frames; ++f)
        counts_out[f] = h->counts[f];
    return EK_OK;
}

extern "C" int ek_pockets_fetch(ek_pockets *h, int32_t *cells_out, int32_t *labels_out)
{
    if (!h || ((!cells_out || !labels_out) && h->total > 0))
        return ek_set_error(EK_EARG, "ek_pockets_fetch: null argument");
    if (h->total > 0) {
        memcpy(cells_out, h->cells, (size_t)h->total * sizeof(int32_t));
        memcpy(labels_out, h->labels, (size_t)h->total * sizeof(int32_t));
    }
    return EK_OK;
}

extern "C" int ek_pockets_last_timing(ek_pockets *h, double *ms_out)
{
    if (!h || !ms_out)
        return ek_set_error(EK_EARG, "ek_pockets_last_timing: null argument");
    for (int i = 0; i < 4; ++i)
        ms_out[i] = h->ms[i];
    return EK_OK;
}

// ---- one stage on one dense grid -------------------------------------------------------
static int pock_single_frame(int device, const int32_t *dims, const float *origin, const char *who,
                             PockFrame *fr, PockShape *sh)
{
    if (!dims)
        return ek_set_error(EK_EARG, "%s: null argument", who);
    int rc = pock_check_dims(dims, who, 0);
    if (rc != EK_OK)
        return rc;
    if (pock_frame_cells(dims) < 1)
        return ek_set_error(EK_EARG, "%s: the grid has no cells", who);
    const float zero[3] = {0.f, 0.f, 0.f};
    pock_fill_frames(fr, origin ? origin : zero, dims, 1, sh);
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    return EK_OK;
}

static int pock_touches(PockDev &d, double **d_c, double **d_c2, const float *xyz, int32_t atoms,
                        const double *cutoff, double spacing, const PockFrame &fr,
                        const PockShape &sh, uint8_t *out)
{
    POCK_TRY(ek_dev_malloc((void **)&d.xyz, (size_t)atoms * 3 * sizeof(float)));
    POCK_TRY(ek_dev_malloc((void **)&d.fr, sizeof(PockFrame)));
    POCK_TRY(ek_dev_malloc((void **)&d.touch, (size_t)sh.cells));
    int rc = pock_upload_cutoffs(cutoff, atoms, d_c, d_c2, nullptr);
    if (rc != EK_OK)
        return rc;
    POCK_TRY(hipMemcpy(d.xyz, xyz, (size_t)atoms * 3 * sizeof(float), hipMemcpyHostToDevice));
    POCK_TRY(hipMemcpy(d.fr, &fr, sizeof(PockFrame), hipMemcpyHostToDevice));
    POCK_TRY(hipMemset(d.touch, 0, (size_t)sh.cells));
    hipLaunchKernelGGL(pock_touch_kernel,
                       dim3((unsigned)((atoms + POCK_WG / EK_WAVE - 1) / (POCK_WG / EK_WAVE)), 1),
                       dim3(POCK_WG), 0, nullptr, d.xyz, atoms, *d_c, *d_c2, spacing, d.fr,
                       d.touch);
    POCK_TRY(hipGetLastError());
    POCK_TRY(hipMemcpy(out, d.touch, (size_t)sh.cells, hipMemcpyDeviceToHost));
    return EK_OK;
}

extern "C" int ek_pockets_touches(int device, const float *xyz, int32_t atoms,
                                  const double *cutoff, double spacing, const float *origin,
                                  const int32_t *dims, uint8_t *touches_out)
{
    if (!xyz || !origin || !touches_out)
        return ek_set_error(EK_EARG, "ek_pockets_touches: null argument");
    int rc = pock_check_cutoffs(cutoff, atoms, spacing, "ek_pockets_touches");
    if (rc != EK_OK)
        return rc;
    for (size_t q = 0; q < (size_t)atoms * 3; ++q)
        if (!isfinite(xyz[q]))
            return ek_set_error(EK_EARG, "ek_pockets_touches: coordinate %zu is not finite", q);
    for (int k = 0; k < 3; ++k)
        if (!isfinite(origin[k]))
            return ek_set_error(EK_EARG, "ek_pockets_touches: the origin is not finite");
    PockFrame fr;
    PockShape sh;
    rc = pock_single_frame(device, dims, origin, "ek_pockets_touches", &fr, &sh);
    if (rc != EK_OK)
        return rc;
    PockDev d;
    double *d_c = nullptr, *d_c2 = nullptr;
    rc = pock_touches(d, &d_c, &d_c2, xyz, atoms, cutoff, spacing, fr, sh, touches_out);
    (void)hipDeviceSynchronize();
    (void)ek_dev_free(d_c);
    (void)ek_dev_free(d_c2);
    pock_dev_free(d);
    return rc;
}

static int pock_ranks(PockDev &d, const uint8_t *touches, const PockFrame &fr, const PockShape &sh,
                      uint8_t *out)
{
    POCK_TRY(ek_dev_malloc((void **)&d.fr, sizeof(PockFrame)));
    POCK_TRY(ek_dev_malloc((void **)&d.touch, (size_t)sh.cells));
    POCK_TRY(ek_dev_malloc((void **)&d.rank, (size_t)sh.cells));
    POCK_TRY(ek_dev_malloc((void **)&d.ext, (size_t)sh.lines * sizeof(uint32_t)));
    POCK_TRY(hipMemcpy(d.fr, &fr, sizeof(PockFrame), hipMemcpyHostToDevice));
    POCK_TRY(hipMemcpy(d.touch, touches, (size_t)sh.cells, hipMemcpyHostToDevice));
    pock_launch_rank(d, 1, sh, 0, d.rank, nullptr, nullptr);
    POCK_TRY(hipGetLastError());
    POCK_TRY(hipMemcpy(out, d.rank, (size_t)sh.cells, hipMemcpyDeviceToHost));
    return EK_OK;
}

extern "C" int ek_pockets_ranks(int device, const uint8_t *touches, const int32_t *dims,
                                uint8_t *ranks_out)
{
    if (!touches || !ranks_out)
        return ek_set_error(EK_EARG, "ek_pockets_ranks: null argument");
    PockFrame fr;
    PockShape sh;
    int rc = pock_single_frame(device, dims, nullptr, "ek_pockets_ranks", &fr, &sh);
    if (rc != EK_OK)
        return rc;
    PockDev d;
    rc = pock_ranks(d, touches, fr, sh, ranks_out);
    (void)hipDeviceSynchronize();
    pock_dev_free(d);
    return rc;
}

static int pock_labels(PockDev &d, const uint8_t *mask, const PockFrame &fr, const PockShape &sh,
                       int32_t *out)
{
    POCK_TRY(ek_dev_malloc((void **)&d.fr, sizeof(PockFrame)));
    POCK_TRY(ek_dev_malloc((void **)&d.touch, (size_t)sh.cells));
    POCK_TRY(ek_dev_malloc((void **)&d.parent, (size_t)sh.cells * sizeof(int32_t)));
    POCK_TRY(hipMemcpy(d.fr, &fr, sizeof(PockFrame), hipMemcpyHostToDevice));
    POCK_TRY(hipMemcpy(d.touch, mask, (size_t)sh.cells, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(pock_mask_kernel, dim3(pock_blocks(sh.cells)), dim3(POCK_WG), 0, nullptr,
                       d.touch, (int32_t)sh.cells, d.parent);
    pock_launch_label(d, 1, sh, nullptr);
    POCK_TRY(hipGetLastError());
    POCK_TRY(hipMemcpy(out, d.parent, (size_t)sh.cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    return EK_OK;
}

extern "C" int ek_pockets_labels(int device, const uint8_t *mask, const int32_t *dims,
                                 int32_t *labels_out)
{
    if (!mask || !labels_out)
        return ek_set_error(EK_EARG, "ek_pockets_labels: null argument");
    PockFrame fr;
    PockShape sh;
    int rc = pock_single_frame(device, dims, nullptr, "ek_pockets_labels", &fr, &sh);
    if (rc != EK_OK)
        return rc;
    PockDev d;
    rc = pock_labels(d, mask, fr, sh, labels_out);
    (void)hipDeviceSynchronize();
    pock_dev_free(d);
    return rc;
}
