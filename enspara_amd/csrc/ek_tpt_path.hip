// ek_tpt_path.hip -- the highest-flux pathways of a net-flux matrix: the widest-path
// searches of the reference's enspara/tpt/path.py (top_path :46-160, the two ways of
// removing a path :163-194, paths :197-320) on the device.
//
// The reference runs Dijkstra's algorithm with min() in the place of + on a dense
// matrix, with a Python list for a queue, and copies the matrix twice per path.  Here
// the matrix is compacted ONCE into a CSR of its entries > 0 (columns ascending within
// a row), the searches read the popped row's segment only, and removing a path edits
// the CSR values in place: an entry that reaches 0 fails `> 0` from then on.
//
// Which node the reference's list pops, duplicates and ties included, is this rule:
//   among the nodes inserted and not yet visited, the largest min_flux; on ties the
//   earliest FIRST insertion.  The sources are inserted first, in the order given (a
//   repeated source at its first position); the relaxation of the node popped at step t
//   inserts its improved neighbours in ascending state index; inserting a node again
//   does not move it.  So the key  t * n + state  (sources: their rank, t = 0) orders
//   the insertions.
//   relaxation of u: w = min(F[u][v], min_flux[u]) for F[u][v] > 0, taken iff v is not
//   visited and w > min_flux[v] (strict); previous[v] = u.
//   after each pop the node is visited; the search ends when every sink is visited or
//   nothing is left.  The path ends at the first sink (of the list given) with the
//   largest min_flux and is walked back along `previous`.
//   'subtract' takes the least of the path's edges off each of them and then sets the
//   first least edge along the path to 0.0; 'bottleneck' does the last step only.
// The results are integers and doubles made by single IEEE operations in the
// reference's order (flux / total_flux, the running sum): they are the reference's bits.
//
// Two kernels.  The compaction runs across the device: a wave per row counts, one
// workgroup scans, a wave per row fills.  The search is ONE workgroup that stays
// resident for a batch of paths; per state it keeps min_flux, the insertion key,
// `previous` as the CSR slot of the edge (so that removal needs no lookup), the flags
// and a compact frontier list (the pop is a reduction over the frontier, not over n):
// TPT_PATH_STATE_BYTES per state, in the LDS up to TPT_PATH_LDS_STATES states and in
// global memory above, through the same code.  Every loop is bounded by construction
// (a search pops a state at most once, a walk back takes fewer steps than there are
// states) and carries a counter all the same: a counter that runs out ends the handle
// with an error code.  A batch is capped in paths, in output nodes and in pops, so a
// launch stays short; the host loops over batches.  No workgroup waits for another.
#include "ek_common.h"

#include <math.h>
#include <new>
#include <string.h>

extern int ek_set_error(int code, const char *fmt, ...);
int ek_mi_check_memory(size_t bytes, const char *who);

#define PATH_HIP(call)                                                         \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define TPT_PATH_WG 256             // the search workgroup: one wave per SIMD
#define TPT_PATH_WAVES (TPT_PATH_WG / EK_WAVE)
// per state: min_flux 8, key 4, previous 4, frontier 4, flags 1
#define TPT_PATH_STATE_BYTES 21
// 7680 * 21 = 161280 of the 163840 bytes a workgroup may have; the rest is the
// reductions' scratch and the control words
#define TPT_PATH_LDS_STATES 7680
#define TPT_PATH_MAX_N 65535        // t * n + state fits 32 bits for t <= n
#define TPT_PATH_BATCH_PATHS 32     // of one launch, by default
#define TPT_PATH_BATCH_NODES 65536
#define TPT_PATH_BATCH_POPS 65536   // a launch ends after the path that crosses this
#define TPT_PATH_COMPACT_WG 256     // compaction: a wave per row
#define TPT_PATH_SCAN_WG 1024

enum { PATH_KEEP = 0, PATH_SUBTRACT = 1, PATH_BOTTLENECK = 2 };
enum { PATH_VISITED = 1, PATH_QUEUED = 2, PATH_SINK = 4 };
enum { PATH_INFO_OK = 0, PATH_INFO_POPS = 1, PATH_INFO_WALK = 2 };
#define PATH_NONE 0xffffffffu

// ---- compaction ------------------------------------------------------------------------
__global__ void __launch_bounds__(TPT_PATH_COMPACT_WG)
tpt_path_count_kernel(int32_t n, const double *__restrict__ F, int32_t *__restrict__ cnt)
{
    const int lane = threadIdx.x % EK_WAVE;
    const int32_t row = blockIdx.x * (TPT_PATH_COMPACT_WG / EK_WAVE) + threadIdx.x / EK_WAVE;
    if (row >= n)
        return;
    const double *r = F + (size_t)row * n;
    int32_t c = 0;
    for (int32_t j0 = 0; j0 < n; j0 += EK_WAVE) {
        const int32_t j = j0 + lane;
        const bool p = j < n && r[j] > 0.0;
        c += __popcll(__ballot(p));
    }
    if (lane == 0)
        cnt[row] = c;
}

// indptr[i] = the sum of cnt[0 .. i), i <= n: one workgroup, a run of states per thread
__global__ void __launch_bounds__(TPT_PATH_SCAN_WG)
tpt_path_scan_kernel(int32_t n, const int32_t *__restrict__ cnt, int64_t *__restrict__ indptr)
{
    __shared__ int64_t part[TPT_PATH_SCAN_WG];
    const int tid = threadIdx.x;
    const int32_t per = (n + TPT_PATH_SCAN_WG - 1) / TPT_PATH_SCAN_WG;
    const int32_t lo = tid * per < n ? tid * per : n;
    const int32_t hi = lo + per < n ? lo + per : n;
    int64_t own = 0;
    for (int32_t i = lo; i < hi; ++i)
        own += cnt[i];
    part[tid] = own;
    __syncthreads();
    for (int off = 1; off < TPT_PATH_SCAN_WG; off <<= 1) {
        const int64_t x = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += x;
        __syncthreads();
    }
    int64_t base = part[tid] - own;
    for (int32_t i = lo; i < hi; ++i) {
        indptr[i] = base;
        base += cnt[i];
    }
    if (tid == TPT_PATH_SCAN_WG - 1)
        indptr[n] = part[tid];
}

// the entries > 0 of row `row` to indptr[row] .., columns ascending (the count kernel's
// predicate on the same data: a row writes exactly its own segment)
__global__ void __launch_bounds__(TPT_PATH_COMPACT_WG)
tpt_path_fill_kernel(int32_t n, const double *__restrict__ F,
                     const int64_t *__restrict__ indptr, int32_t *__restrict__ cols,
                     double *__restrict__ vals, int32_t *__restrict__ rowof)
{
    const int lane = threadIdx.x % EK_WAVE;
    const int32_t row = blockIdx.x * (TPT_PATH_COMPACT_WG / EK_WAVE) + threadIdx.x / EK_WAVE;
    if (row >= n)
        return;
    const double *r = F + (size_t)row * n;
    int64_t base = indptr[row];
    for (int32_t j0 = 0; j0 < n; j0 += EK_WAVE) {
        const int32_t j = j0 + lane;
        const double x = j < n ? r[j] : 0.0;
        const bool p = x > 0.0;
        const unsigned long long mask = __ballot(p);
        if (p) {
            const int64_t pos = base + __popcll(mask & ((1ull << lane) - 1ull));
            cols[pos] = j;
            vals[pos] = x;
            rowof[pos] = row;
        }
        base += __popcll(mask);
    }
}

// CSR input: the row of every slot (the host checked that indptr ascends from 0 to nnz)
__global__ void __launch_bounds__(TPT_PATH_COMPACT_WG)
tpt_path_rowof_kernel(int32_t n, const int64_t *__restrict__ indptr, int32_t *__restrict__ rowof)
{
    const int lane = threadIdx.x % EK_WAVE;
    const int32_t row = blockIdx.x * (TPT_PATH_COMPACT_WG / EK_WAVE) + threadIdx.x / EK_WAVE;
    if (row >= n)
        return;
    const int64_t e1 = indptr[row + 1];
    for (int64_t e = indptr[row] + lane; e < e1; e += EK_WAVE)
        rowof[e] = row;
}

// ---- search ----------------------------------------------------------------------------
// what a handle keeps on the device between batches
struct PathState {
    double expl;            // the running sum of flux / total_flux
    long long counter;      // paths appended so far
    long long pops;         // pops of all searches so far
    int32_t done, info;
    int32_t count, n_nodes; // the last batch's paths and nodes
};

struct PathArgs {
    int32_t n, n_src, n_sinks, n_sinks_distinct, mode;
    int32_t cap_paths, cap_nodes;
    long long num_paths;
    double total, cutoff;
    const int64_t *indptr;
    const int32_t *cols, *rowof;
    double *vals;
    const int32_t *src;         // the distinct sources, in the order of their first mention
    const int32_t *sinks;       // as given
    unsigned char *gstate;      // the per-state arrays above TPT_PATH_LDS_STATES
    int32_t *pslot;             // [n] the walk back's slots, last edge first
    int32_t *nodes, *offsets;
    double *fluxes;
    PathState *state;
};

// The workgroup's best (v, k): the largest v (MIN: the smallest), then the smallest k; p
// rides along.  A thread with nothing passes k = PATH_NONE.  Every thread gets the result.
// One barrier inside; the caller has another between two calls (the scratch is reused).
template <bool MIN>
__device__ inline void path_best(double &v, uint32_t &k, int32_t &p, double *rv, uint32_t *rk,
                                 int32_t *rp)
{
    for (int off = EK_WAVE / 2; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off);
        const uint32_t ok = __shfl_down(k, off);
        const int32_t op = __shfl_down(p, off);
        if (ok != PATH_NONE &&
            (k == PATH_NONE || (MIN ? ov < v : ov > v) || (ov == v && ok < k))) {
            v = ov;
            k = ok;
            p = op;
        }
    }
    if (threadIdx.x % EK_WAVE == 0) {
        rv[threadIdx.x / EK_WAVE] = v;
        rk[threadIdx.x / EK_WAVE] = k;
        rp[threadIdx.x / EK_WAVE] = p;
    }
    __syncthreads();
    v = rv[0];
    k = rk[0];
    p = rp[0];
    for (int w = 1; w < TPT_PATH_WAVES; ++w) {
        const double ov = rv[w];
        const uint32_t ok = rk[w];
        if (ok != PATH_NONE &&
            (k == PATH_NONE || (MIN ? ov < v : ov > v) || (ov == v && ok < k))) {
            v = ov;
            k = ok;
            p = rp[w];
        }
    }
}

template <bool LDS>
__global__ void __launch_bounds__(TPT_PATH_WG) tpt_path_search_kernel(PathArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char path_lds[];
    __shared__ double rv[TPT_PATH_WAVES];
    __shared__ uint32_t rk[TPT_PATH_WAVES];
    __shared__ int32_t rp[TPT_PATH_WAVES];
    __shared__ int32_t s_fcount, s_sinks_left, s_u, s_edges, s_walk;

    const int tid = threadIdx.x;
    const int32_t n = a.n;
    unsigned char *base = LDS ? path_lds : a.gstate;
    double *min_flux = (double *)base;
    uint32_t *key = (uint32_t *)(min_flux + n);
    int32_t *prev = (int32_t *)(key + n);
    int32_t *frontier = prev + n;
    uint8_t *flags = (uint8_t *)(frontier + n);

    // (every thread carries the same values: they come from reductions all of them get)
    double expl = a.state->expl;
    long long counter = a.state->counter;
    long long pops = 0;
    int32_t count = 0, off = 0, done = 0, info = PATH_INFO_OK;
    if (tid == 0)
        a.offsets[0] = 0;

    while (count < a.cap_paths && pops < TPT_PATH_BATCH_POPS) {
        // ---- one search ----
        for (int32_t i = tid; i < n; i += TPT_PATH_WG) {
            min_flux[i] = -INFINITY;
            prev[i] = -1;
            flags[i] = 0;
        }
        __syncthreads();
        for (int32_t i = tid; i < a.n_sinks; i += TPT_PATH_WG)
            flags[a.sinks[i]] = PATH_SINK;
        __syncthreads();
        for (int32_t i = tid; i < a.n_src; i += TPT_PATH_WG) {
            const int32_t s = a.src[i];
            min_flux[s] = INFINITY;
            key[s] = (uint32_t)i;
            flags[s] |= PATH_QUEUED;
            frontier[i] = s;
        }
        if (tid == 0) {
            s_fcount = a.n_src;
            s_sinks_left = a.n_sinks_distinct;
        }
        uint32_t t = 0;
        for (;;) {
            __syncthreads();
            const int32_t fc = s_fcount;
            if (fc == 0)
                break;
            if (t == (uint32_t)n) {     // more pops than states
                info = PATH_INFO_POPS;
                break;
            }
            ++t;
            double bv = -INFINITY;
            uint32_t bk = PATH_NONE;
            int32_t bp = -1;
            for (int32_t i = tid; i < fc; i += TPT_PATH_WG) {
                const int32_t v = frontier[i];
                const double mf = min_flux[v];
                const uint32_t kk = key[v];
                if (bk == PATH_NONE || mf > bv || (mf == bv && kk < bk)) {
                    bv = mf;
                    bk = kk;
                    bp = i;
                }
            }
            path_best<false>(bv, bk, bp, rv, rk, rp);
            if (tid == 0) {
                const int32_t u = frontier[bp];
                s_u = u;
                frontier[bp] = frontier[fc - 1];
                s_fcount = fc - 1;
                const uint8_t fu = flags[u];
                flags[u] = fu | PATH_VISITED;
                if (fu & PATH_SINK)
                    s_sinks_left -= 1;
            }
            __syncthreads();
            if (s_sinks_left == 0)
                break;
            const int32_t u = s_u;
            const int64_t e1 = a.indptr[u + 1];
            for (int64_t e = a.indptr[u] + tid; e < e1; e += TPT_PATH_WG) {
                const double f = a.vals[e];
                if (!(f > 0.0))
                    continue;
                const int32_t v = a.cols[e];
                const uint8_t fl = flags[v];
                if (fl & PATH_VISITED)
                    continue;
                const double w = f > bv ? bv : f;       // bv = min_flux[u]
                if (w > min_flux[v]) {
                    min_flux[v] = w;
                    prev[v] = (int32_t)e;
                    if (!(fl & PATH_QUEUED)) {
                        flags[v] = fl | PATH_QUEUED;
                        key[v] = t * (uint32_t)n + (uint32_t)v;
                        frontier[atomicAdd(&s_fcount, 1)] = v;
                    }
                }
            }
        }
        pops += t;
        if (info != PATH_INFO_OK)
            break;

        // ---- the path: the first sink with the largest min_flux, walked back ----
        double flux = -INFINITY;
        uint32_t best_sink = PATH_NONE;
        int32_t unused = 0;
        for (int32_t i = tid; i < a.n_sinks; i += TPT_PATH_WG) {
            const double mf = min_flux[a.sinks[i]];
            if (best_sink == PATH_NONE || mf > flux) {
                flux = mf;
                best_sink = (uint32_t)i;
            }
        }
        path_best<false>(flux, best_sink, unused, rv, rk, rp);
        const int32_t end = a.sinks[best_sink];
        if (tid == 0) {
            int32_t v = end, edges = 0, walk = PATH_INFO_OK;
            while (prev[v] >= 0) {
                if (edges == n) {       // more steps than states
                    walk = PATH_INFO_WALK;
                    break;
                }
                const int32_t e = prev[v];
                a.pslot[edges++] = e;
                v = a.rowof[e];
            }
            s_edges = edges;
            s_walk = walk;
        }
        __syncthreads();
        const int32_t edges = s_edges;
        if (s_walk != PATH_INFO_OK) {
            info = s_walk;
            break;
        }
        if (a.mode != PATH_KEEP && isinf(flux)) {
            done = 1;
            break;
        }
        if (count > 0 && off + edges + 1 > a.cap_nodes)
            break;                      // it opens the next batch
        double mv = INFINITY;
        uint32_t mk = PATH_NONE;
        for (int32_t i = tid; i < edges; i += TPT_PATH_WG) {
            const int32_t s = a.pslot[edges - 1 - i];
            a.nodes[off + i] = a.rowof[s];
            const double x = a.vals[s];
            if (mk == PATH_NONE || x < mv) {
                mv = x;
                mk = (uint32_t)i;
            }
        }
        if (tid == 0) {
            a.nodes[off + edges] = end;
            a.fluxes[count] = flux;
            a.offsets[count + 1] = off + edges + 1;
        }
        off += edges + 1;
        count += 1;
        if (a.mode == PATH_KEEP) {
            done = 1;
            break;
        }
        expl += flux / a.total;
        counter += 1;
        if (counter >= a.num_paths || expl >= a.cutoff) {
            done = 1;
            break;
        }
        // ---- remove it ----
        path_best<true>(mv, mk, unused, rv, rk, rp);
        if (a.mode == PATH_SUBTRACT) {
            double nv = INFINITY;
            uint32_t nk = PATH_NONE;
            for (int32_t i = tid; i < edges; i += TPT_PATH_WG) {
                const int32_t s = a.pslot[edges - 1 - i];
                const double x = a.vals[s] - mv;
                a.vals[s] = x;
                if (nk == PATH_NONE || x < nv) {
                    nv = x;
                    nk = (uint32_t)i;
                }
            }
            __syncthreads();
            path_best<true>(nv, nk, unused, rv, rk, rp);
            mk = nk;
        }
        if (tid == 0 && mk != PATH_NONE)
            a.vals[a.pslot[edges - 1 - (int32_t)mk]] = 0.0;
        __syncthreads();
    }
    if (tid == 0) {
        PathState *st = a.state;
        st->expl = expl;
        st->counter = counter;
        st->pops += pops;
        st->done = (done || info != PATH_INFO_OK) ? 1 : 0;
        st->info = info;
        st->count = count;
        st->n_nodes = off;
    }
}

// ---- host side -------------------------------------------------------------------------
struct ek_tpt_paths {
    int device;
    int done;
    int lds;                    // the per-state arrays are in the LDS
    size_t lds_bytes;
    int32_t node_buf;           // entries of `nodes`: max(cap_nodes, n)
    int64_t nnz;
    PathArgs a;
    int32_t *cols, *rowof, *src, *sinks;
    int64_t *indptr;
    hipStream_t s;
    hipEvent_t ev[4];           // compaction from / to, the last search launch from / to
    double ms_compact, ms_search;
    long long n_paths;
};

static bool path_states_ok(const int32_t *s, int32_t count, int32_t n)
{
    if (!s || count < 1)
        return false;
    for (int32_t i = 0; i < count; ++i)
        if (s[i] < 0 || s[i] >= n)
            return false;
    return true;
}

static int path_bind(ek_tpt_paths *h, const char *who)
{
    if (!h)
        return ek_set_error(EK_EARG, "%s: null handle", who);
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", h->device, hipGetErrorString(e));
    return EK_OK;
}

extern "C" int ek_tpt_paths_close(ek_tpt_paths *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(h->indptr);
    (void)ek_dev_free(h->cols);
    (void)ek_dev_free(h->rowof);
    (void)ek_dev_free(h->a.vals);
    (void)ek_dev_free(h->src);
    (void)ek_dev_free(h->sinks);
    (void)ek_dev_free(h->a.gstate);
    (void)ek_dev_free(h->a.pslot);
    (void)ek_dev_free(h->a.nodes);
    (void)ek_dev_free(h->a.offsets);
    (void)ek_dev_free(h->a.fluxes);
    (void)ek_dev_free(h->a.state);
    for (hipEvent_t e : h->ev)
        if (e)
            (void)ek_event_destroy(e);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    delete h;
    return EK_OK;
}

extern "C" int ek_tpt_paths_open(int device, int32_t n, const double *dense,
                                 const int64_t *indptr, const int32_t *cols,
                                 const double *vals, const int32_t *sources,
                                 int32_t n_sources, const int32_t *sinks, int32_t n_sinks,
                                 int32_t mode, int64_t num_paths, double total_flux,
                                 double flux_cutoff, int32_t max_paths, int32_t max_nodes,
                                 int32_t *caps_out, ek_tpt_paths **out)
{
    const char *who = "ek_tpt_paths_open";
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "%s: null output", who);
    *out = nullptr;
    if (n < 1 || n > TPT_PATH_MAX_N)
        return ek_set_error(EK_EARG, "%s: 1 <= n <= %d", who, TPT_PATH_MAX_N);
    if ((dense != nullptr) == (indptr != nullptr))
        return ek_set_error(EK_EARG, "%s: either a dense matrix or CSR arrays", who);
    if (!path_states_ok(sources, n_sources, n))
        return ek_set_error(EK_EARG, "%s: sources are indices below n, at least one", who);
    if (!path_states_ok(sinks, n_sinks, n))
        return ek_set_error(EK_EARG, "%s: sinks are indices below n, at least one", who);
    if (mode != PATH_KEEP && mode != PATH_SUBTRACT && mode != PATH_BOTTLENECK)
        return ek_set_error(EK_EARG, "%s: mode %d is none of keep (0), subtract (1), "
                                     "bottleneck (2)", who, mode);
    if (max_paths < 0 || max_paths > 4096 || max_nodes < 0)
        return ek_set_error(EK_EARG, "%s: a batch has 0 (the default) to 4096 paths and 0 "
                                     "(the default) or more nodes", who);
    int64_t nnz = 0;
    if (indptr) {
        nnz = indptr[n];
        if (indptr[0] != 0 || nnz < 0 || nnz > INT32_MAX || (nnz > 0 && (!cols || !vals)))
            return ek_set_error(EK_EARG, "%s: indptr does not span 0 .. 2^31 - 1 entries", who);
        for (int32_t i = 0; i < n; ++i) {
            if (indptr[i + 1] < indptr[i] || indptr[i + 1] > nnz)
                return ek_set_error(EK_EARG, "%s: indptr decreases at row %d", who, i);
            for (int64_t j = indptr[i]; j < indptr[i + 1]; ++j)
                if (cols[j] < 0 || cols[j] >= n || (j > indptr[i] && cols[j] <= cols[j - 1]))
                    return ek_set_error(EK_EARG, "%s: row %d is not sorted inside [0, %d)",
                                        who, i, n);
        }
    }
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess)
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
    }
    ek_tpt_paths *h = new (std::nothrow) ek_tpt_paths();
    int32_t *h_src = new (std::nothrow) int32_t[(size_t)n_sources];
    unsigned char *seen = new (std::nothrow) unsigned char[(size_t)n]();
    if (!h || !h_src || !seen) {
        delete h;
        delete[] h_src;
        delete[] seen;
        return ek_set_error(EK_ENOMEM, "%s: out of host memory", who);
    }
    // the distinct sources in the order of their first mention, the distinct sinks counted
    int32_t n_src = 0, n_sinks_distinct = 0;
    for (int32_t i = 0; i < n_sources; ++i)
        if (!(seen[sources[i]] & 1)) {
            seen[sources[i]] |= 1;
            h_src[n_src++] = sources[i];
        }
    for (int32_t i = 0; i < n_sinks; ++i)
        if (!(seen[sinks[i]] & 2)) {
            seen[sinks[i]] |= 2;
            n_sinks_distinct += 1;
        }
    delete[] seen;

    const size_t nn = (size_t)n * n;
    const size_t state_bytes = ((size_t)n * TPT_PATH_STATE_BYTES + 15) & ~(size_t)15;
    double *d_dense = nullptr;
    int32_t *d_cnt = nullptr;
    const unsigned rows_grid = (unsigned)((n + TPT_PATH_COMPACT_WG / EK_WAVE - 1) /
                                          (TPT_PATH_COMPACT_WG / EK_WAVE));
    PathState st0;
    float ms = 0.f;
    memset(&st0, 0, sizeof(st0));
    h->device = device;
    h->lds = n <= TPT_PATH_LDS_STATES;
    h->lds_bytes = h->lds ? state_bytes : 0;
    h->a.n = n;
    h->a.n_src = n_src;
    h->a.n_sinks = n_sinks;
    h->a.n_sinks_distinct = n_sinks_distinct;
    h->a.mode = mode;
    h->a.cap_paths = mode == PATH_KEEP ? 1 : max_paths ? max_paths : TPT_PATH_BATCH_PATHS;
    h->a.cap_nodes = max_nodes ? max_nodes : TPT_PATH_BATCH_NODES;
    h->node_buf = h->a.cap_nodes > n ? h->a.cap_nodes : n;
    h->a.num_paths = num_paths;
    h->a.total = total_flux;
    h->a.cutoff = flux_cutoff;

    rc = ek_mi_check_memory((dense ? nn * sizeof(double) : (size_t)nnz * 16) +
                                (size_t)n * 64 + (size_t)h->node_buf * 4, who);
    if (rc != EK_OK)
        goto done;
    PATH_HIP(ek_stream_create_flags(&h->s, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev)
        PATH_HIP(ek_event_create(&e));
    PATH_HIP(ek_dev_malloc(&h->indptr, ((size_t)n + 1) * sizeof(int64_t)));
    PATH_HIP(ek_dev_malloc(&h->src, (size_t)n_src * sizeof(int32_t)));
    PATH_HIP(ek_dev_malloc(&h->sinks, (size_t)n_sinks * sizeof(int32_t)));
    PATH_HIP(ek_dev_malloc(&h->a.pslot, (size_t)n * sizeof(int32_t)));
    PATH_HIP(ek_dev_malloc(&h->a.nodes, (size_t)h->node_buf * sizeof(int32_t)));
    PATH_HIP(ek_dev_malloc(&h->a.offsets, ((size_t)h->a.cap_paths + 1) * sizeof(int32_t)));
    PATH_HIP(ek_dev_malloc(&h->a.fluxes, (size_t)h->a.cap_paths * sizeof(double)));
    PATH_HIP(ek_dev_malloc(&h->a.state, sizeof(PathState)));
    if (!h->lds)
        PATH_HIP(ek_dev_malloc(&h->a.gstate, state_bytes));
    PATH_HIP(hipMemcpyAsync(h->src, h_src, (size_t)n_src * sizeof(int32_t),
                            hipMemcpyHostToDevice, h->s));
    PATH_HIP(hipMemcpyAsync(h->sinks, sinks, (size_t)n_sinks * sizeof(int32_t),
                            hipMemcpyHostToDevice, h->s));
    PATH_HIP(hipMemcpyAsync(h->a.state, &st0, sizeof(st0), hipMemcpyHostToDevice, h->s));
    if (dense) {
        PATH_HIP(ek_dev_malloc(&d_dense, nn * sizeof(double)));
        PATH_HIP(ek_dev_malloc(&d_cnt, (size_t)n * sizeof(int32_t)));
        PATH_HIP(hipMemcpyAsync(d_dense, dense, nn * sizeof(double), hipMemcpyHostToDevice,
                                h->s));
        PATH_HIP(hipEventRecord(h->ev[0], h->s));
        hipLaunchKernelGGL(tpt_path_count_kernel, dim3(rows_grid), dim3(TPT_PATH_COMPACT_WG), 0,
                           h->s, n, d_dense, d_cnt);
        hipLaunchKernelGGL(tpt_path_scan_kernel, dim3(1), dim3(TPT_PATH_SCAN_WG), 0, h->s, n,
                           d_cnt, h->indptr);
        PATH_HIP(hipGetLastError());
        PATH_HIP(hipMemcpyAsync(&nnz, h->indptr + n, sizeof(int64_t), hipMemcpyDeviceToHost,
                                h->s));
        PATH_HIP(hipStreamSynchronize(h->s));
        if (nnz < 0 || nnz > INT32_MAX) {
            rc = ek_set_error(EK_EARG, "%s: %lld entries > 0: more than 2^31 - 1", who,
                              (long long)nnz);
            goto done;
        }
    } else {
        PATH_HIP(hipMemcpyAsync(h->indptr, indptr, ((size_t)n + 1) * sizeof(int64_t),
                                hipMemcpyHostToDevice, h->s));
    }
    h->nnz = nnz;
    {
        // (a matrix without an entry still gets arrays to point at)
        const size_t slots = nnz > 0 ? (size_t)nnz : 1;
        PATH_HIP(ek_dev_malloc(&h->cols, slots * sizeof(int32_t)));
        PATH_HIP(ek_dev_malloc(&h->rowof, slots * sizeof(int32_t)));
        PATH_HIP(ek_dev_malloc(&h->a.vals, slots * sizeof(double)));
    }
    if (dense) {
        hipLaunchKernelGGL(tpt_path_fill_kernel, dim3(rows_grid), dim3(TPT_PATH_COMPACT_WG), 0,
                           h->s, n, d_dense, h->indptr, h->cols, h->a.vals, h->rowof);
    } else {
        if (nnz > 0) {
            PATH_HIP(hipMemcpyAsync(h->cols, cols, (size_t)nnz * sizeof(int32_t),
                                    hipMemcpyHostToDevice, h->s));
            PATH_HIP(hipMemcpyAsync(h->a.vals, vals, (size_t)nnz * sizeof(double),
                                    hipMemcpyHostToDevice, h->s));
        }
        PATH_HIP(hipEventRecord(h->ev[0], h->s));
        hipLaunchKernelGGL(tpt_path_rowof_kernel, dim3(rows_grid), dim3(TPT_PATH_COMPACT_WG), 0,
                           h->s, n, h->indptr, h->rowof);
    }
    PATH_HIP(hipGetLastError());
    PATH_HIP(hipEventRecord(h->ev[1], h->s));
    PATH_HIP(hipStreamSynchronize(h->s));
    PATH_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms_compact = ms;
    if (h->lds && h->lds_bytes > 48 * 1024)
        PATH_HIP(hipFuncSetAttribute((const void *)tpt_path_search_kernel<true>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)h->lds_bytes));
    h->a.indptr = h->indptr;
    h->a.cols = h->cols;
    h->a.rowof = h->rowof;
    h->a.src = h->src;
    h->a.sinks = h->sinks;
    if (caps_out) {
        caps_out[0] = h->a.cap_paths;
        caps_out[1] = h->node_buf;
    }
done:
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    (void)ek_dev_free(d_dense);
    (void)ek_dev_free(d_cnt);
    delete[] h_src;
    if (rc != EK_OK) {
        (void)ek_tpt_paths_close(h);
        return rc;
    }
    *out = h;
    return EK_OK;
}

extern "C" int ek_tpt_paths_next(ek_tpt_paths *h, int32_t *nodes_out, int32_t *offsets_out,
                                 double *fluxes_out, int32_t *count_out, int32_t *done_out,
                                 int32_t *info_out)
{
    const char *who = "ek_tpt_paths_next";
    int rc = path_bind(h, who);
    if (rc != EK_OK)
        return rc;
    if (!nodes_out || !offsets_out || !fluxes_out || !count_out || !done_out || !info_out)
        return ek_set_error(EK_EARG, "%s: null output", who);
    *count_out = 0;
    *done_out = 1;
    *info_out = PATH_INFO_OK;
    offsets_out[0] = 0;
    if (h->done)
        return EK_OK;
    PathState st;
    float ms = 0.f;
    PATH_HIP(hipEventRecord(h->ev[2], h->s));
    if (h->lds)
        hipLaunchKernelGGL(tpt_path_search_kernel<true>, dim3(1), dim3(TPT_PATH_WG),
                           h->lds_bytes, h->s, h->a);
    else
        hipLaunchKernelGGL(tpt_path_search_kernel<false>, dim3(1), dim3(TPT_PATH_WG), 0, h->s,
                           h->a);
    PATH_HIP(hipGetLastError());
    PATH_HIP(hipEventRecord(h->ev[3], h->s));
    PATH_HIP(hipMemcpyAsync(&st, h->a.state, sizeof(st), hipMemcpyDeviceToHost, h->s));
    PATH_HIP(hipStreamSynchronize(h->s));
    PATH_HIP(hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
    h->ms_search += ms;
    if (st.count < 0 || st.count > h->a.cap_paths || st.n_nodes < 0 || st.n_nodes > h->node_buf) {
        h->done = 1;
        return ek_set_error(EK_ESTATE, "%s: the batch reports %d paths, %d nodes", who,
                            st.count, st.n_nodes);
    }
    if (st.count > 0) {
        PATH_HIP(hipMemcpyAsync(nodes_out, h->a.nodes, (size_t)st.n_nodes * sizeof(int32_t),
                                hipMemcpyDeviceToHost, h->s));
        PATH_HIP(hipMemcpyAsync(offsets_out, h->a.offsets,
                                ((size_t)st.count + 1) * sizeof(int32_t), hipMemcpyDeviceToHost,
                                h->s));
        PATH_HIP(hipMemcpyAsync(fluxes_out, h->a.fluxes, (size_t)st.count * sizeof(double),
                                hipMemcpyDeviceToHost, h->s));
        PATH_HIP(hipStreamSynchronize(h->s));
    }
    h->n_paths += st.count;
    h->done = st.done;
    *count_out = st.count;
    *done_out = st.done;
    *info_out = st.info;
done:
    if (rc != EK_OK) {
        (void)hipStreamSynchronize(h->s);
        h->done = 1;
    }
    return rc;
}

extern "C" int ek_tpt_paths_stats(ek_tpt_paths *h, int64_t *counts_out, double *ms_out)
{
    const char *who = "ek_tpt_paths_stats";
    int rc = path_bind(h, who);
    if (rc != EK_OK)
        return rc;
    if (!counts_out || !ms_out)
        return ek_set_error(EK_EARG, "%s: null output", who);
    PathState st;
    PATH_HIP(hipMemcpyAsync(&st, h->a.state, sizeof(st), hipMemcpyDeviceToHost, h->s));
    PATH_HIP(hipStreamSynchronize(h->s));
    counts_out[0] = h->nnz;
    counts_out[1] = st.pops;
    counts_out[2] = h->n_paths;
    counts_out[3] = h->lds;
    ms_out[0] = h->ms_compact;
    ms_out[1] = h->ms_search;
done:
    return rc;
}
