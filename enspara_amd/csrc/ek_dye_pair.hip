// ek_dye_pair.hip -- donor-excitation Monte Carlo on a pair of dye MSMs.
//
// Replaces enspara/geometry/dye_lifetimes.py (resolve_excitation, explicit_static_dyes,
// fully_averaged_explict_dyes) and the per-pair arithmetic of
// enspara/geometry/explicit_r0_calc.py (calc_k2_r, calc_R0).  DESIGN.md 4m is the contract;
// in short:
//
// A handle holds P problems (a protein centre with its donor and its acceptor MSM), stored
//   side by side: per side the states of all problems in one numbering (problem p owns
//   off[p] .. off[p + 1]), their compressed rows (indptr, cols in that numbering, cdf), the
//   initial-state cdf and 9 doubles a state (emission centre, dipole origin, dipole vector);
//   per problem the constants K = {p_rad, p_nonrad, dt, c6, 1 / Td, 0} made by the host.
// A pair (dp_pair, the one function every kernel calls; its geometry up to FE is dp_geom of
//   ek_dye_geom.h, which ek_dye_bursts.hip calls too).  r2 = |centre_D - centre_A|^2, r =
//   sqrt(r2); rvec = origin_D - origin_A; cosT = A.D / (|A| |D|), cosD = rvec.D / (|rvec| |D|),
//   cosA = A.rvec / (|A| |rvec|); k2 = (cosT - 3 cosD cosA)^2; R0^6 = c6 k2; r6 = r2 r2 r2;
//   FE = R0^6 / (R0^6 + r6); kRET = (1 / Td) R0^6 / r6; p_RET = 1 - exp(-kRET dt); p = {p_rad,
//   p_nonrad, p_RET, 1 - p_rad - p_nonrad - p_RET}, and where the last is negative {p_rad,
//   p_nonrad, p_RET, 0} / their sum; cdf = cumsum(p) / cumsum(p)[3], three entries kept.
//   No root but the two norms' and r's; no sixth root at all.
// An excitation (chain c).  States d, a = the inverse initial cdf of u(DONOR, c, 0) and
//   u(ACCEPTOR, c, 0).  Step t: channel = the first cdf entry > u(DECAY, c, t) (3: still
//   excited), d hops with u(DONOR, c, t + 1), a with u(ACCEPTOR, c, t + 1), ++steps; it ends
//   unless the channel is 3.  A lane per live excitation, at most step_cap steps a launch;
//   every live excitation is at the same step, so (sample, d, a) is all that is carried.
//   After a launch the survivors are compacted in order (a ballot per wave, one workgroup's
//   prefix over the waves' counts, a scatter): integers only, the same list every run.  The
//   default step_cap is longer than any excitation measured: a call is as long as its longest
//   excitation whatever the lanes' use, and the compaction measured 7 % slower.
//   Results go to steps[sample], outcome[sample].  Trajectories are a replay with known
//   step counts into flat buffers at cumsum(steps + 1).
// A sample j of problem p is chain first_chain + p 2^32 + j.
// A side that has to hop from a row without nonzeros records the state (integer atomicMin)
// and stays; the caller raises.  No float atomics.
#include "ek_common.h"
#include "ek_dye_geom.h"
#include "ek_kmc_dev.h"
#include "ek_mi_launch.h"

#include <memory>
#include <new>

extern int ek_set_error(int code, const char *fmt, ...);

#define DP_HIP(call)                                                                \
    do {                                                                            \
        hipError_t e_ = (call);                                                     \
        if (e_ != hipSuccess)                                                       \
            return ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,           \
                                hipGetErrorString(e_), __FILE__, __LINE__);         \
    } while (0)

#define DP_WG 256
#define DP_K 6                  // doubles of a problem's constants
#define DP_STEP_CAP 65536       // steps of a launch unless the caller says otherwise: longer than
                                // any excitation measured, so one launch and no compaction
                                // (Measured: the compaction did not pay)
#define DP_MAX_STEPS ((int64_t)1 << 20)     // steps of an excitation unless the caller says
#define DP_TRAJ_CELLS ((int64_t)16 << 20)   // states of a side's trajectory buffer (64 MiB)
#define DP_NO_BAD 0xffffffffu
#define DP_EXCITED 3

static double dp_ms[3];         // upload, kernels, download of the last call

struct DpSide {
    KmcRows R;                  // all problems' rows; cols in the side's numbering
    const int64_t *off;         // [P + 1]
    const double *init;         // [n]: per problem cumsum(eq) / last
    const double *xyz;          // [n][9]
};

struct DpModel {
    DpSide D, A;
    const double *K;            // [P][DP_K]
    int32_t P;
};

struct DpPair {
    double k2, r, FE, cdf[3];
};

// ---- the pair ------------------------------------------------------------------------------
__device__ __forceinline__ void dp_pair(const double *__restrict__ d, const double *__restrict__ a,
                                        double p_rad, double p_nonrad, double dt, double c6,
                                        double inv_td, DpPair &q)
{
    DpGeom g;
    dp_geom(d, a, c6, g);       // (ek_dye_geom.h)
    q.k2 = g.k2;
    q.r = g.r;
    q.FE = g.FE;
    const double r06 = g.r06, r6 = g.r6;
    const double kret = inv_td * r06 / r6;
    const double p_ret = 1.0 - exp(-kret * dt);
    double p0 = p_rad, p1 = p_nonrad, p2 = p_ret, p3 = 1.0 - p_rad - p_nonrad - p_ret;
    if (p3 < 0.0) {
        const double sum = p0 + p1 + p2 + 0.0;
        p0 = p0 / sum;
        p1 = p1 / sum;
        p2 = p2 / sum;
        p3 = 0.0 / sum;
    }
    const double c1 = p0 + p1, c2 = c1 + p2, c3 = c2 + p3;
    q.cdf[0] = p0 / c3;
    q.cdf[1] = c1 / c3;
    q.cdf[2] = c2 / c3;
}

// the first of the four cdf entries (the fourth is 1) that is > u
__device__ __forceinline__ int dp_channel(const DpPair &q, double u)
{
    return (q.cdf[0] > u) ? 0 : (q.cdf[1] > u) ? 1 : (q.cdf[2] > u) ? 2 : DP_EXCITED;
}

// what a lane keeps of its problem for a launch
struct DpLane {
    double p_rad, p_nonrad, dt, c6, inv_td;
    uint64_t chain;
    int64_t d0, a0;             // the problem's first state of either side
};

__device__ __forceinline__ void dp_lane(const DpModel &M, uint64_t first_chain, int64_t n,
                                        int64_t sample, DpLane &L)
{
    const int64_t p = sample / n, j = sample - p * n;
    const double *K = M.K + p * DP_K;
    L.p_rad = K[0];
    L.p_nonrad = K[1];
    L.dt = K[2];
    L.c6 = K[3];
    L.inv_td = K[4];
    L.chain = first_chain + ((uint64_t)p << 32) + (uint64_t)j;
    L.d0 = M.D.off[p];
    L.a0 = M.A.off[p];
}

// the states chain L.chain starts in (u_d, u_a: index 0 of its donor and acceptor streams)
__device__ __forceinline__ void dp_initial(const DpModel &M, const DpLane &L, int64_t p,
                                           double u_d, double u_a, int32_t &sd, int32_t &sa)
{
    sd = (int32_t)kmc_upper(M.D.init, L.d0, M.D.off[p + 1], u_d);
    sa = (int32_t)kmc_upper(M.A.init, L.a0, M.A.off[p + 1], u_a);
}

// the doubles of both hops of step t (index t + 1 of either stream); call: the Philox call
// held in (d0, d1, a0, a1), ~0 for none
__device__ __forceinline__ void dp_hop_doubles(uint64_t seed, uint64_t chain, uint64_t t,
                                               uint64_t &call, double &d0, double &d1,
                                               double &a0, double &a1, double &ud, double &ua)
{
    const uint64_t h = t + 1;
    if ((h >> 1) != call) {
        call = h >> 1;
        kmc_pair(seed, KMC_DONOR, chain, call, d0, d1);
        kmc_pair(seed, KMC_ACCEPTOR, chain, call, a0, a1);
    }
    ud = (h & 1) ? d1 : d0;
    ua = (h & 1) ? a1 : a0;
}

// ---- kernels -------------------------------------------------------------------------------
// problem p: a lane per (donor state, acceptor state)
__global__ void __launch_bounds__(DP_WG)
dp_table_kernel(DpModel M, int32_t p, double *__restrict__ k2, double *__restrict__ r,
                double *__restrict__ fe, double *__restrict__ cdf)
{
    const int64_t d0 = M.D.off[p], a0 = M.A.off[p];
    const int64_t nd = M.D.off[p + 1] - d0, na = M.A.off[p + 1] - a0;
    const int64_t i = (int64_t)blockIdx.x * DP_WG + threadIdx.x;
    if (i >= nd * na)
        return;
    const int64_t sd = i / na, sa = i - sd * na;
    const double *K = M.K + (int64_t)p * DP_K;
    DpPair q;
    dp_pair(M.D.xyz + 9 * (d0 + sd), M.A.xyz + 9 * (a0 + sa), K[0], K[1], K[2], K[3], K[4], q);
    k2[i] = q.k2;
    r[i] = q.r;
    fe[i] = q.FE;
    cdf[3 * i] = q.cdf[0];
    cdf[3 * i + 1] = q.cdf[1];
    cdf[3 * i + 2] = q.cdf[2];
}

// steps t0 .. t0 + m - 1 of the n_live excitations of the list (live null: sample = position).
// sd, sa: the states by position, read unless t0 == 0, written for the survivors.  wmask[w]:
// the lanes of wave w (of the grid) that are still excited.
__global__ void __launch_bounds__(DP_WG)
dp_excite_kernel(DpModel M, uint64_t seed, uint64_t first_chain, int64_t n, int64_t n_live,
                 const int32_t *__restrict__ live, int32_t *__restrict__ sd_io,
                 int32_t *__restrict__ sa_io, int64_t t0, int64_t m, int32_t *__restrict__ steps,
                 int8_t *__restrict__ outcome, unsigned long long *__restrict__ wmask,
                 uint32_t *__restrict__ bad)
{
    const int64_t l = (int64_t)blockIdx.x * DP_WG + threadIdx.x;
    bool alive = false;
    if (l < n_live) {
        const int64_t sample = live ? (int64_t)live[l] : l;
        DpLane L;
        dp_lane(M, first_chain, n, sample, L);
        int32_t sd, sa;
        uint64_t hop_call = ~(uint64_t)0, dec_call = ~(uint64_t)0;
        double d0 = 0.0, d1 = 0.0, a0 = 0.0, a1 = 0.0, e0 = 0.0, e1 = 0.0;
        if (t0 == 0) {
            hop_call = 0;
            kmc_pair(seed, KMC_DONOR, L.chain, 0, d0, d1);
            kmc_pair(seed, KMC_ACCEPTOR, L.chain, 0, a0, a1);
            dp_initial(M, L, sample / n, d0, a0, sd, sa);
        } else {
            sd = sd_io[l];
            sa = sa_io[l];
        }
        int ch = DP_EXCITED;
        for (int64_t k = 0; k < m && ch == DP_EXCITED; ++k) {
            const uint64_t t = (uint64_t)(t0 + k);
            if ((t >> 1) != dec_call) {
                dec_call = t >> 1;
                kmc_pair(seed, KMC_DECAY, L.chain, dec_call, e0, e1);
            }
            double ud, ua;
            dp_hop_doubles(seed, L.chain, t, hop_call, d0, d1, a0, a1, ud, ua);
            DpPair q;
            dp_pair(M.D.xyz + 9 * (int64_t)sd, M.A.xyz + 9 * (int64_t)sa, L.p_rad, L.p_nonrad,
                    L.dt, L.c6, L.inv_td, q);
            ch = dp_channel(q, (t & 1) ? e1 : e0);
            sd = kmc_step_lane(M.D.R, sd, ud, bad);
            sa = kmc_step_lane(M.A.R, sa, ua, bad + 1);
            if (ch != DP_EXCITED) {
                steps[sample] = (int32_t)(t + 1);
                outcome[sample] = (int8_t)ch;
            }
        }
        alive = ch == DP_EXCITED;
        if (alive) {
            sd_io[l] = sd;
            sa_io[l] = sa;
        }
    }
    const unsigned long long mask = __ballot(alive);
    if ((threadIdx.x & (EK_WAVE - 1)) == 0)
        wmask[l / EK_WAVE] = mask;      // (whole waves: the grid is padded to workgroups)
}

// one workgroup: woff[w] = the survivors of the waves before w; ctl[2] = all survivors
__global__ void __launch_bounds__(DP_WG)
dp_scan_kernel(const unsigned long long *__restrict__ wmask, int64_t n_waves,
               uint32_t *__restrict__ woff, uint32_t *__restrict__ ctl)
{
    __shared__ uint32_t sh[DP_WG];
    uint32_t running = 0;
    for (int64_t base = 0; base < n_waves; base += DP_WG) {
        const int64_t w = base + threadIdx.x;
        const uint32_t v = w < n_waves ? (uint32_t)__popcll(wmask[w]) : 0u;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < DP_WG; off <<= 1) {
            const uint32_t add = (int)threadIdx.x >= off ? sh[threadIdx.x - off] : 0u;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (w < n_waves)
            woff[w] = running + sh[threadIdx.x] - v;
        running += sh[DP_WG - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        ctl[2] = running;
}

// the survivors of positions [0, n_live) move up, in order
__global__ void __launch_bounds__(DP_WG)
dp_compact_kernel(const unsigned long long *__restrict__ wmask, const uint32_t *__restrict__ woff,
                  int64_t n_live, const int32_t *__restrict__ live,
                  const int32_t *__restrict__ sd, const int32_t *__restrict__ sa,
                  int32_t *__restrict__ live_out, int32_t *__restrict__ sd_out,
                  int32_t *__restrict__ sa_out)
{
    const int64_t l = (int64_t)blockIdx.x * DP_WG + threadIdx.x;
    if (l >= n_live)
        return;
    const int lane = threadIdx.x & (EK_WAVE - 1);
    const unsigned long long mask = wmask[l / EK_WAVE];
    if (!((mask >> lane) & 1ull))
        return;
    const int64_t dst = (int64_t)woff[l / EK_WAVE] +
                        __popcll(mask & (((unsigned long long)1 << lane) - 1ull));
    live_out[dst] = live ? live[l] : (int32_t)l;
    sd_out[dst] = sd[l];
    sa_out[dst] = sa[l];
}

// the states of samples i0 .. i0 + cnt - 1 after the hops of steps t0 .. t0 + m - 1 (and the
// initial ones, t0 == 0): sample i's state s goes to traj[toff[i] - cell0 + s], the
// problem's own numbering.  cur: by sample.
__global__ void __launch_bounds__(DP_WG)
dp_replay_kernel(DpModel M, uint64_t seed, uint64_t first_chain, int64_t n, int64_t i0,
                 int64_t cnt, const int32_t *__restrict__ steps, const int64_t *__restrict__ toff,
                 int64_t cell0, int32_t *__restrict__ cur_d, int32_t *__restrict__ cur_a,
                 int64_t t0, int64_t m, int32_t *__restrict__ dtraj, int32_t *__restrict__ atraj,
                 uint32_t *__restrict__ bad)
{
    const int64_t k = (int64_t)blockIdx.x * DP_WG + threadIdx.x;
    if (k >= cnt)
        return;
    const int64_t sample = i0 + k, S = steps[sample];
    if (t0 >= S)
        return;
    DpLane L;
    dp_lane(M, first_chain, n, sample, L);
    const int64_t base = toff[sample] - cell0;
    int32_t sd, sa;
    uint64_t hop_call = ~(uint64_t)0;
    double d0 = 0.0, d1 = 0.0, a0 = 0.0, a1 = 0.0;
    if (t0 == 0) {
        hop_call = 0;
        kmc_pair(seed, KMC_DONOR, L.chain, 0, d0, d1);
        kmc_pair(seed, KMC_ACCEPTOR, L.chain, 0, a0, a1);
        dp_initial(M, L, sample / n, d0, a0, sd, sa);
        dtraj[base] = sd - (int32_t)L.d0;
        atraj[base] = sa - (int32_t)L.a0;
    } else {
        sd = cur_d[sample];
        sa = cur_a[sample];
    }
    const int64_t t1 = t0 + m < S ? t0 + m : S;
    for (int64_t t = t0; t < t1; ++t) {
        double ud, ua;
        dp_hop_doubles(seed, L.chain, (uint64_t)t, hop_call, d0, d1, a0, a1, ud, ua);
        sd = kmc_step_lane(M.D.R, sd, ud, bad);
        sa = kmc_step_lane(M.A.R, sa, ua, bad + 1);
        dtraj[base + t + 1] = sd - (int32_t)L.d0;
        atraj[base + t + 1] = sa - (int32_t)L.a0;
    }
    cur_d[sample] = sd;
    cur_a[sample] = sa;
}

// a lane per sample: the initial states of its chain, acceptor iff coin <= FE of that pair
// (fe_fixed null) or <= fe_fixed[problem]
__global__ void __launch_bounds__(DP_WG)
dp_static_kernel(DpModel M, uint64_t seed, uint64_t first_chain, int64_t n, int64_t total,
                 const double *__restrict__ fe_fixed, int8_t *__restrict__ acceptor,
                 int32_t *__restrict__ ds, int32_t *__restrict__ as)
{
    const int64_t i = (int64_t)blockIdx.x * DP_WG + threadIdx.x;
    if (i >= total)
        return;
    DpLane L;
    dp_lane(M, first_chain, n, i, L);
    int32_t sd, sa;
    dp_initial(M, L, i / n, kmc_uniform(seed, KMC_DONOR, L.chain, 0),
               kmc_uniform(seed, KMC_ACCEPTOR, L.chain, 0), sd, sa);
    double FE;
    if (fe_fixed) {
        FE = fe_fixed[i / n];
    } else {
        DpPair q;
        dp_pair(M.D.xyz + 9 * (int64_t)sd, M.A.xyz + 9 * (int64_t)sa, L.p_rad, L.p_nonrad, L.dt,
                L.c6, L.inv_td, q);
        FE = q.FE;
    }
    acceptor[i] = kmc_uniform(seed, KMC_FRET_COIN, L.chain, 0) <= FE ? 1 : 0;
    ds[i] = sd - (int32_t)L.d0;
    as[i] = sa - (int32_t)L.a0;
}

// ---- host ----------------------------------------------------------------------------------
// what a call allocated, released whichever way the call returns
struct DpScope {
    void *ptr[24];
    int n = 0;
    hipStream_t sync = nullptr;     // not owned: waited for before anything is freed
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    template <class T> hipError_t alloc(T **p, size_t bytes)
    {
        if (n >= 24)
            return hipErrorOutOfMemory;
        hipError_t e = ek_dev_malloc((void **)p, bytes ? bytes : 1);
        if (e == hipSuccess)
            ptr[n++] = (void *)*p;
        return e;
    }
    hipError_t events()
    {
        for (hipEvent_t &e : ev) {
            hipError_t r = ek_event_create(&e);
            if (r != hipSuccess)
                return r;
        }
        return hipSuccess;
    }
    ~DpScope()
    {
        if (sync)
            (void)hipStreamSynchronize(sync);
        for (int i = 0; i < n; ++i)
            (void)ek_dev_free(ptr[i]);
        for (hipEvent_t e : ev)
            if (e)
                (void)ek_event_destroy(e);
    }
};

struct DpSideMem {
    int64_t *off = nullptr, *indptr = nullptr;
    int32_t *cols = nullptr;
    double *cdf = nullptr, *init = nullptr, *xyz = nullptr;
    int64_t n = 0, nnz = 0;
};

struct ek_dye_pair {
    int device = 0;
    int32_t P = 0;
    DpSideMem D, A;
    double *K = nullptr;
    int64_t *h_doff = nullptr, *h_aoff = nullptr;   // host copies of the offsets
    hipStream_t s = nullptr;
};

static DpSide dp_side(const DpSideMem &m)
{
    DpSide S;
    S.R.indptr = m.indptr;
    S.R.cols = m.cols;
    S.R.cdf = m.cdf;
    S.R.n = (int32_t)m.n;
    S.off = m.off;
    S.init = m.init;
    S.xyz = m.xyz;
    return S;
}

static DpModel dp_model(const ek_dye_pair *h)
{
    DpModel M;
    M.D = dp_side(h->D);
    M.A = dp_side(h->A);
    M.K = h->K;
    M.P = h->P;
    return M;
}

static int dp_set_device(int device)
{
    hipError_t e0 = hipSetDevice(device);
    if (e0 != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
    return EK_OK;
}

static unsigned dp_blocks(int64_t items) { return (unsigned)((items + DP_WG - 1) / DP_WG); }

static int64_t dp_bad(uint32_t w) { return w == DP_NO_BAD ? (int64_t)-1 : (int64_t)w; }

// one side's arrays: the offsets ascend from 0 with a state at least per problem, the rows
// ascend from 0, every column lies in its row's problem
static int dp_check_side(int32_t P, const int64_t *off, const int64_t *indptr,
                         const int32_t *cols, const double *cdf, const double *init,
                         const double *xyz, const char *side)
{
    if (!off || !indptr || !init || !xyz || off[0] != 0 || indptr[0] != 0)
        return ek_set_error(EK_EARG, "ek_dye_pair_create: %s: null argument, or offsets that "
                                     "do not start at 0", side);
    for (int32_t p = 0; p < P; ++p)
        if (off[p + 1] <= off[p])
            return ek_set_error(EK_EARG, "ek_dye_pair_create: %s of problem %d has no state",
                                side, p);
    if (off[P] >= ((int64_t)1 << 31) - 1)
        return ek_set_error(EK_EARG, "ek_dye_pair_create: %s: 2^31 states or more", side);
    for (int64_t g = 0; g < off[P]; ++g)
        if (indptr[g + 1] < indptr[g])
            return ek_set_error(EK_EARG, "ek_dye_pair_create: %s: indptr descends at row %lld",
                                side, (long long)g);
    if (indptr[off[P]] > 0 && (!cols || !cdf))
        return ek_set_error(EK_EARG, "ek_dye_pair_create: %s: null argument", side);
    for (int32_t p = 0; p < P; ++p)
        for (int64_t k = indptr[off[p]]; k < indptr[off[p + 1]]; ++k)
            if (cols[k] < off[p] || cols[k] >= off[p + 1])
                return ek_set_error(EK_EARG, "ek_dye_pair_create: %s: column %d of entry %lld "
                                             "is no state of problem %d", side, cols[k],
                                    (long long)k, p);
    return EK_OK;
}

static size_t dp_side_bytes(int32_t P, const int64_t *off, const int64_t *indptr)
{
    const size_t n = (size_t)off[P], nnz = (size_t)indptr[off[P]];
    return (size_t)(P + 1) * 8 + (n + 1) * 8 + nnz * 12 + n * 8 + n * 72;
}

static hipError_t dp_upload_side(DpSideMem &m, int32_t P, const int64_t *off,
                                 const int64_t *indptr, const int32_t *cols, const double *cdf,
                                 const double *init, const double *xyz, hipStream_t s)
{
    m.n = off[P];
    m.nnz = indptr[m.n];
    const size_t ob = (size_t)(P + 1) * sizeof(int64_t), ib = (size_t)(m.n + 1) * sizeof(int64_t),
                 cb = (size_t)m.nnz * sizeof(int32_t), fb = (size_t)m.nnz * sizeof(double),
                 nb = (size_t)m.n * sizeof(double);
    hipError_t e = ek_dev_malloc(&m.off, ob);
    if (e == hipSuccess)
        e = ek_dev_malloc(&m.indptr, ib);
    if (e == hipSuccess)
        e = ek_dev_malloc(&m.cols, cb ? cb : 1);
    if (e == hipSuccess)
        e = ek_dev_malloc(&m.cdf, fb ? fb : 1);
    if (e == hipSuccess)
        e = ek_dev_malloc(&m.init, nb);
    if (e == hipSuccess)
        e = ek_dev_malloc(&m.xyz, 9 * nb);
    if (e == hipSuccess)
        e = hipMemcpyAsync(m.off, off, ob, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(m.indptr, indptr, ib, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && m.nnz > 0)
        e = hipMemcpyAsync(m.cols, cols, cb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && m.nnz > 0)
        e = hipMemcpyAsync(m.cdf, cdf, fb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(m.init, init, nb, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(m.xyz, xyz, 9 * nb, hipMemcpyHostToDevice, s);
    return e;
}

static void dp_free_side(DpSideMem &m)
{
    (void)ek_dev_free(m.off);
    (void)ek_dev_free(m.indptr);
    (void)ek_dev_free(m.cols);
    (void)ek_dev_free(m.cdf);
    (void)ek_dev_free(m.init);
    (void)ek_dev_free(m.xyz);
}

static void dp_release(ek_dye_pair *h)
{
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    dp_free_side(h->D);
    dp_free_side(h->A);
    (void)ek_dev_free(h->K);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    delete[] h->h_doff;
    delete[] h->h_aoff;
    delete h;
}

extern "C" int ek_dye_pair_create(int device, int32_t n_problems, const int64_t *d_off,
                                  const int64_t *d_indptr, const int32_t *d_cols,
                                  const double *d_cdf, const double *d_init, const double *d_xyz,
                                  const int64_t *a_off, const int64_t *a_indptr,
                                  const int32_t *a_cols, const double *a_cdf,
                                  const double *a_init, const double *a_xyz,
                                  const double *consts, ek_dye_pair **out)
{
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "ek_dye_pair_create: null argument");
    *out = nullptr;
    if (n_problems < 1 || n_problems > (1 << 27) || !consts)
        return ek_set_error(EK_EARG, "ek_dye_pair_create: 1 <= n_problems <= 2^27, consts");
    if ((rc = dp_check_side(n_problems, d_off, d_indptr, d_cols, d_cdf, d_init, d_xyz,
                            "the donors")) != EK_OK ||
        (rc = dp_check_side(n_problems, a_off, a_indptr, a_cols, a_cdf, a_init, a_xyz,
                            "the acceptors")) != EK_OK)
        return rc;
    if ((rc = dp_set_device(device)) != EK_OK)
        return rc;
    const size_t kb = (size_t)n_problems * DP_K * sizeof(double);
    if ((rc = ek_mi_check_memory(dp_side_bytes(n_problems, d_off, d_indptr) +
                                 dp_side_bytes(n_problems, a_off, a_indptr) + kb,
                                 "ek_dye_pair_create")) != EK_OK)
        return rc;
    ek_dye_pair *h = new (std::nothrow) ek_dye_pair();
    if (h) {
        h->h_doff = new (std::nothrow) int64_t[n_problems + 1];
        h->h_aoff = new (std::nothrow) int64_t[n_problems + 1];
    }
    if (!h || !h->h_doff || !h->h_aoff) {
        if (h)
            dp_release(h);
        return ek_set_error(EK_ENOMEM, "ek_dye_pair_create: out of host memory");
    }
    h->device = device;
    h->P = n_problems;
    for (int32_t p = 0; p <= n_problems; ++p) {
        h->h_doff[p] = d_off[p];
        h->h_aoff[p] = a_off[p];
    }
    hipError_t e = ek_stream_create_flags(&h->s, hipStreamNonBlocking);
    if (e == hipSuccess)
        e = dp_upload_side(h->D, n_problems, d_off, d_indptr, d_cols, d_cdf, d_init, d_xyz, h->s);
    if (e == hipSuccess)
        e = dp_upload_side(h->A, n_problems, a_off, a_indptr, a_cols, a_cdf, a_init, a_xyz, h->s);
    if (e == hipSuccess)
        e = ek_dev_malloc(&h->K, kb);
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->K, consts, kb, hipMemcpyHostToDevice, h->s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(h->s);
    if (e != hipSuccess) {
        rc = ek_set_error(EK_EHIP, "ek_dye_pair_create: %s", hipGetErrorString(e));
        dp_release(h);
        return rc;
    }
    *out = h;
    return EK_OK;
}

extern "C" int ek_dye_pair_destroy(ek_dye_pair *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    dp_release(h);
    return EK_OK;
}

static int dp_store_ms(DpScope &sc)
{
    float ms = 0.f;
    for (int q = 0; q < 3; ++q) {
        DP_HIP(hipEventElapsedTime(&ms, sc.ev[q], sc.ev[q + 1]));
        dp_ms[q] = ms;
    }
    return EK_OK;
}

extern "C" int ek_dye_pair_table(ek_dye_pair *h, int32_t problem, double *k2_out, double *r_out,
                                 double *fe_out, double *cdf_out)
{
    int rc = EK_OK;
    if (!h || problem < 0 || problem >= h->P || !k2_out || !r_out || !fe_out || !cdf_out)
        return ek_set_error(EK_EARG, "ek_dye_pair_table: null argument, or no such problem");
    const int64_t nd = h->h_doff[problem + 1] - h->h_doff[problem],
                  na = h->h_aoff[problem + 1] - h->h_aoff[problem];
    if (nd > ((int64_t)1 << 36) / na)
        return ek_set_error(EK_EARG, "ek_dye_pair_table: more than 2^36 pairs");
    const size_t pb = (size_t)(nd * na) * sizeof(double);
    if ((rc = dp_set_device(h->device)) != EK_OK ||
        (rc = ek_mi_check_memory(6 * pb + 256, "ek_dye_pair_table")) != EK_OK)
        return rc;
    DpScope sc;
    sc.sync = h->s;
    double *d_k2 = nullptr, *d_r = nullptr, *d_fe = nullptr, *d_cdf = nullptr;
    DP_HIP(sc.events());
    DP_HIP(sc.alloc(&d_k2, pb));
    DP_HIP(sc.alloc(&d_r, pb));
    DP_HIP(sc.alloc(&d_fe, pb));
    DP_HIP(sc.alloc(&d_cdf, 3 * pb));
    DP_HIP(hipEventRecord(sc.ev[0], h->s));
    DP_HIP(hipEventRecord(sc.ev[1], h->s));
    hipLaunchKernelGGL(dp_table_kernel, dim3(dp_blocks(nd * na)), dim3(DP_WG), 0, h->s,
                       dp_model(h), problem, d_k2, d_r, d_fe, d_cdf);
    DP_HIP(hipGetLastError());
    DP_HIP(hipEventRecord(sc.ev[2], h->s));
    DP_HIP(hipMemcpyAsync(k2_out, d_k2, pb, hipMemcpyDeviceToHost, h->s));
    DP_HIP(hipMemcpyAsync(r_out, d_r, pb, hipMemcpyDeviceToHost, h->s));
    DP_HIP(hipMemcpyAsync(fe_out, d_fe, pb, hipMemcpyDeviceToHost, h->s));
    DP_HIP(hipMemcpyAsync(cdf_out, d_cdf, 3 * pb, hipMemcpyDeviceToHost, h->s));
    DP_HIP(hipEventRecord(sc.ev[3], h->s));
    DP_HIP(hipStreamSynchronize(h->s));
    return dp_store_ms(sc);
}

// the chains of a call: sample j of problem p is chain first_chain + p 2^32 + j < 2^60
static int dp_check_chains(const ek_dye_pair *h, int64_t first_chain, int64_t n_samples,
                           const char *who)
{
    if (n_samples < 1 || n_samples >= ((int64_t)1 << 32) || first_chain < 0 ||
        first_chain >= ((int64_t)1 << 59) || n_samples > (((int64_t)1 << 31) - 1) / h->P)
        return ek_set_error(EK_EARG, "%s: 1 <= n_samples < 2^32, n_problems * n_samples < "
                                     "2^31, 0 <= first_chain < 2^59", who);
    return EK_OK;
}

// the first pass: steps and outcomes of every sample
static int dp_excite(ek_dye_pair *h, uint64_t seed, int64_t first_chain, int64_t n,
                     int64_t cap, int64_t max_steps, int32_t *steps_out, int8_t *outcomes_out,
                     int64_t *bad_out, int64_t *over_out)
{
    int rc = EK_OK;
    const int64_t N = (int64_t)h->P * n;
    const int64_t n_waves = (N + DP_WG - 1) / DP_WG * (DP_WG / EK_WAVE);
    if ((rc = ek_mi_check_memory((size_t)N * 29 + (size_t)n_waves * 12 + 1024,
                                 "ek_dye_pair_resolve")) != EK_OK)
        return rc;
    DpScope sc;
    sc.sync = h->s;
    hipStream_t s = h->s;
    int32_t *d_live[2] = {nullptr, nullptr}, *d_sd[2] = {nullptr, nullptr},
            *d_sa[2] = {nullptr, nullptr}, *d_steps = nullptr;
    int8_t *d_out = nullptr;
    unsigned long long *d_wmask = nullptr;
    uint32_t *d_woff = nullptr, *d_ctl = nullptr, ctl[4] = {DP_NO_BAD, DP_NO_BAD, 0, 0};
    DP_HIP(sc.events());
    for (int b = 0; b < 2; ++b) {
        DP_HIP(sc.alloc(&d_live[b], (size_t)N * sizeof(int32_t)));
        DP_HIP(sc.alloc(&d_sd[b], (size_t)N * sizeof(int32_t)));
        DP_HIP(sc.alloc(&d_sa[b], (size_t)N * sizeof(int32_t)));
    }
    DP_HIP(sc.alloc(&d_steps, (size_t)N * sizeof(int32_t)));
    DP_HIP(sc.alloc(&d_out, (size_t)N));
    DP_HIP(sc.alloc(&d_wmask, (size_t)n_waves * sizeof(unsigned long long)));
    DP_HIP(sc.alloc(&d_woff, (size_t)n_waves * sizeof(uint32_t)));
    DP_HIP(sc.alloc(&d_ctl, 4 * sizeof(uint32_t)));
    DP_HIP(hipEventRecord(sc.ev[0], s));
    DP_HIP(hipMemsetAsync(d_steps, 0, (size_t)N * sizeof(int32_t), s));
    DP_HIP(hipMemsetAsync(d_out, DP_EXCITED, (size_t)N, s));
    DP_HIP(hipMemcpyAsync(d_ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
    DP_HIP(hipStreamSynchronize(s));           // (ctl is read back into below)
    DP_HIP(hipEventRecord(sc.ev[1], s));
    const DpModel M = dp_model(h);
    int64_t n_live = N, t0 = 0;
    int cur = 0;
    const int32_t *live = nullptr;
    while (n_live > 0 && t0 < max_steps) {
        const int64_t m = max_steps - t0 < cap ? max_steps - t0 : cap;
        const int64_t waves = (n_live + DP_WG - 1) / DP_WG * (DP_WG / EK_WAVE);
        hipLaunchKernelGGL(dp_excite_kernel, dim3(dp_blocks(n_live)), dim3(DP_WG), 0, s, M, seed,
                           (uint64_t)first_chain, n, n_live, live, d_sd[cur], d_sa[cur], t0, m,
                           d_steps, d_out, d_wmask, d_ctl);
        hipLaunchKernelGGL(dp_scan_kernel, dim3(1), dim3(DP_WG), 0, s, d_wmask, waves, d_woff,
                           d_ctl);
        hipLaunchKernelGGL(dp_compact_kernel, dim3(dp_blocks(n_live)), dim3(DP_WG), 0, s, d_wmask,
                           d_woff, n_live, live, d_sd[cur], d_sa[cur], d_live[1 - cur],
                           d_sd[1 - cur], d_sa[1 - cur]);
        DP_HIP(hipGetLastError());
        DP_HIP(hipMemcpyAsync(ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
        DP_HIP(hipStreamSynchronize(s));
        n_live = (int64_t)ctl[2];
        cur = 1 - cur;
        live = d_live[cur];
        t0 += m;
    }
    DP_HIP(hipEventRecord(sc.ev[2], s));
    int32_t first_over = -1;
    if (n_live > 0)
        DP_HIP(hipMemcpyAsync(&first_over, live, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DP_HIP(hipMemcpyAsync(steps_out, d_steps, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost,
                          s));
    DP_HIP(hipMemcpyAsync(outcomes_out, d_out, (size_t)N, hipMemcpyDeviceToHost, s));
    DP_HIP(hipEventRecord(sc.ev[3], s));
    DP_HIP(hipStreamSynchronize(s));
    bad_out[0] = dp_bad(ctl[0]);
    bad_out[1] = dp_bad(ctl[1]);
    *over_out = first_over;
    return dp_store_ms(sc);
}

// the second pass: steps known, the states of every sample into the flat outputs
static int dp_replay(ek_dye_pair *h, uint64_t seed, int64_t first_chain, int64_t n, int64_t cap,
                     const int32_t *steps, int32_t *dtraj_out, int32_t *atraj_out,
                     int64_t traj_cells, int64_t *bad_out)
{
    int rc = EK_OK;
    const int64_t N = (int64_t)h->P * n;
    std::unique_ptr<int64_t[]> toff(new (std::nothrow) int64_t[N + 1]);
    if (!toff)
        return ek_set_error(EK_ENOMEM, "ek_dye_pair_resolve: out of host memory");
    toff[0] = 0;
    int64_t longest = 0;
    for (int64_t i = 0; i < N; ++i) {
        if (steps[i] < 1 || steps[i] > DP_TRAJ_CELLS - 1)
            return ek_set_error(EK_EARG, "ek_dye_pair_resolve: %d steps of sample %lld: a "
                                         "trajectory has 1 to 2^24 - 1", steps[i], (long long)i);
        toff[i + 1] = toff[i] + steps[i] + 1;
        longest = steps[i] > longest ? steps[i] : longest;
    }
    if (toff[N] != traj_cells)
        return ek_set_error(EK_EARG, "ek_dye_pair_resolve: traj_cells = %lld, the steps ask for "
                                     "%lld", (long long)traj_cells, (long long)toff[N]);
    const int64_t cells = toff[N] < DP_TRAJ_CELLS ? toff[N] : DP_TRAJ_CELLS;
    if ((rc = ek_mi_check_memory((size_t)N * 20 + (size_t)cells * 8 + 1024,
                                 "ek_dye_pair_resolve")) != EK_OK)
        return rc;
    DpScope sc;
    sc.sync = h->s;
    hipStream_t s = h->s;
    int32_t *d_steps = nullptr, *d_cd = nullptr, *d_ca = nullptr, *d_dt = nullptr, *d_at = nullptr;
    int64_t *d_toff = nullptr;
    uint32_t *d_ctl = nullptr, ctl[4] = {DP_NO_BAD, DP_NO_BAD, 0, 0};
    float ms = 0.f;
    DP_HIP(sc.events());
    DP_HIP(sc.alloc(&d_steps, (size_t)N * sizeof(int32_t)));
    DP_HIP(sc.alloc(&d_toff, (size_t)N * sizeof(int64_t)));
    DP_HIP(sc.alloc(&d_cd, (size_t)N * sizeof(int32_t)));
    DP_HIP(sc.alloc(&d_ca, (size_t)N * sizeof(int32_t)));
    DP_HIP(sc.alloc(&d_dt, (size_t)cells * sizeof(int32_t)));
    DP_HIP(sc.alloc(&d_at, (size_t)cells * sizeof(int32_t)));
    DP_HIP(sc.alloc(&d_ctl, 4 * sizeof(uint32_t)));
    DP_HIP(hipEventRecord(sc.ev[0], s));
    DP_HIP(hipMemcpyAsync(d_steps, steps, (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, s));
    DP_HIP(hipMemcpyAsync(d_toff, toff.get(), (size_t)N * sizeof(int64_t), hipMemcpyHostToDevice,
                          s));
    DP_HIP(hipMemcpyAsync(d_ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, s));
    DP_HIP(hipEventRecord(sc.ev[1], s));
    DP_HIP(hipStreamSynchronize(s));
    DP_HIP(hipEventElapsedTime(&ms, sc.ev[0], sc.ev[1]));
    dp_ms[0] = ms;
    dp_ms[1] = dp_ms[2] = 0.0;
    const DpModel M = dp_model(h);
    // samples i0 .. i1 - 1: as many as the buffers hold (one always fits)
    for (int64_t i0 = 0, i1; i0 < N; i0 = i1) {
        int64_t most = 0;
        for (i1 = i0; i1 < N && toff[i1 + 1] - toff[i0] <= cells; ++i1)
            most = steps[i1] > most ? steps[i1] : most;
        DP_HIP(hipEventRecord(sc.ev[1], s));
        for (int64_t t0 = 0; t0 < most; t0 += cap) {
            hipLaunchKernelGGL(dp_replay_kernel, dim3(dp_blocks(i1 - i0)), dim3(DP_WG), 0, s, M,
                               seed, (uint64_t)first_chain, n, i0, i1 - i0, d_steps, d_toff,
                               toff[i0], d_cd, d_ca, t0, cap, d_dt, d_at, d_ctl);
            DP_HIP(hipGetLastError());
        }
        DP_HIP(hipEventRecord(sc.ev[2], s));
        const size_t gb = (size_t)(toff[i1] - toff[i0]) * sizeof(int32_t);
        DP_HIP(hipMemcpyAsync(dtraj_out + toff[i0], d_dt, gb, hipMemcpyDeviceToHost, s));
        DP_HIP(hipMemcpyAsync(atraj_out + toff[i0], d_at, gb, hipMemcpyDeviceToHost, s));
        DP_HIP(hipEventRecord(sc.ev[3], s));
        DP_HIP(hipStreamSynchronize(s));
        DP_HIP(hipEventElapsedTime(&ms, sc.ev[1], sc.ev[2]));
        dp_ms[1] += ms;
        DP_HIP(hipEventElapsedTime(&ms, sc.ev[2], sc.ev[3]));
        dp_ms[2] += ms;
    }
    DP_HIP(hipMemcpyAsync(ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    DP_HIP(hipStreamSynchronize(s));
    bad_out[0] = dp_bad(ctl[0]);
    bad_out[1] = dp_bad(ctl[1]);
    return EK_OK;
}

extern "C" int ek_dye_pair_resolve(ek_dye_pair *h, uint64_t seed, int64_t first_chain,
                                   int64_t n_samples, int64_t step_cap, int64_t max_steps,
                                   int32_t *steps, int8_t *outcomes_out, int32_t *dtraj_out,
                                   int32_t *atraj_out, int64_t traj_cells, int64_t *bad_out,
                                   int64_t *over_out)
{
    int rc = EK_OK;
    const bool replay = dtraj_out != nullptr;
    if (!h || !steps || !bad_out || !over_out || (!replay && !outcomes_out) ||
        (replay != (atraj_out != nullptr)) || step_cap < 0 || max_steps < 0 ||
        max_steps > DP_TRAJ_CELLS - 1)
        return ek_set_error(EK_EARG, "ek_dye_pair_resolve: null argument, step_cap < 0, or "
                                     "max_steps outside [0, 2^24 - 1]");
    if ((rc = dp_check_chains(h, first_chain, n_samples, "ek_dye_pair_resolve")) != EK_OK)
        return rc;
    bad_out[0] = bad_out[1] = -1;
    *over_out = -1;
    if ((rc = dp_set_device(h->device)) != EK_OK)
        return rc;
    const int64_t cap = step_cap > 0 ? step_cap : DP_STEP_CAP;
    if (replay)
        return dp_replay(h, seed, first_chain, n_samples, cap, steps, dtraj_out, atraj_out,
                         traj_cells, bad_out);
    return dp_excite(h, seed, first_chain, n_samples, cap, max_steps > 0 ? max_steps : DP_MAX_STEPS,
                     steps, outcomes_out, bad_out, over_out);
}

extern "C" int ek_dye_pair_static(ek_dye_pair *h, uint64_t seed, int64_t first_chain,
                                  int64_t n_samples, const double *fe_fixed, int8_t *acceptor_out,
                                  int32_t *dstate_out, int32_t *astate_out)
{
    int rc = EK_OK;
    if (!h || !acceptor_out || !dstate_out || !astate_out)
        return ek_set_error(EK_EARG, "ek_dye_pair_static: null argument");
    if ((rc = dp_check_chains(h, first_chain, n_samples, "ek_dye_pair_static")) != EK_OK)
        return rc;
    const int64_t N = (int64_t)h->P * n_samples;
    if ((rc = dp_set_device(h->device)) != EK_OK ||
        (rc = ek_mi_check_memory((size_t)N * 9 + (size_t)h->P * 8 + 256,
                                 "ek_dye_pair_static")) != EK_OK)
        return rc;
    DpScope sc;
    sc.sync = h->s;
    hipStream_t s = h->s;
    int8_t *d_acc = nullptr;
    int32_t *d_ds = nullptr, *d_as = nullptr;
    double *d_fe = nullptr;
    DP_HIP(sc.events());
    DP_HIP(sc.alloc(&d_acc, (size_t)N));
    DP_HIP(sc.alloc(&d_ds, (size_t)N * sizeof(int32_t)));
    DP_HIP(sc.alloc(&d_as, (size_t)N * sizeof(int32_t)));
    if (fe_fixed)
        DP_HIP(sc.alloc(&d_fe, (size_t)h->P * sizeof(double)));
    DP_HIP(hipEventRecord(sc.ev[0], s));
    if (fe_fixed)
        DP_HIP(hipMemcpyAsync(d_fe, fe_fixed, (size_t)h->P * sizeof(double),
                              hipMemcpyHostToDevice, s));
    DP_HIP(hipEventRecord(sc.ev[1], s));
    hipLaunchKernelGGL(dp_static_kernel, dim3(dp_blocks(N)), dim3(DP_WG), 0, s, dp_model(h), seed,
                       (uint64_t)first_chain, n_samples, N, d_fe, d_acc, d_ds, d_as);
    DP_HIP(hipGetLastError());
    DP_HIP(hipEventRecord(sc.ev[2], s));
    DP_HIP(hipMemcpyAsync(acceptor_out, d_acc, (size_t)N, hipMemcpyDeviceToHost, s));
    DP_HIP(hipMemcpyAsync(dstate_out, d_ds, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost,
                          s));
    DP_HIP(hipMemcpyAsync(astate_out, d_as, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost,
                          s));
    DP_HIP(hipEventRecord(sc.ev[3], s));
    DP_HIP(hipStreamSynchronize(s));
    return dp_store_ms(sc);
}

extern "C" int ek_dye_pair_last_timing(double *ms_out)
{
    if (!ms_out)
        return ek_set_error(EK_EARG, "ek_dye_pair_last_timing: null argument");
    for (int i = 0; i < 3; ++i)
        ms_out[i] = dp_ms[i];
    return EK_OK;
}
