// ek_dye_bursts.hip -- smFRET bursts with explicitly modelled dyes: two photon rules on the
// burst loop of ek_kmc_burst.h.
//
// Replaces enspara/geometry/dye_lifetimes.py (_sample_lifetimes_guarenteed_photon,
// sample_lifetimes_guarenteed_photon, the sampling of run_mc) and
// enspara/geometry/explicit_r0_calc.py (sample_dye_coords, _simulate_burst_k2,
// simulate_burst_k2).  DESIGN.md 4n is the contract; in short:
//
// The chain of burst b is that of ek_kmc_fret_bursts: chain first_burst + b, KMC_INIT, KMC_TRANS.
// Photon ph of it draws from (seed, chain, ph) alone, on streams of its own.
// The pick.  pick(u, m) = min(m - 1, (int64)(u * (double)m)), m < 2^31.  The product is rounded
//   once; the clamp keeps the index inside the list whatever it rounds to (for the Philox
//   doubles, u <= 1 - 2^-53, round-to-nearest leaves it below m: DESIGN.md 4n has the
//   argument; the clamp does not lean on it).  One draw among the photon events is the
//   distribution of the reference's uniform draw with redraws of the non-radiative ones.
// Lifetime rule.  Per protein state the photon events of its excitations (the host compacted
//   the event list: radiative -> flag 0, energy transfer -> flag 1, in the list's order), ragged:
//   ev_off [n + 1], ev_life, ev_flag.  The photon takes entry ev_off[s] + pick(u(KMC_EVENT), m_s)
//   and writes its flag byte and its lifetime.
// Kappa-squared rule.  Per protein state the conformations of either dye, rows of 9 doubles,
//   ragged: d_off, d_xyz, a_off, a_xyz.  The photon takes donor row pick(u(KMC_DCONF), nd_s) and
//   acceptor row pick(u(KMC_ACONF), na_s), their k2, r and FE = c6 k2 / (c6 k2 + r2 r2 r2)
//   (dp_geom of ek_dye_geom.h: the bits of the pair table), flag = u(KMC_COIN) <= FE.
// A photon in a state with nothing to pick from records the state (integer atomicMin, the
// second bad word of the loop) and writes zeros; the caller raises.  Every photon also writes
// the state it was emitted from.  No float atomics: every run gives the same bits.
// The per-entry calls run the same rule functions on a list of states: entry k of chain c draws
// what photon k of burst c draws.
#include "ek_dye_geom.h"
#include "ek_kmc_burst.h"

#define DB_MAX_PICK (((int64_t)1 << 31) - 1)    // entries of a state's list: m < 2^31

static double db_ms[3];         // upload, kernels, download of the last call

__device__ __forceinline__ int64_t db_pick(double u, int64_t m)
{
    const int64_t j = (int64_t)(u * (double)m);
    return j < m - 1 ? j : m - 1;
}

// ---- the rules -----------------------------------------------------------------------------
struct DbLifeRule {
    uint64_t seed;
    const int64_t *ev_off;
    const double *ev_life;
    const uint8_t *ev_flag;
    uint8_t *flags;
    double *life;
    int32_t *states;            // null in a per-entry call
    uint32_t *bad;
    __device__ __forceinline__ void none(int64_t k) const
    {
        flags[k] = 0;
        life[k] = 0.0;
    }
    __device__ __forceinline__ void photon(int32_t s, uint64_t chain, uint64_t ph, int64_t k) const
    {
        if (states)
            states[k] = s;
        const int64_t lo = ev_off[s], m = ev_off[s + 1] - lo;
        if (m <= 0) {
            atomicMin(bad, (uint32_t)s);
            none(k);
            return;
        }
        const int64_t e = lo + db_pick(kmc_uniform(seed, KMC_EVENT, chain, ph), m);
        flags[k] = ev_flag[e];
        life[k] = ev_life[e];
    }
};

struct DbK2Rule {
    uint64_t seed;
    const int64_t *d_off, *a_off;
    const double *d_xyz, *a_xyz;
    double c6;
    uint8_t *flags;
    double *k2, *r;
    int32_t *states;            // null in a per-entry call
    int32_t *drow, *arow;       // null unless asked for
    uint32_t *bad;
    __device__ __forceinline__ void none(int64_t k) const
    {
        flags[k] = 0;
        k2[k] = 0.0;
        r[k] = 0.0;
        if (drow) {
            drow[k] = -1;
            arow[k] = -1;
        }
    }
    __device__ __forceinline__ void photon(int32_t s, uint64_t chain, uint64_t ph, int64_t k) const
    {
        if (states)
            states[k] = s;
        const int64_t d0 = d_off[s], nd = d_off[s + 1] - d0, a0 = a_off[s], na = a_off[s + 1] - a0;
        if (nd <= 0 || na <= 0) {
            atomicMin(bad, (uint32_t)s);
            none(k);
            return;
        }
        const int64_t i = db_pick(kmc_uniform(seed, KMC_DCONF, chain, ph), nd);
        const int64_t j = db_pick(kmc_uniform(seed, KMC_ACONF, chain, ph), na);
        DpGeom g;
        dp_geom(d_xyz + 9 * (d0 + i), a_xyz + 9 * (a0 + j), c6, g);
        flags[k] = kmc_uniform(seed, KMC_COIN, chain, ph) <= g.FE ? 1 : 0;
        k2[k] = g.k2;
        r[k] = g.r;
        if (drow) {
            drow[k] = (int32_t)i;
            arow[k] = (int32_t)j;
        }
    }
};

// ---- the per-entry kernels ---------------------------------------------------------------------
template <class Rule>
__global__ void __launch_bounds__(KMC_WG)
db_photons_kernel(Rule rule, uint64_t chain, int64_t n, const int32_t *__restrict__ states,
                  int32_t n_states)
{
    const int64_t k = (int64_t)blockIdx.x * KMC_WG + threadIdx.x;
    if (k >= n)
        return;
    const int32_t s = states[k];
    if (s < 0 || s >= n_states) {   // (the host has checked; never out of bounds)
        rule.none(k);
        return;
    }
    rule.photon(s, chain, (uint64_t)k, k);
}

__global__ void __launch_bounds__(KMC_WG)
db_pick_kernel(int64_t n, const int32_t *__restrict__ states, const double *__restrict__ u,
               int32_t n_states, const int64_t *__restrict__ ev_off, int64_t *__restrict__ index,
               uint32_t *__restrict__ bad)
{
    const int64_t k = (int64_t)blockIdx.x * KMC_WG + threadIdx.x;
    if (k >= n)
        return;
    const int32_t s = states[k];
    if (s < 0 || s >= n_states) {   // (the host has checked)
        index[k] = -1;
        return;
    }
    const int64_t m = ev_off[s + 1] - ev_off[s];
    if (m <= 0) {
        atomicMin(bad, (uint32_t)s);
        index[k] = -1;
        return;
    }
    index[k] = db_pick(u[k], m);
}

// ---- host ----------------------------------------------------------------------------------
// offsets of a ragged table over the states: they start at 0, do not descend, and no state
// has 2^31 entries or more (a state may have none)
static int db_check_off(int32_t n_states, const int64_t *off, const char *what, const char *who)
{
    if (n_states < 1 || !off || off[0] != 0)
        return ek_set_error(EK_EARG, "%s: %s: n_states >= 1, offsets from 0", who, what);
    for (int32_t i = 0; i < n_states; ++i)
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > DB_MAX_PICK)
            return ek_set_error(EK_EARG, "%s: %s: the offsets descend at state %d, or it has "
                                         "2^31 entries or more", who, what, i);
    return EK_OK;
}

// the lifetime rule's host side (kmc_run_bursts; the per-entry call)
struct DbLifePlan {
    int32_t n_states;
    const int64_t *ev_off;
    const double *ev_life;
    const uint8_t *ev_flag;
    double *life_out;
    int32_t *states_out;        // null: a per-entry call
    int64_t *d_off = nullptr;
    double *d_life = nullptr, *d_out = nullptr;
    uint8_t *d_flag = nullptr;
    int32_t *d_states = nullptr;
    size_t bytes(int64_t n_ph) const
    {
        return (size_t)(n_states + 1) * 8 + (size_t)ev_off[n_states] * 9 + (size_t)n_ph * 12;
    }
    int upload(KmcScope &sc, hipStream_t s, int64_t n_ph)
    {
        KMC_HIP(sc.upload(&d_off, ev_off, (size_t)n_states + 1, s));
        KMC_HIP(sc.upload(&d_life, ev_life, (size_t)ev_off[n_states], s));
        KMC_HIP(sc.upload(&d_flag, ev_flag, (size_t)ev_off[n_states], s));
        KMC_HIP(sc.alloc(&d_out, (size_t)n_ph * sizeof(double)));
        if (states_out)
            KMC_HIP(sc.alloc(&d_states, (size_t)n_ph * sizeof(int32_t)));
        return EK_OK;
    }
    DbLifeRule rule(uint64_t seed, uint8_t *d_flags, uint32_t *d_bad) const
    {
        return DbLifeRule{seed, d_off, d_life, d_flag, d_flags, d_out, d_states, d_bad};
    }
    int download(hipStream_t s, int64_t n_ph)
    {
        KMC_HIP(hipMemcpyAsync(life_out, d_out, (size_t)n_ph * sizeof(double),
                               hipMemcpyDeviceToHost, s));
        if (states_out)
            KMC_HIP(hipMemcpyAsync(states_out, d_states, (size_t)n_ph * sizeof(int32_t),
                                   hipMemcpyDeviceToHost, s));
        return EK_OK;
    }
};

// the kappa-squared rule's
struct DbK2Plan {
    int32_t n_states;
    const int64_t *d_off, *a_off;
    const double *d_xyz, *a_xyz;
    double c6;
    double *k2_out, *r_out;
    int32_t *states_out;        // null: a per-entry call
    int32_t *drow_out, *arow_out;   // both or neither
    int64_t *g_doff = nullptr, *g_aoff = nullptr;
    double *g_dxyz = nullptr, *g_axyz = nullptr, *g_k2 = nullptr, *g_r = nullptr;
    int32_t *g_states = nullptr, *g_drow = nullptr, *g_arow = nullptr;
    size_t bytes(int64_t n_ph) const
    {
        return (size_t)(n_states + 1) * 16 + (size_t)(d_off[n_states] + a_off[n_states]) * 72 +
               (size_t)n_ph * 28;
    }
    int upload(KmcScope &sc, hipStream_t s, int64_t n_ph)
    {
        KMC_HIP(sc.upload(&g_doff, d_off, (size_t)n_states + 1, s));
        KMC_HIP(sc.upload(&g_aoff, a_off, (size_t)n_states + 1, s));
        KMC_HIP(sc.upload(&g_dxyz, d_xyz, (size_t)d_off[n_states] * 9, s));
        KMC_HIP(sc.upload(&g_axyz, a_xyz, (size_t)a_off[n_states] * 9, s));
        KMC_HIP(sc.alloc(&g_k2, (size_t)n_ph * sizeof(double)));
        KMC_HIP(sc.alloc(&g_r, (size_t)n_ph * sizeof(double)));
        if (states_out)
            KMC_HIP(sc.alloc(&g_states, (size_t)n_ph * sizeof(int32_t)));
        if (drow_out) {
            KMC_HIP(sc.alloc(&g_drow, (size_t)n_ph * sizeof(int32_t)));
            KMC_HIP(sc.alloc(&g_arow, (size_t)n_ph * sizeof(int32_t)));
        }
        return EK_OK;
    }
    DbK2Rule rule(uint64_t seed, uint8_t *d_flags, uint32_t *d_bad) const
    {
        return DbK2Rule{seed, g_doff, g_aoff, g_dxyz, g_axyz, c6, d_flags, g_k2, g_r, g_states,
                        g_drow, g_arow, d_bad};
    }
    int download(hipStream_t s, int64_t n_ph)
    {
        const size_t fb = (size_t)n_ph * sizeof(double), ib = (size_t)n_ph * sizeof(int32_t);
        KMC_HIP(hipMemcpyAsync(k2_out, g_k2, fb, hipMemcpyDeviceToHost, s));
        KMC_HIP(hipMemcpyAsync(r_out, g_r, fb, hipMemcpyDeviceToHost, s));
        if (states_out)
            KMC_HIP(hipMemcpyAsync(states_out, g_states, ib, hipMemcpyDeviceToHost, s));
        if (drow_out) {
            KMC_HIP(hipMemcpyAsync(drow_out, g_drow, ib, hipMemcpyDeviceToHost, s));
            KMC_HIP(hipMemcpyAsync(arow_out, g_arow, ib, hipMemcpyDeviceToHost, s));
        }
        return EK_OK;
    }
};

static int db_check_k2(int32_t n_states, const int64_t *d_off, const double *d_xyz,
                       const int64_t *a_off, const double *a_xyz, const int32_t *drow_out,
                       const int32_t *arow_out, const char *who)
{
    int rc = EK_OK;
    if ((rc = db_check_off(n_states, d_off, "donor conformations", who)) != EK_OK ||
        (rc = db_check_off(n_states, a_off, "acceptor conformations", who)) != EK_OK)
        return rc;
    if ((d_off[n_states] > 0 && !d_xyz) || (a_off[n_states] > 0 && !a_xyz) ||
        ((drow_out != nullptr) != (arow_out != nullptr)))
        return ek_set_error(EK_EARG, "%s: null conformations, or one of the two row outputs", who);
    return EK_OK;
}

extern "C" int ek_dye_bursts_lifetimes(ek_kmc *h, uint64_t seed, int64_t first_burst,
                                       int64_t n_bursts, const int64_t *frame_off,
                                       const int64_t *frames, const double *pop_cdf,
                                       const int64_t *ev_off, const double *ev_life,
                                       const uint8_t *ev_flag, int64_t step_cap,
                                       uint8_t *flags_out, double *life_out, int32_t *states_out,
                                       int32_t *traj_out, int64_t *bad_row_out,
                                       int64_t *bad_state_out)
{
    const char *who = "ek_dye_bursts_lifetimes";
    int rc = EK_OK;
    if (!h || !life_out || !states_out || !bad_state_out)
        return ek_set_error(EK_EARG, "%s: null argument", who);
    if ((rc = db_check_off(h->n, ev_off, "photon events", who)) != EK_OK)
        return rc;
    if (ev_off[h->n] > 0 && (!ev_life || !ev_flag))
        return ek_set_error(EK_EARG, "%s: null argument", who);
    DbLifePlan plan{h->n, ev_off, ev_life, ev_flag, life_out, states_out};
    return kmc_run_bursts(h, who, db_ms, seed, first_burst, n_bursts, frame_off, frames, pop_cdf,
                          step_cap, flags_out, traj_out, bad_row_out, bad_state_out, plan);
}

extern "C" int ek_dye_bursts_k2(ek_kmc *h, uint64_t seed, int64_t first_burst, int64_t n_bursts,
                                const int64_t *frame_off, const int64_t *frames,
                                const double *pop_cdf, const int64_t *d_off, const double *d_xyz,
                                const int64_t *a_off, const double *a_xyz, double c6,
                                int64_t step_cap, uint8_t *flags_out, double *k2_out,
                                double *r_out, int32_t *states_out, int32_t *drow_out,
                                int32_t *arow_out, int32_t *traj_out, int64_t *bad_row_out,
                                int64_t *bad_state_out)
{
    const char *who = "ek_dye_bursts_k2";
    int rc = EK_OK;
    if (!h || !k2_out || !r_out || !states_out || !bad_state_out)
        return ek_set_error(EK_EARG, "%s: null argument", who);
    if ((rc = db_check_k2(h->n, d_off, d_xyz, a_off, a_xyz, drow_out, arow_out, who)) != EK_OK)
        return rc;
    DbK2Plan plan{h->n, d_off, a_off, d_xyz, a_xyz, c6, k2_out, r_out, states_out, drow_out,
                  arow_out};
    return kmc_run_bursts(h, who, db_ms, seed, first_burst, n_bursts, frame_off, frames, pop_cdf,
                          step_cap, flags_out, traj_out, bad_row_out, bad_state_out, plan);
}

// entry k of `states` under the plan's rule, as photon k of burst `chain`
template <class Plan>
static int db_run_photons(int device, const char *who, uint64_t seed, int64_t chain, int64_t n,
                          const int32_t *states, int32_t n_states, uint8_t *flags_out,
                          int64_t *bad_state_out, Plan &plan)
{
    int rc = EK_OK;
    if (n < 1 || n > ((int64_t)1 << 36) || !states || !flags_out || !bad_state_out || chain < 0 ||
        chain >= ((int64_t)1 << 60))
        return ek_set_error(EK_EARG, "%s: bad argument (1 <= n <= 2^36, 0 <= chain < 2^60)", who);
    for (int64_t k = 0; k < n; ++k)
        if (states[k] < 0 || states[k] >= n_states)
            return ek_set_error(EK_EARG, "%s: state %d of photon %lld is no state of %d", who,
                                states[k], (long long)k, n_states);
    *bad_state_out = -1;
    if ((rc = kmc_set_device(device)) != EK_OK ||
        (rc = ek_mi_check_memory((size_t)n * 5 + plan.bytes(n) + 1024, who)) != EK_OK)
        return rc;
    KmcScope sc;
    int32_t *d_s = nullptr;
    uint8_t *d_flags = nullptr;
    uint32_t *d_bad = nullptr, bad = KMC_NO_BAD;
    KMC_HIP(ek_stream_create_flags(&sc.own, hipStreamNonBlocking));
    hipStream_t s = sc.own;
    KMC_HIP(sc.events());
    KMC_HIP(sc.alloc(&d_flags, (size_t)n));
    KMC_HIP(sc.alloc(&d_bad, sizeof(uint32_t)));
    KMC_HIP(hipEventRecord(sc.ev[0], s));
    if ((rc = plan.upload(sc, s, n)) != EK_OK)
        return rc;
    KMC_HIP(sc.upload(&d_s, states, (size_t)n, s));
    KMC_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(uint32_t), s));
    KMC_HIP(hipEventRecord(sc.ev[1], s));
    auto rule = plan.rule(seed, d_flags, d_bad);
    hipLaunchKernelGGL(db_photons_kernel<decltype(rule)>, dim3(kmc_blocks(n, KMC_WG)),
                       dim3(KMC_WG), 0, s, rule, (uint64_t)chain, n, d_s, n_states);
    KMC_HIP(hipGetLastError());
    KMC_HIP(hipEventRecord(sc.ev[2], s));
    KMC_HIP(hipMemcpyAsync(flags_out, d_flags, (size_t)n, hipMemcpyDeviceToHost, s));
    if ((rc = plan.download(s, n)) != EK_OK)
        return rc;
    KMC_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    KMC_HIP(hipEventRecord(sc.ev[3], s));
    KMC_HIP(hipStreamSynchronize(s));
    *bad_state_out = kmc_bad(bad);
    return kmc_store_ms(sc, db_ms);
}

extern "C" int ek_dye_photons_lifetimes(int device, uint64_t seed, int64_t chain, int64_t n,
                                        const int32_t *states, int32_t n_states,
                                        const int64_t *ev_off, const double *ev_life,
                                        const uint8_t *ev_flag, uint8_t *flags_out,
                                        double *life_out, int64_t *bad_state_out)
{
    const char *who = "ek_dye_photons_lifetimes";
    int rc = EK_OK;
    if (!life_out)
        return ek_set_error(EK_EARG, "%s: null argument", who);
    if ((rc = db_check_off(n_states, ev_off, "photon events", who)) != EK_OK)
        return rc;
    if (ev_off[n_states] > 0 && (!ev_life || !ev_flag))
        return ek_set_error(EK_EARG, "%s: null argument", who);
    DbLifePlan plan{n_states, ev_off, ev_life, ev_flag, life_out, nullptr};
    return db_run_photons(device, who, seed, chain, n, states, n_states, flags_out, bad_state_out,
                          plan);
}

extern "C" int ek_dye_photons_k2(int device, uint64_t seed, int64_t chain, int64_t n,
                                 const int32_t *states, int32_t n_states, const int64_t *d_off,
                                 const double *d_xyz, const int64_t *a_off, const double *a_xyz,
                                 double c6, uint8_t *flags_out, double *k2_out, double *r_out,
                                 int32_t *drow_out, int32_t *arow_out, int64_t *bad_state_out)
{
    const char *who = "ek_dye_photons_k2";
    int rc = EK_OK;
    if (!k2_out || !r_out)
        return ek_set_error(EK_EARG, "%s: null argument", who);
    if ((rc = db_check_k2(n_states, d_off, d_xyz, a_off, a_xyz, drow_out, arow_out, who)) != EK_OK)
        return rc;
    DbK2Plan plan{n_states, d_off, a_off, d_xyz, a_xyz, c6, k2_out, r_out, nullptr, drow_out,
                  arow_out};
    return db_run_photons(device, who, seed, chain, n, states, n_states, flags_out, bad_state_out,
                          plan);
}

extern "C" int ek_dye_pick_events(int device, int64_t n, const int32_t *states, const double *u,
                                  int32_t n_states, const int64_t *ev_off, int64_t *index_out,
                                  int64_t *bad_state_out)
{
    const char *who = "ek_dye_pick_events";
    int rc = EK_OK;
    if (n < 1 || n > ((int64_t)1 << 36) || !states || !u || !index_out || !bad_state_out)
        return ek_set_error(EK_EARG, "%s: bad argument (1 <= n <= 2^36)", who);
    if ((rc = db_check_off(n_states, ev_off, "photon events", who)) != EK_OK)
        return rc;
    for (int64_t k = 0; k < n; ++k)
        if (states[k] < 0 || states[k] >= n_states || !(u[k] >= 0.0 && u[k] < 1.0))
            return ek_set_error(EK_EARG, "%s: entry %lld: state %d is no state of %d, or its "
                                         "double is outside [0, 1)", who, (long long)k, states[k],
                                n_states);
    *bad_state_out = -1;
    if ((rc = kmc_set_device(device)) != EK_OK ||
        (rc = ek_mi_check_memory((size_t)n * 20 + (size_t)n_states * 8 + 1024, who)) != EK_OK)
        return rc;
    KmcScope sc;
    int32_t *d_s = nullptr;
    double *d_u = nullptr;
    int64_t *d_off = nullptr, *d_idx = nullptr;
    uint32_t *d_bad = nullptr, bad = KMC_NO_BAD;
    KMC_HIP(ek_stream_create_flags(&sc.own, hipStreamNonBlocking));
    hipStream_t s = sc.own;
    KMC_HIP(sc.events());
    KMC_HIP(sc.alloc(&d_idx, (size_t)n * sizeof(int64_t)));
    KMC_HIP(sc.alloc(&d_bad, sizeof(uint32_t)));
    KMC_HIP(hipEventRecord(sc.ev[0], s));
    KMC_HIP(sc.upload(&d_s, states, (size_t)n, s));
    KMC_HIP(sc.upload(&d_u, u, (size_t)n, s));
    KMC_HIP(sc.upload(&d_off, ev_off, (size_t)n_states + 1, s));
    KMC_HIP(hipMemsetAsync(d_bad, 0xff, sizeof(uint32_t), s));
    KMC_HIP(hipEventRecord(sc.ev[1], s));
    hipLaunchKernelGGL(db_pick_kernel, dim3(kmc_blocks(n, KMC_WG)), dim3(KMC_WG), 0, s, n, d_s,
                       d_u, n_states, d_off, d_idx, d_bad);
    KMC_HIP(hipGetLastError());
    KMC_HIP(hipEventRecord(sc.ev[2], s));
    KMC_HIP(hipMemcpyAsync(index_out, d_idx, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost,
                           s));
    KMC_HIP(hipMemcpyAsync(&bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    KMC_HIP(hipEventRecord(sc.ev[3], s));
    KMC_HIP(hipStreamSynchronize(s));
    *bad_state_out = kmc_bad(bad);
    return kmc_store_ms(sc, db_ms);
}

extern "C" int ek_dye_bursts_last_timing(double *ms_out)
{
    if (!ms_out)
        return ek_set_error(EK_EARG, "ek_dye_bursts_last_timing: null argument");
    for (int i = 0; i < 3; ++i)
        ms_out[i] = db_ms[i];
    return EK_OK;
}
