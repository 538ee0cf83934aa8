// ek_dye_map.hip -- a library of dye conformations superposed on a labelled residue of
// every protein centre, the conformations that clash with the protein counted out, and
// the emission centre and transition dipole of every conformation, on the device.
//
// Replaces map_dye_on_protein of the reference's enspara/geometry/explicit_r0_calc.py and
// what it calls (:122-166 remove_touches_protein_dye_traj, :169-220 assemble_dye_r_mu,
// :294-345 align_full_dye_to_res, :347-455).  The contract is DESIGN.md 4q;
// include/enspara_hip.h has the full text.
//
//   fit      per (centre p, conformation d): ek_rmsf.hip's steps 1-2 with the sums taken
//            sequentially in selection order.  What depends on d alone (centroid, centred
//            float32 coordinates, Gx) and on p alone (c_ref, centred float32 coordinates,
//            Gy) is made on the host, once per handle and once per run; the kernel forms
//            S, lambda (ek_msd_lambda_from_S) and R (ek_superpose_from_S), one LANE per
//            (p, d): 64 independent serial chains a wave.  -> R [p][9][d], flags [p][d]
//   cull     one workgroup per centre: the atoms that are not excluded and lie within
//            reach + cutoff_a + margin_p of c_ref, compacted in their order as (x, y, z,
//            threshold) doubles.  An atom outside can touch no dye atom (4q, "Margin").
//   touch    one lane per (p, d, dye atom), 256 consecutive (d, atom) pairs a workgroup:
//            the lane places its atom (step 3 of ek_rmsf.hip, the same expressions), the
//            centre's culled atoms pass through the LDS in batches of DM_STAGE; a lane
//            stops at its first touching atom, a workgroup once none of its lanes is left.
//            Lanes that stay to the end add 1 to their conformation's counter in the LDS
//            (ds_add_u32), the counters then go to counts [p][d] with integer atomics (a
//            conformation may span two workgroups).  The lane of r_atom writes the emission
//            centre, the lane of mu_atoms[0] places mu_atoms[1] again (the same bits) and
//            writes the dipole's origin and the float32 difference.
// Counts are integers: the order of the additions is free, every run gives the same bits.
#include "ek_common.h"
#include "ek_qcp.h"
#include "ek_superpose.h"
#include "ek_sq_threshold.h"

#include <math.h>
#include <new>
#include <vector>

extern int ek_set_error(int code, const char *fmt, ...);
int ek_mi_check_memory(size_t bytes, const char *who);

#define DM_HIP(call)                                                           \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define DM_WG 256
#define DM_STAGE 1024                       // atoms of one batch: 32 KiB of LDS
#define DM_MAX_SEL 16                       // atoms of a selection
#define DM_MAX_CENTRES 32768                // of one run: grid.y
#define DM_MAX_COORD 1048576.0              // nm
#define DM_CEN 8                            // doubles per centre: c_ref [3], Gy, reach + margin
#define DM_GRID_SLACK (1.0 + 0x1p-40)       // the cull's own float64 roundings

struct ek_dye_map {
    int device;
    int32_t atoms, D, A, n_sel, r_atom, mu0, mu1;
    bool fit;                   // false: coordinates as they are
    double reach;               // the largest distance of a dye atom from its cull centre
    double cc[3];               // !fit: the cull centre (the mean of all dye atoms)
    std::vector<int32_t> psel;  // [n_sel]
    double *thr, *cut;          // [atoms] squared threshold; radius + probe
    uint8_t *excl;              // [atoms]
    float *dye;                 // [D][A][3]
    float *xc;                  // [D][n_sel][3] the selection centred, float32
    double *cx, *Gx;            // [D][3], [D]
    // a run's buffers, kept between runs while they fit
    int64_t cap;
    bool cap_aligned;
    float *xyz, *yc, *aligned;  // [cap][atoms][3], [cap][n_sel][3], [cap][D][A][3]
    double *cen, *R, *coords;   // [cap][DM_CEN], [cap][9][D], [cap][D][9]
    double4 *list;              // [cap][atoms]
    int32_t *nlist, *counts;    // [cap], [cap][D]
    uint8_t *flags;             // [cap][D]
    int64_t n_last;             // centres of the last run
    bool last_aligned;
    std::vector<int32_t> list_len;
    hipStream_t s;
    hipEvent_t ev[7];
    double ms[5];               // upload, fit, cull, touch; the last fetch's download
};

// ---- device ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(DM_WG)
dm_fit_kernel(const float *__restrict__ xc, const double *__restrict__ Gx, int32_t D,
              int32_t n_sel, const float *__restrict__ yc, const double *__restrict__ cen,
              double *__restrict__ R, uint8_t *__restrict__ flags)
{
    __shared__ float ys[3 * DM_MAX_SEL];
    const int p = (int)blockIdx.y;
    if ((int)threadIdx.x < 3 * n_sel)
        ys[threadIdx.x] = yc[(size_t)p * 3 * n_sel + threadIdx.x];
    __syncthreads();
    const int32_t d = (int32_t)blockIdx.x * DM_WG + (int32_t)threadIdx.x;
    if (d >= D)
        return;
    double v[9];
#pragma unroll
    for (int j = 0; j < 9; ++j)
        v[j] = 0.0;
    const float *x = xc + (size_t)d * n_sel * 3;
    for (int k = 0; k < n_sel; ++k) {
        const double x0 = (double)x[3 * k], x1 = (double)x[3 * k + 1], x2 = (double)x[3 * k + 2];
        const double y0 = (double)ys[3 * k], y1 = (double)ys[3 * k + 1], y2 = (double)ys[3 * k + 2];
        v[0] = v[0] + x0 * y0;
        v[1] = v[1] + x0 * y1;
        v[2] = v[2] + x0 * y2;
        v[3] = v[3] + x1 * y0;
        v[4] = v[4] + x1 * y1;
        v[5] = v[5] + x1 * y2;
        v[6] = v[6] + x2 * y0;
        v[7] = v[7] + x2 * y1;
        v[8] = v[8] + x2 * y2;
    }
    float S[9];
#pragma unroll
    for (int j = 0; j < 9; ++j)
        S[j] = (float)v[j];
    const double gx = Gx[d], gy = cen[(size_t)p * DM_CEN + 3];
    double lam, Rm[9];
    (void)ek_msd_lambda_from_S(S, gx, gy, n_sel, &lam);
    const int bad = ek_superpose_from_S(S, gx, gy, lam, Rm);
    double *out = R + (size_t)p * 9 * D + d;
#pragma unroll
    for (int j = 0; j < 9; ++j)
        out[(size_t)j * D] = Rm[j];
    flags[(size_t)p * D + d] = (uint8_t)bad;
}

__global__ void __launch_bounds__(DM_WG)
dm_cull_kernel(const float *__restrict__ xyz, int32_t atoms, const double *__restrict__ cut,
               const double *__restrict__ thr, const uint8_t *__restrict__ excl,
               const double *__restrict__ cen, double4 *__restrict__ list,
               int32_t *__restrict__ nlist)
{
    __shared__ int wsum[DM_WG / EK_WAVE];
    const int tid = threadIdx.x, lane = tid & (EK_WAVE - 1), wave = tid / EK_WAVE;
    const int p = (int)blockIdx.x;
    const float *X = xyz + (size_t)p * atoms * 3;
    const double *c = cen + (size_t)p * DM_CEN;
    const double c0 = c[0], c1 = c[1], c2 = c[2], rpm = c[4];
    double4 *out = list + (size_t)p * atoms;
    int32_t base = 0;
    for (int32_t i0 = 0; i0 < atoms; i0 += DM_WG) {
        const int32_t i = i0 + tid;
        bool k = false;
        double x = 0.0, y = 0.0, z = 0.0;
        if (i < atoms && excl[i] == 0) {
            x = (double)X[3 * (size_t)i];
            y = (double)X[3 * (size_t)i + 1];
            z = (double)X[3 * (size_t)i + 2];
            const double dx = x - c0, dy = y - c1, dz = z - c2;
            const double t = (rpm + cut[i]) * DM_GRID_SLACK;
            k = !((dx * dx + dy * dy) + dz * dz > t * t);
        }
        const unsigned long long m = __ballot(k);
        if (lane == 0)
            wsum[wave] = __popcll(m);
        __syncthreads();
        int32_t off = base, tot = 0;
        for (int w = 0; w < DM_WG / EK_WAVE; ++w) {
            if (w < wave)
                off += wsum[w];
            tot += wsum[w];
        }
        if (k)          // (off + rank < base + tot <= atoms)
            out[off + __popcll(m & (((unsigned long long)1 << lane) - 1))] =
                make_double4(x, y, z, thr[i]);
        base += tot;
        __syncthreads();
    }
    if (tid == 0)
        nlist[p] = base;
}

struct DmTouch {
    const float *dye;           // [D][A][3]
    const double *cx;           // [D][3]
    const double *R;            // [P][9][D] or null: coordinates as they are
    const double *cen;          // [P][DM_CEN]
    const double4 *list;        // [P][atoms]
    const int32_t *nlist;       // [P]
    int32_t atoms, D, A, r_atom, mu0, mu1;
    int32_t *counts;            // [P][D], cleared
    double *coords;             // [P][D][9]
    float *aligned;             // [P][D][A][3] or null
};

// atom i of conformation d on centre p: step 3 of ek_rmsf.hip
__device__ __forceinline__ void dm_place(const DmTouch &a, int p, int32_t d, int32_t i, float &ox,
                                         float &oy, float &oz)
{
    const float *q = a.dye + ((size_t)d * a.A + i) * 3;
    if (!a.R) {
        ox = q[0];
        oy = q[1];
        oz = q[2];
        return;
    }
    const double *c = a.cx + 3 * (size_t)d;
    const double *cr = a.cen + (size_t)p * DM_CEN;
    const double *R = a.R + (size_t)p * 9 * a.D + d;
    const size_t D = (size_t)a.D;
    const double x = (double)q[0] - c[0], y = (double)q[1] - c[1], z = (double)q[2] - c[2];
    ox = (float)(__builtin_fma(R[2 * D], z, __builtin_fma(R[D], y, R[0] * x)) + cr[0]);
    oy = (float)(__builtin_fma(R[5 * D], z, __builtin_fma(R[4 * D], y, R[3 * D] * x)) + cr[1]);
    oz = (float)(__builtin_fma(R[8 * D], z, __builtin_fma(R[7 * D], y, R[6 * D] * x)) + cr[2]);
}

__global__ void __launch_bounds__(DM_WG) dm_touch_kernel(const DmTouch a)
{
    __shared__ double4 at[DM_STAGE];
    __shared__ unsigned int cnt[DM_WG];
    const int tid = threadIdx.x;
    const int p = (int)blockIdx.y;
    const int64_t total = (int64_t)a.D * a.A;
    const int64_t j0 = (int64_t)blockIdx.x * DM_WG;     // (< total: the grid is cut to it)
    const bool valid = j0 + tid < total;
    const int64_t j = valid ? j0 + tid : j0;
    const int32_t d = (int32_t)(j / a.A), i = (int32_t)(j - (int64_t)d * a.A);
    const int32_t d_first = (int32_t)(j0 / a.A);
    const int64_t j_last = (j0 + DM_WG < total) ? j0 + DM_WG - 1 : total - 1;
    const int32_t nd = (int32_t)(j_last / a.A) - d_first + 1;   // (<= DM_WG: A >= 1)
    cnt[tid] = 0u;
    float fx, fy, fz;
    dm_place(a, p, d, i, fx, fy, fz);
    if (valid) {
        const size_t pd = (size_t)p * a.D + d;
        if (a.aligned) {
            float *o = a.aligned + (pd * a.A + i) * 3;
            o[0] = fx;
            o[1] = fy;
            o[2] = fz;
        }
        double *o9 = a.coords + pd * 9;
        if (i == a.r_atom) {
            o9[0] = (double)fx;
            o9[1] = (double)fy;
            o9[2] = (double)fz;
        }
        if (i == a.mu0) {
            float gx, gy, gz;
            dm_place(a, p, d, a.mu1, gx, gy, gz);
            o9[3] = (double)fx;
            o9[4] = (double)fy;
            o9[5] = (double)fz;
            o9[6] = (double)(fx - gx);
            o9[7] = (double)(fy - gy);
            o9[8] = (double)(fz - gz);
        }
    }
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    const int32_t L = a.nlist[p];
    const double4 *list = a.list + (size_t)p * a.atoms;
    bool alive = valid;
    __syncthreads();            // the counters are cleared
    for (int32_t base = 0; base < L; base += DM_STAGE) {
        const int32_t n = (L - base < DM_STAGE) ? L - base : DM_STAGE;
        for (int32_t k = tid; k < n; k += DM_WG)
            at[k] = list[base + k];
        __syncthreads();
        if (alive)
            for (int32_t k = 0; k < n; ++k) {
                const double4 e = at[k];
                const double dx = e.x - px, dy = e.y - py, dz = e.z - pz;
                if (!((dx * dx + dy * dy) + dz * dz >= e.w)) {
                    alive = false;
                    break;
                }
            }
        // (also the barrier before the next batch overwrites the list)
        if (!__syncthreads_or(alive ? 1 : 0))
            break;
    }
    if (alive)
        atomicAdd(&cnt[d - d_first], 1u);
    __syncthreads();
    if (tid < nd && cnt[tid])
        atomicAdd(&a.counts[(size_t)p * a.D + d_first + tid], (int32_t)cnt[tid]);
}

// ---- host ------------------------------------------------------------------------------------
static int dm_check_coords(const float *x, size_t n, const char *who, const char *what)
{
    for (size_t q = 0; q < n; ++q)
        if (!(fabs((double)x[q]) <= DM_MAX_COORD))
            return ek_set_error(EK_EARG, "%s: %s %zu is not finite or beyond 2^20 nm", who, what, q);
    return EK_OK;
}

static int dm_bind(ek_dye_map *h, const char *who)
{
    if (!h)
        return ek_set_error(EK_EARG, "%s: null handle", who);
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", h->device, hipGetErrorString(e));
    return EK_OK;
}

static void dm_free_run(ek_dye_map *h)
{
    (void)ek_dev_free(h->xyz);
    (void)ek_dev_free(h->yc);
    (void)ek_dev_free(h->aligned);
    (void)ek_dev_free(h->cen);
    (void)ek_dev_free(h->R);
    (void)ek_dev_free(h->coords);
    (void)ek_dev_free(h->list);
    (void)ek_dev_free(h->nlist);
    (void)ek_dev_free(h->counts);
    (void)ek_dev_free(h->flags);
    h->xyz = h->yc = h->aligned = nullptr;
    h->cen = h->R = h->coords = nullptr;
    h->list = nullptr;
    h->nlist = h->counts = nullptr;
    h->flags = nullptr;
    h->cap = 0;
    h->cap_aligned = false;
}

extern "C" int ek_dye_map_close(ek_dye_map *h)
{
    if (!h)
        return EK_OK;
    (void)hipSetDevice(h->device);
    if (h->s)
        (void)hipStreamSynchronize(h->s);
    dm_free_run(h);
    (void)ek_dev_free(h->thr);
    (void)ek_dev_free(h->cut);
    (void)ek_dev_free(h->excl);
    (void)ek_dev_free(h->dye);
    (void)ek_dev_free(h->xc);
    (void)ek_dev_free(h->cx);
    (void)ek_dev_free(h->Gx);
    for (hipEvent_t e : h->ev)
        if (e)
            (void)ek_event_destroy(e);
    if (h->s)
        (void)ek_stream_destroy(h->s);
    delete h;
    return EK_OK;
}

extern "C" int ek_dye_map_open(int device, int32_t atoms, const double *cutoff, int32_t n_excl,
                               const int32_t *excl, int32_t D, int32_t A, const float *dye_xyz,
                               int32_t n_sel, const int32_t *prot_sel, const int32_t *dye_sel,
                               int32_t r_atom, int32_t mu0, int32_t mu1, ek_dye_map **out)
{
    int rc = EK_OK;
    if (!out)
        return ek_set_error(EK_EARG, "ek_dye_map_open: null output");
    *out = nullptr;
    const bool fit = prot_sel != nullptr;
    if (!cutoff || !dye_xyz || atoms < 1 || D < 1 || A < 1 || n_excl < 0 || (n_excl > 0 && !excl) ||
        (int64_t)D * A > INT32_MAX - DM_WG || r_atom < 0 || r_atom >= A || mu0 < 0 || mu0 >= A ||
        mu1 < 0 || mu1 >= A)
        return ek_set_error(EK_EARG, "ek_dye_map_open: bad argument (atoms, D, A >= 1, D * A < 2^31, "
                                     "r_atom and mu_atoms in [0, A))");
    if (fit) {
        if (!dye_sel || n_sel < 3 || n_sel > DM_MAX_SEL)
            return ek_set_error(EK_EARG, "ek_dye_map_open: a selection has 3 to %d atoms",
                                DM_MAX_SEL);
        for (int32_t k = 0; k < n_sel; ++k)
            if (prot_sel[k] < 0 || prot_sel[k] >= atoms || dye_sel[k] < 0 || dye_sel[k] >= A)
                return ek_set_error(EK_EARG, "ek_dye_map_open: selected atom %d is out of range", k);
    } else {
        n_sel = 0;
    }
    for (int32_t k = 0; k < n_excl; ++k)
        if (excl[k] < 0 || excl[k] >= atoms)
            return ek_set_error(EK_EARG, "ek_dye_map_open: excluded atom %d is not in [0, %d)",
                                excl[k], atoms);
    if ((rc = dm_check_coords(dye_xyz, (size_t)D * A * 3, "ek_dye_map_open", "dye coordinate")) !=
        EK_OK)
        return rc;
    std::vector<double> thr, cx, Gx;
    std::vector<uint8_t> ex;
    std::vector<float> xc;
    ek_dye_map *h = nullptr;
    try {
        thr.resize(atoms);
        ex.assign(atoms, 0);
        cx.assign((size_t)D * 3, 0.0);
        Gx.assign(D, 0.0);
        xc.assign((size_t)D * (n_sel > 0 ? n_sel : 1) * 3, 0.0f);
        h = new ek_dye_map();
        if (fit)
            h->psel.assign(prot_sel, prot_sel + n_sel);
    } catch (const std::bad_alloc &) {
        delete h;
        return ek_set_error(EK_ENOMEM, "ek_dye_map_open: out of host memory");
    }
    for (int32_t i = 0; i < atoms; ++i) {
        if (!(cutoff[i] > 0.0 && cutoff[i] <= DM_MAX_COORD)) {
            delete h;
            return ek_set_error(EK_EARG, "ek_dye_map_open: radius + probe of atom %d is not in "
                                         "(0, 2^20] nm", i);
        }
        // free iff sqrt(s) > cutoff iff sqrt(s) >= the next double iff s >= this
        thr[i] = dy_sq_at_least(nextafter(cutoff[i], INFINITY));
    }
    for (int32_t k = 0; k < n_excl; ++k)
        ex[excl[k]] = 1;
    h->device = device;
    h->atoms = atoms;
    h->D = D;
    h->A = A;
    h->n_sel = n_sel;
    h->r_atom = r_atom;
    h->mu0 = mu0;
    h->mu1 = mu1;
    h->fit = fit;
    h->reach = 0.0;
    if (fit) {
        // per conformation: the centroid of the selection as a float64 sum in selection order,
        // the centred coordinates rounded to float32, Gx the float64 sum of their exact squares
        for (int32_t d = 0; d < D; ++d) {
            const float *q = dye_xyz + (size_t)d * A * 3;
            double c[3] = {0.0, 0.0, 0.0};
            for (int32_t k = 0; k < n_sel; ++k)
                for (int t = 0; t < 3; ++t)
                    c[t] = c[t] + (double)q[3 * (size_t)dye_sel[k] + t];
            for (int t = 0; t < 3; ++t)
                cx[3 * (size_t)d + t] = c[t] = c[t] / (double)n_sel;
            double G = 0.0;
            for (int32_t k = 0; k < n_sel; ++k) {
                double x[3];
                for (int t = 0; t < 3; ++t) {
                    const float f = (float)((double)q[3 * (size_t)dye_sel[k] + t] - c[t]);
                    xc[((size_t)d * n_sel + k) * 3 + t] = f;
                    x[t] = (double)f;
                }
                G = G + ((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
            }
            Gx[d] = G;
            for (int32_t i = 0; i < A; ++i) {
                const double x = (double)q[3 * (size_t)i] - c[0], y = (double)q[3 * (size_t)i + 1] - c[1],
                             z = (double)q[3 * (size_t)i + 2] - c[2];
                const double r = sqrt((x * x + y * y) + z * z);
                h->reach = r > h->reach ? r : h->reach;
            }
        }
    } else {
        const size_t n = (size_t)D * A;
        double c[3] = {0.0, 0.0, 0.0};
        for (size_t q = 0; q < n; ++q)
            for (int t = 0; t < 3; ++t)
                c[t] += (double)dye_xyz[3 * q + t];
        for (int t = 0; t < 3; ++t)
            h->cc[t] = c[t] / (double)n;
        for (size_t q = 0; q < n; ++q) {
            const double x = (double)dye_xyz[3 * q] - h->cc[0], y = (double)dye_xyz[3 * q + 1] - h->cc[1],
                         z = (double)dye_xyz[3 * q + 2] - h->cc[2];
            const double r = sqrt((x * x + y * y) + z * z);
            h->reach = r > h->reach ? r : h->reach;
        }
    }
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess) {
            delete h;
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e0));
        }
    }
    DM_HIP(ek_stream_create_flags(&h->s, hipStreamNonBlocking));
    for (hipEvent_t &e : h->ev)
        DM_HIP(ek_event_create(&e));
    DM_HIP(ek_dev_malloc(&h->thr, (size_t)atoms * sizeof(double)));
    DM_HIP(ek_dev_malloc(&h->cut, (size_t)atoms * sizeof(double)));
    DM_HIP(ek_dev_malloc(&h->excl, (size_t)atoms));
    DM_HIP(ek_dev_malloc(&h->dye, (size_t)D * A * 3 * sizeof(float)));
    DM_HIP(ek_dev_malloc(&h->xc, xc.size() * sizeof(float)));
    DM_HIP(ek_dev_malloc(&h->cx, cx.size() * sizeof(double)));
    DM_HIP(ek_dev_malloc(&h->Gx, Gx.size() * sizeof(double)));
    DM_HIP(hipMemcpyAsync(h->thr, thr.data(), (size_t)atoms * sizeof(double), hipMemcpyHostToDevice,
                          h->s));
    DM_HIP(hipMemcpyAsync(h->cut, cutoff, (size_t)atoms * sizeof(double), hipMemcpyHostToDevice,
                          h->s));
    DM_HIP(hipMemcpyAsync(h->excl, ex.data(), (size_t)atoms, hipMemcpyHostToDevice, h->s));
    DM_HIP(hipMemcpyAsync(h->dye, dye_xyz, (size_t)D * A * 3 * sizeof(float), hipMemcpyHostToDevice,
                          h->s));
    DM_HIP(hipMemcpyAsync(h->xc, xc.data(), xc.size() * sizeof(float), hipMemcpyHostToDevice, h->s));
    DM_HIP(hipMemcpyAsync(h->cx, cx.data(), cx.size() * sizeof(double), hipMemcpyHostToDevice, h->s));
    DM_HIP(hipMemcpyAsync(h->Gx, Gx.data(), Gx.size() * sizeof(double), hipMemcpyHostToDevice, h->s));
    DM_HIP(hipStreamSynchronize(h->s));     // (the vectors go with this frame)
    *out = h;
    return EK_OK;
done:
    ek_dye_map_close(h);
    return rc;
}

// device bytes of one centre of a run
static size_t dm_per_centre(const ek_dye_map *h, bool aligned)
{
    const size_t D = (size_t)h->D;
    return (size_t)h->atoms * (3 * sizeof(float) + sizeof(double4)) +
           (size_t)(h->n_sel > 0 ? h->n_sel : 1) * 3 * sizeof(float) + DM_CEN * sizeof(double) +
           D * (9 * sizeof(double) * 2 + sizeof(int32_t) + 1) + sizeof(int32_t) +
           (aligned ? D * h->A * 3 * sizeof(float) : 0);
}

extern "C" int ek_dye_map_max_centres(ek_dye_map *h, int32_t want_aligned, int64_t *out)
{
    int rc = dm_bind(h, "ek_dye_map_max_centres");
    if (rc != EK_OK)
        return rc;
    if (!out)
        return ek_set_error(EK_EARG, "ek_dye_map_max_centres: null output");
    size_t free_b = 0, total_b = 0;
    hipError_t e = hipMemGetInfo(&free_b, &total_b);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "ek_dye_map_max_centres: hipMemGetInfo: %s",
                            hipGetErrorString(e));
    // (a handle's own run buffers count as free: the next run replaces them)
    free_b += (size_t)h->cap * dm_per_centre(h, h->cap_aligned);
    int64_t n = (int64_t)(free_b / 2 / dm_per_centre(h, want_aligned != 0));
    if (n < 1)
        return ek_set_error(EK_ENOMEM, "ek_dye_map_max_centres: one centre of %d atoms and %d x %d "
                                       "dye atoms does not fit %zu MiB of free device memory",
                            h->atoms, h->D, h->A, free_b >> 20);
    *out = n > DM_MAX_CENTRES ? DM_MAX_CENTRES : n;
    return EK_OK;
}

extern "C" int ek_dye_map_run(ek_dye_map *h, const float *xyz, int64_t centres,
                              int32_t want_aligned)
{
    int rc = dm_bind(h, "ek_dye_map_run");
    if (rc != EK_OK)
        return rc;
    if (!xyz || centres < 1 || centres > DM_MAX_CENTRES)
        return ek_set_error(EK_EARG, "ek_dye_map_run: bad argument (1 <= centres <= %d)",
                            DM_MAX_CENTRES);
    const int32_t atoms = h->atoms, D = h->D, A = h->A, ns = h->n_sel;
    const bool al = want_aligned != 0;
    h->n_last = 0;
    h->ms[0] = h->ms[1] = h->ms[2] = h->ms[3] = h->ms[4] = 0.0;
    // (xyz finite and within 2^20 nm is the caller's to check, as for ek_rmsf_run: no index
    // below depends on a coordinate)
    // per centre, on the host: c_ref as a float64 sum in selection order, the centred
    // coordinates rounded to float32, Gy; reach + margin ("Margin")
    std::vector<double> cen;
    std::vector<float> yc;
    try {
        cen.assign((size_t)centres * DM_CEN, 0.0);
        yc.assign((size_t)centres * (ns > 0 ? ns : 1) * 3, 0.0f);
        h->list_len.assign((size_t)centres, 0);
    } catch (const std::bad_alloc &) {
        return ek_set_error(EK_ENOMEM, "ek_dye_map_run: out of host memory");
    }
    for (int64_t p = 0; p < centres; ++p) {
        double *c = cen.data() + (size_t)p * DM_CEN;
        if (!h->fit) {
            for (int t = 0; t < 3; ++t)
                c[t] = h->cc[t];
            c[4] = h->reach;
            continue;
        }
        const float *X = xyz + (size_t)p * atoms * 3;
        double s[3] = {0.0, 0.0, 0.0};
        for (int32_t k = 0; k < ns; ++k)
            for (int t = 0; t < 3; ++t)
                s[t] = s[t] + (double)X[3 * (size_t)h->psel[k] + t];
        double G = 0.0, cmax = 0.0;
        for (int t = 0; t < 3; ++t) {
            c[t] = s[t] / (double)ns;
            cmax = fabs(c[t]) > cmax ? fabs(c[t]) : cmax;
        }
        for (int32_t k = 0; k < ns; ++k) {
            double y[3];
            for (int t = 0; t < 3; ++t) {
                const float f = (float)((double)X[3 * (size_t)h->psel[k] + t] - c[t]);
                yc[((size_t)p * ns + k) * 3 + t] = f;
                y[t] = (double)f;
            }
            G = G + ((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]);
        }
        c[3] = G;
        c[4] = h->reach + ((cmax + h->reach) * 0x1p-22 + h->reach * 0x1p-40);
    }
    if (centres > h->cap || (al && !h->cap_aligned)) {
        dm_free_run(h);
        if ((rc = ek_mi_check_memory((size_t)centres * dm_per_centre(h, al), "ek_dye_map_run")) !=
            EK_OK)
            return rc;
        DM_HIP(ek_dev_malloc(&h->xyz, (size_t)centres * atoms * 3 * sizeof(float)));
        DM_HIP(ek_dev_malloc(&h->yc, yc.size() * sizeof(float)));
        DM_HIP(ek_dev_malloc(&h->cen, cen.size() * sizeof(double)));
        DM_HIP(ek_dev_malloc(&h->R, (size_t)centres * 9 * D * sizeof(double)));
        DM_HIP(ek_dev_malloc(&h->coords, (size_t)centres * D * 9 * sizeof(double)));
        DM_HIP(ek_dev_malloc(&h->list, (size_t)centres * atoms * sizeof(double4)));
        DM_HIP(ek_dev_malloc(&h->nlist, (size_t)centres * sizeof(int32_t)));
        DM_HIP(ek_dev_malloc(&h->counts, (size_t)centres * D * sizeof(int32_t)));
        DM_HIP(ek_dev_malloc(&h->flags, (size_t)centres * D));
        if (al)
            DM_HIP(ek_dev_malloc(&h->aligned, (size_t)centres * D * A * 3 * sizeof(float)));
        h->cap = centres;
        h->cap_aligned = al;
    }
    {
        DmTouch a;
        a.dye = h->dye;
        a.cx = h->cx;
        a.R = h->fit ? h->R : nullptr;
        a.cen = h->cen;
        a.list = h->list;
        a.nlist = h->nlist;
        a.atoms = atoms;
        a.D = D;
        a.A = A;
        a.r_atom = h->r_atom;
        a.mu0 = h->mu0;
        a.mu1 = h->mu1;
        a.counts = h->counts;
        a.coords = h->coords;
        a.aligned = al ? h->aligned : nullptr;
        DM_HIP(hipEventRecord(h->ev[0], h->s));
        DM_HIP(hipMemcpyAsync(h->xyz, xyz, (size_t)centres * atoms * 3 * sizeof(float),
                              hipMemcpyHostToDevice, h->s));
        DM_HIP(hipMemcpyAsync(h->cen, cen.data(), cen.size() * sizeof(double),
                              hipMemcpyHostToDevice, h->s));
        DM_HIP(hipMemcpyAsync(h->yc, yc.data(), yc.size() * sizeof(float), hipMemcpyHostToDevice,
                              h->s));
        DM_HIP(hipMemsetAsync(h->counts, 0, (size_t)centres * D * sizeof(int32_t), h->s));
        DM_HIP(hipMemsetAsync(h->flags, 0, (size_t)centres * D, h->s));
        DM_HIP(hipEventRecord(h->ev[1], h->s));
        if (h->fit)
            hipLaunchKernelGGL(dm_fit_kernel, dim3((unsigned)((D + DM_WG - 1) / DM_WG),
                                                   (unsigned)centres),
                               dim3(DM_WG), 0, h->s, h->xc, h->Gx, D, ns, h->yc, h->cen, h->R,
                               h->flags);
        DM_HIP(hipEventRecord(h->ev[2], h->s));
        hipLaunchKernelGGL(dm_cull_kernel, dim3((unsigned)centres), dim3(DM_WG), 0, h->s, h->xyz,
                           atoms, h->cut, h->thr, h->excl, h->cen, h->list, h->nlist);
        DM_HIP(hipEventRecord(h->ev[3], h->s));
        hipLaunchKernelGGL(dm_touch_kernel,
                           dim3((unsigned)(((int64_t)D * A + DM_WG - 1) / DM_WG), (unsigned)centres),
                           dim3(DM_WG), 0, h->s, a);
        DM_HIP(hipEventRecord(h->ev[4], h->s));
        DM_HIP(hipGetLastError());
        DM_HIP(hipMemcpyAsync(h->list_len.data(), h->nlist, (size_t)centres * sizeof(int32_t),
                              hipMemcpyDeviceToHost, h->s));
        DM_HIP(hipStreamSynchronize(h->s));
        for (int q = 0; q < 4; ++q) {
            float ms = 0.f;
            DM_HIP(hipEventElapsedTime(&ms, h->ev[q], h->ev[q + 1]));
            h->ms[q] = ms;
        }
    }
    h->n_last = centres;
    h->last_aligned = al;
done:
    (void)hipStreamSynchronize(h->s);
    return rc;
}

extern "C" int ek_dye_map_fetch(ek_dye_map *h, int64_t centres, int32_t *counts_out,
                                double *coords_out, uint8_t *flags_out, float *aligned_out)
{
    int rc = dm_bind(h, "ek_dye_map_fetch");
    if (rc != EK_OK)
        return rc;
    if (!counts_out || !coords_out || !flags_out)
        return ek_set_error(EK_EARG, "ek_dye_map_fetch: null argument");
    if (centres != h->n_last || centres < 1)
        return ek_set_error(EK_ESTATE, "ek_dye_map_fetch: the last run had %lld centres, not %lld",
                            (long long)h->n_last, (long long)centres);
    if (aligned_out && !h->last_aligned)
        return ek_set_error(EK_ESTATE, "ek_dye_map_fetch: the last run kept no aligned coordinates");
    const size_t n = (size_t)centres * h->D;
    float ms = 0.f;
    DM_HIP(hipEventRecord(h->ev[5], h->s));
    DM_HIP(hipMemcpyAsync(counts_out, h->counts, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->s));
    DM_HIP(hipMemcpyAsync(coords_out, h->coords, n * 9 * sizeof(double), hipMemcpyDeviceToHost,
                          h->s));
    DM_HIP(hipMemcpyAsync(flags_out, h->flags, n, hipMemcpyDeviceToHost, h->s));
    if (aligned_out)
        DM_HIP(hipMemcpyAsync(aligned_out, h->aligned, n * h->A * 3 * sizeof(float),
                              hipMemcpyDeviceToHost, h->s));
    DM_HIP(hipEventRecord(h->ev[6], h->s));
    DM_HIP(hipStreamSynchronize(h->s));
    DM_HIP(hipEventElapsedTime(&ms, h->ev[5], h->ev[6]));
    h->ms[4] = ms;
done:
    (void)hipStreamSynchronize(h->s);
    return rc;
}

extern "C" int ek_dye_map_stats(ek_dye_map *h, int64_t centres, int32_t *list_len_out,
                                double *reach_out)
{
    if (!h || !list_len_out)
        return ek_set_error(EK_EARG, "ek_dye_map_stats: null argument");
    if (centres != h->n_last)
        return ek_set_error(EK_ESTATE, "ek_dye_map_stats: the last run had %lld centres, not %lld",
                            (long long)h->n_last, (long long)centres);
    for (int64_t p = 0; p < centres; ++p)
        list_len_out[p] = h->list_len[(size_t)p];
    if (reach_out)
        *reach_out = h->reach;
    return EK_OK;
}

extern "C" int ek_dye_map_last_timing(ek_dye_map *h, double *ms_out)
{
    if (!h || !ms_out)
        return ek_set_error(EK_EARG, "ek_dye_map_last_timing: null argument");
    for (int i = 0; i < 5; ++i)
        ms_out[i] = h->ms[i];
    return EK_OK;
}
