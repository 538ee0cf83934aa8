// ek_tpt.hip -- transition path theory on the device: committors, mean first
// passage times and reactive fluxes of a dense transition matrix.
//
// Replaces the arithmetic of the reference's enspara/tpt/core.py (_I_m_Q :25-37,
// committors :40-102 with its spsolve, mfpts :105-155 with its inv / solve) and
// enspara/tpt/tpt.py (reactive_fluxes :48-91, net_fluxes :94-125).  Every entry
// point uploads T once, assembles its system on the device as the augmented
// matrix the solver of ek_lu.hip works on, solves, runs one fused epilogue and
// downloads the result and the solver's status word: one stream, no host round
// trip in between.
//   assemble   [I - Q | r] for a set of absorbing states, or [I - T + W | I]
//   solve      ek_lu_solve_dev
//   epilogue   q with q[sinks] = 1, q[sources] = 0;  lagtime * t;
//              lagtime * (Z_jj - Z_ij) / pi_j;  the fluxes (the net fluxes read the
//              transposed tile through the LDS)
// All of it float64, in the reference's order of operations where it has one:
// (I - T) + W, (T_ij * (pi_i * (1 - q_i))) * q_j, (lagtime * (Z_jj - Z_ij)) / pi_j.
#include "ek_lu.h"

#include <new>

extern int ek_set_error(int code, const char *fmt, ...);

#define TPT_HIP(call)                                                          \
    do {                                                                       \
        hipError_t e_ = (call);                                                \
        if (e_ != hipSuccess) {                                                \
            rc = ek_set_error(EK_EHIP, "%s failed: %s at %s:%d", #call,        \
                              hipGetErrorString(e_), __FILE__, __LINE__);      \
            goto done;                                                         \
        }                                                                      \
    } while (0)

#define TPT_WG 256
#define TPT_TILE 32

enum { TPT_COMMITTORS = 0, TPT_MFPT_SINKS = 1, TPT_MFPT_ALL = 2, TPT_GENERAL = 3 };
enum { TPT_FREE = 0, TPT_SOURCE = 1, TPT_SINK = 2 };

// ---- assembly ------------------------------------------------------------------------
// one thread per element of the padded augmented matrix; role[n]: TPT_FREE / SOURCE /
// SINK (both absorbing); sinks[n_sinks] in the caller's order (the order of r's sum)
__global__ void __launch_bounds__(TPT_WG)
tpt_assemble_kernel(int mode, int32_t n, int32_t npad, int32_t nrp,
                    const double *__restrict__ T, const int32_t *__restrict__ role,
                    const int32_t *__restrict__ sinks, int32_t n_sinks,
                    const double *__restrict__ pi, double *__restrict__ aug)
{
    const size_t ld = (size_t)npad + nrp;
    const int32_t j = blockIdx.x * TPT_WG + threadIdx.x;
    const int32_t i = blockIdx.y;
    if (j >= (int32_t)ld)
        return;
    double v;
    if (j < npad) {
        const double eye = (i == j) ? 1.0 : 0.0;
        if (i >= n || j >= n) {
            v = eye;
        } else if (mode == TPT_MFPT_ALL) {
            v = (eye - T[(size_t)i * n + j]) + pi[j];
        } else if (role[i] != TPT_FREE || role[j] != TPT_FREE) {
            v = eye;        // absorbing: row and column zeroed, the diagonal 1
        } else {
            v = eye - T[(size_t)i * n + j];
        }
    } else {
        const int32_t c = j - npad;
        v = 0.0;
        if (i < n) {
            if (mode == TPT_MFPT_ALL) {
                v = (i == c) ? 1.0 : 0.0;
            } else if (c == 0 && mode == TPT_MFPT_SINKS) {
                v = (role[i] == TPT_SINK) ? 0.0 : 1.0;
            } else if (c == 0) {
                if (role[i] == TPT_SINK) {
                    v = 1.0;
                } else if (role[i] == TPT_FREE) {
                    for (int32_t s = 0; s < n_sinks; ++s)
                        v += T[(size_t)i * n + sinks[s]];
                }
            }
        }
    }
    aug[(size_t)i * ld + j] = v;
}

// the general solve: A and B are copied in; this fills the padding
__global__ void __launch_bounds__(TPT_WG)
tpt_pad_kernel(int32_t n, int32_t nrhs, int32_t npad, int32_t nrp, double *__restrict__ aug)
{
    const size_t ld = (size_t)npad + nrp;
    const int32_t j = blockIdx.x * TPT_WG + threadIdx.x;
    const int32_t i = blockIdx.y;
    if (j >= (int32_t)ld)
        return;
    if (j < npad) {
        if (i >= n || j >= n)
            aug[(size_t)i * ld + j] = (i == j) ? 1.0 : 0.0;
    } else if (i >= n || j - npad >= nrhs) {
        aug[(size_t)i * ld + j] = 0.0;
    }
}

// ---- epilogues -------------------------------------------------------------------------
// the first right-hand side's solution -> out[n]; committors: the absorbing states exact
__global__ void __launch_bounds__(TPT_WG)
tpt_vector_kernel(int mode, int32_t n, int32_t npad, int32_t nrp,
                  const double *__restrict__ aug, const int32_t *__restrict__ role,
                  double lagtime, double *__restrict__ out)
{
    const int32_t i = blockIdx.x * TPT_WG + threadIdx.x;
    if (i >= n)
        return;
    const double x = aug[(size_t)i * ((size_t)npad + nrp) + npad];
    if (mode == TPT_MFPT_SINKS)
        out[i] = lagtime * x;
    else
        out[i] = (role[i] == TPT_SINK) ? 1.0 : (role[i] == TPT_SOURCE) ? 0.0 : x;
}

// out[i][j] = lagtime * (Z_jj - Z_ij) / pi_j, Z the solution block of the augmented matrix
__global__ void __launch_bounds__(TPT_WG)
tpt_mfpt_all_kernel(int32_t n, int32_t npad, const double *__restrict__ aug,
                    const double *__restrict__ pi, double lagtime, double *__restrict__ out)
{
    const size_t ld = 2 * (size_t)npad;
    const int32_t j = blockIdx.x * TPT_WG + threadIdx.x;
    const int32_t i = blockIdx.y;
    if (j >= n)
        return;
    const double zjj = aug[(size_t)j * ld + npad + j];
    const double zij = aug[(size_t)i * ld + npad + j];
    out[(size_t)i * n + j] = (lagtime * (zjj - zij)) / pi[j];
}

// f_ij = (T_ij * (pi_i * (1 - q_i))) * q_j, f_ii = 0; net: max(f_ij - f_ji, 0).  A
// workgroup takes the 32 x 32 tile (by, bx) and, for the net fluxes, reads the tile
// (bx, by) of T row by row as well and turns it over in the LDS.
__global__ void __launch_bounds__(TPT_WG)
tpt_flux_kernel(int32_t n, int net, const double *__restrict__ T,
                const double *__restrict__ pi, const double *__restrict__ q,
                double *__restrict__ out)
{
    __shared__ double ft[TPT_TILE][TPT_TILE + 1];
    const int tx = threadIdx.x % TPT_TILE, ty = threadIdx.x / TPT_TILE;    // 32 x 8
    const int32_t r0 = blockIdx.y * TPT_TILE, c0 = blockIdx.x * TPT_TILE;
    if (net) {
        // the transposed tile: rows c0 .., columns r0 ..
        for (int y = ty; y < TPT_TILE; y += TPT_WG / TPT_TILE) {
            const int32_t i = c0 + y, j = r0 + tx;
            double f = 0.0;
            if (i < n && j < n && i != j)
                f = (T[(size_t)i * n + j] * (pi[i] * (1.0 - q[i]))) * q[j];
            ft[y][tx] = f;
        }
        __syncthreads();
    }
    for (int y = ty; y < TPT_TILE; y += TPT_WG / TPT_TILE) {
        const int32_t i = r0 + y, j = c0 + tx;
        if (i >= n || j >= n)
            continue;
        double f = 0.0;
        if (i != j)
            f = (T[(size_t)i * n + j] * (pi[i] * (1.0 - q[i]))) * q[j];
        if (net) {
            const double d = f - ft[tx][y];
            f = (d < 0.0) ? 0.0 : d;
        }
        out[(size_t)i * n + j] = f;
    }
}

// ---- host side ---------------------------------------------------------------------------
static bool tpt_states_ok(const int32_t *s, int32_t count, int32_t n)
{
    if (!s || count < 1)
        return false;
    for (int32_t i = 0; i < count; ++i)
        if (s[i] < 0 || s[i] >= n)
            return false;
    return true;
}

// device memory for `bytes` more, with room to spare for the runtime
static int tpt_check_memory(size_t bytes, const char *who)
{
    size_t free_b = 0, total_b = 0;
    hipError_t e = hipMemGetInfo(&free_b, &total_b);
    if (e != hipSuccess)
        return ek_set_error(EK_EHIP, "%s: hipMemGetInfo: %s", who, hipGetErrorString(e));
    const size_t slack = (size_t)256 << 20;
    if (bytes + slack > free_b)
        return ek_set_error(EK_ENOMEM, "%s: the system needs %zu MiB of device memory, "
                                       "%zu MiB are free", who, bytes >> 20, free_b >> 20);
    return EK_OK;
}

// everything but TPT_GENERAL.  flux: 0 none, 1 fluxes, 2 net fluxes (TPT_COMMITTORS
// only: q_out and flux_out are both written)
static int tpt_run(const char *who, int mode, int device, int32_t n, const double *T,
                   const int32_t *sources, int32_t n_sources, const int32_t *sinks,
                   int32_t n_sinks, const double *pops, double lagtime, int flux,
                   double *vec_out, double *mat_out, int32_t *info_out)
{
    int rc = EK_OK;
    if (n < 1 || n > EK_LU_MAX_N || !T || !info_out)
        return ek_set_error(EK_EARG, "%s: bad argument (1 <= n <= %d)", who, EK_LU_MAX_N);
    const bool all = mode == TPT_MFPT_ALL;
    if ((all || flux) && (!pops || !mat_out))
        return ek_set_error(EK_EARG, "%s: populations and an output matrix are needed", who);
    if (!all && (!vec_out || !tpt_states_ok(sinks, n_sinks, n)))
        return ek_set_error(EK_EARG, "%s: sinks are indices below n, at least one", who);
    if (mode == TPT_COMMITTORS && !tpt_states_ok(sources, n_sources, n))
        return ek_set_error(EK_EARG, "%s: sources are indices below n, at least one", who);

    const int32_t npad = ek_lu_pad(n), nrp = all ? npad : EK_LU_NB;
    const size_t ld = (size_t)npad + nrp, nn = (size_t)n * n;
    int32_t *h_role = nullptr;
    double *d_T = nullptr, *d_aug = nullptr, *d_pi = nullptr, *d_vec = nullptr;
    int32_t *d_role = nullptr, *d_sinks = nullptr, *d_piv = nullptr, *d_status = nullptr;
    hipStream_t s = nullptr;

    if (!all) {
        h_role = new (std::nothrow) int32_t[(size_t)n]();
        if (!h_role)
            return ek_set_error(EK_ENOMEM, "%s: out of host memory", who);
        for (int32_t i = 0; i < n_sinks; ++i)
            h_role[sinks[i]] = TPT_SINK;
        for (int32_t i = 0; i < n_sources; ++i) {
            if (h_role[sources[i]] == TPT_SINK) {
                delete[] h_role;
                return ek_set_error(EK_EARG, "%s: state %d is both source and sink", who,
                                    sources[i]);
            }
            h_role[sources[i]] = TPT_SOURCE;
        }
    }
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess) {
            delete[] h_role;
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device,
                                hipGetErrorString(e0));
        }
    }
    rc = tpt_check_memory((nn + (size_t)npad * ld + 4 * (size_t)npad) * sizeof(double), who);
    if (rc != EK_OK) {
        delete[] h_role;
        return rc;
    }
    TPT_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    TPT_HIP(ek_dev_malloc((void **)&d_T, nn * sizeof(double)));
    TPT_HIP(ek_dev_malloc((void **)&d_aug, (size_t)npad * ld * sizeof(double)));
    TPT_HIP(ek_dev_malloc((void **)&d_piv, (size_t)npad * sizeof(int32_t)));
    TPT_HIP(ek_dev_malloc((void **)&d_status, sizeof(int32_t)));
    TPT_HIP(ek_dev_malloc((void **)&d_vec, (size_t)n * sizeof(double)));
    TPT_HIP(hipMemcpyAsync(d_T, T, nn * sizeof(double), hipMemcpyHostToDevice, s));
    TPT_HIP(hipMemsetAsync(d_status, 0xff, sizeof(int32_t), s));
    if (pops) {
        TPT_HIP(ek_dev_malloc((void **)&d_pi, (size_t)n * sizeof(double)));
        TPT_HIP(hipMemcpyAsync(d_pi, pops, (size_t)n * sizeof(double), hipMemcpyHostToDevice,
                               s));
    }
    if (!all) {
        TPT_HIP(ek_dev_malloc((void **)&d_role, (size_t)n * sizeof(int32_t)));
        TPT_HIP(ek_dev_malloc((void **)&d_sinks, (size_t)n_sinks * sizeof(int32_t)));
        TPT_HIP(hipMemcpyAsync(d_role, h_role, (size_t)n * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
        TPT_HIP(hipMemcpyAsync(d_sinks, sinks, (size_t)n_sinks * sizeof(int32_t),
                               hipMemcpyHostToDevice, s));
    }
    ek_lu_mark(EK_LU_T_OTHER, s);
    hipLaunchKernelGGL(tpt_assemble_kernel, dim3((unsigned)((ld + TPT_WG - 1) / TPT_WG), npad),
                       dim3(TPT_WG), 0, s, mode, n, npad, nrp, d_T, d_role, d_sinks, n_sinks,
                       d_pi, d_aug);
    ek_lu_solve_dev(d_aug, npad, nrp, d_piv, d_status, s);
    if (all) {
        // (T is not needed any more: the result takes its place)
        hipLaunchKernelGGL(tpt_mfpt_all_kernel, dim3((n + TPT_WG - 1) / TPT_WG, n),
                           dim3(TPT_WG), 0, s, n, npad, d_aug, d_pi, lagtime, d_T);
        TPT_HIP(hipMemcpyAsync(mat_out, d_T, nn * sizeof(double), hipMemcpyDeviceToHost, s));
    } else {
        hipLaunchKernelGGL(tpt_vector_kernel, dim3((n + TPT_WG - 1) / TPT_WG), dim3(TPT_WG), 0,
                           s, mode, n, npad, nrp, d_aug, d_role, lagtime, d_vec);
        TPT_HIP(hipMemcpyAsync(vec_out, d_vec, (size_t)n * sizeof(double),
                               hipMemcpyDeviceToHost, s));
        if (flux) {
            // (the augmented matrix is not needed any more: the fluxes go there)
            const unsigned nt = (n + TPT_TILE - 1) / TPT_TILE;
            hipLaunchKernelGGL(tpt_flux_kernel, dim3(nt, nt), dim3(TPT_WG), 0, s, n,
                               flux == 2 ? 1 : 0, d_T, d_pi, d_vec, d_aug);
            TPT_HIP(hipMemcpyAsync(mat_out, d_aug, nn * sizeof(double), hipMemcpyDeviceToHost,
                                   s));
        }
    }
    ek_lu_mark(EK_LU_T_OTHER, s);
    TPT_HIP(hipGetLastError());
    TPT_HIP(hipMemcpyAsync(info_out, d_status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    TPT_HIP(hipStreamSynchronize(s));
    ek_lu_collect();
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_T);
    (void)ek_dev_free(d_aug);
    (void)ek_dev_free(d_pi);
    (void)ek_dev_free(d_vec);
    (void)ek_dev_free(d_role);
    (void)ek_dev_free(d_sinks);
    (void)ek_dev_free(d_piv);
    (void)ek_dev_free(d_status);
    if (s)
        (void)ek_stream_destroy(s);
    delete[] h_role;
    return rc;
}

extern "C" int ek_tpt_committors(int device, int32_t n, const double *T,
                                 const int32_t *sources, int32_t n_sources,
                                 const int32_t *sinks, int32_t n_sinks, double *q_out,
                                 int32_t *info_out)
{
    return tpt_run("ek_tpt_committors", TPT_COMMITTORS, device, n, T, sources, n_sources, sinks,
                   n_sinks, nullptr, 1.0, 0, q_out, nullptr, info_out);
}

extern "C" int ek_tpt_mfpts_sinks(int device, int32_t n, const double *T, const int32_t *sinks,
                                  int32_t n_sinks, double lagtime, double *t_out,
                                  int32_t *info_out)
{
    return tpt_run("ek_tpt_mfpts_sinks", TPT_MFPT_SINKS, device, n, T, nullptr, 0, sinks,
                   n_sinks, nullptr, lagtime, 0, t_out, nullptr, info_out);
}

extern "C" int ek_tpt_mfpts_all(int device, int32_t n, const double *T, const double *pops,
                                double lagtime, double *mfpt_out, int32_t *info_out)
{
    return tpt_run("ek_tpt_mfpts_all", TPT_MFPT_ALL, device, n, T, nullptr, 0, nullptr, 0, pops,
                   lagtime, 0, nullptr, mfpt_out, info_out);
}

extern "C" int ek_tpt_fluxes(int device, int32_t n, const double *T, const int32_t *sources,
                             int32_t n_sources, const int32_t *sinks, int32_t n_sinks,
                             const double *pops, int32_t net, double *q_out, double *flux_out,
                             int32_t *info_out)
{
    return tpt_run("ek_tpt_fluxes", TPT_COMMITTORS, device, n, T, sources, n_sources, sinks,
                   n_sinks, pops, 1.0, net ? 2 : 1, q_out, flux_out, info_out);
}

extern "C" int ek_lu_solve(int device, int32_t n, const double *A, int32_t nrhs,
                           const double *B, double *X, int32_t *pivots_out, int32_t *info_out)
{
    int rc = EK_OK;
    if (n < 1 || n > EK_LU_MAX_N || nrhs < 1 || nrhs > n || !A || !B || !X || !info_out)
        return ek_set_error(EK_EARG, "ek_lu_solve: bad argument (1 <= nrhs <= n <= %d)",
                            EK_LU_MAX_N);
    const int32_t npad = ek_lu_pad(n), nrp = ek_lu_pad(nrhs);
    const size_t ld = (size_t)npad + nrp;
    double *d_aug = nullptr;
    int32_t *d_piv = nullptr, *d_status = nullptr;
    hipStream_t s = nullptr;
    {
        hipError_t e0 = hipSetDevice(device);
        if (e0 != hipSuccess)
            return ek_set_error(EK_EHIP, "hipSetDevice(%d): %s", device,
                                hipGetErrorString(e0));
    }
    rc = tpt_check_memory(((size_t)npad * ld + (size_t)npad) * sizeof(double), "ek_lu_solve");
    if (rc != EK_OK)
        return rc;
    TPT_HIP(ek_stream_create_flags(&s, hipStreamNonBlocking));
    TPT_HIP(ek_dev_malloc((void **)&d_aug, (size_t)npad * ld * sizeof(double)));
    TPT_HIP(ek_dev_malloc((void **)&d_piv, (size_t)npad * sizeof(int32_t)));
    TPT_HIP(ek_dev_malloc((void **)&d_status, sizeof(int32_t)));
    TPT_HIP(hipMemsetAsync(d_status, 0xff, sizeof(int32_t), s));
    TPT_HIP(hipMemcpy2DAsync(d_aug, ld * sizeof(double), A, (size_t)n * sizeof(double),
                             (size_t)n * sizeof(double), n, hipMemcpyHostToDevice, s));
    TPT_HIP(hipMemcpy2DAsync(d_aug + npad, ld * sizeof(double), B,
                             (size_t)nrhs * sizeof(double), (size_t)nrhs * sizeof(double), n,
                             hipMemcpyHostToDevice, s));
    ek_lu_mark(EK_LU_T_OTHER, s);
    hipLaunchKernelGGL(tpt_pad_kernel, dim3((unsigned)((ld + TPT_WG - 1) / TPT_WG), npad),
                       dim3(TPT_WG), 0, s, n, nrhs, npad, nrp, d_aug);
    ek_lu_solve_dev(d_aug, npad, nrp, d_piv, d_status, s);
    TPT_HIP(hipGetLastError());
    TPT_HIP(hipMemcpy2DAsync(X, (size_t)nrhs * sizeof(double), d_aug + npad,
                             ld * sizeof(double), (size_t)nrhs * sizeof(double), n,
                             hipMemcpyDeviceToHost, s));
    if (pivots_out)
        TPT_HIP(hipMemcpyAsync(pivots_out, d_piv, (size_t)n * sizeof(int32_t),
                               hipMemcpyDeviceToHost, s));
    TPT_HIP(hipMemcpyAsync(info_out, d_status, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    TPT_HIP(hipStreamSynchronize(s));
    ek_lu_collect();
done:
    if (s)
        (void)hipStreamSynchronize(s);
    (void)ek_dev_free(d_aug);
    (void)ek_dev_free(d_piv);
    (void)ek_dev_free(d_status);
    if (s)
        (void)ek_stream_destroy(s);
    return rc;
}
