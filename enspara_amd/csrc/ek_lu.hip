// ek_lu.hip -- dense float64 solve A X = B: blocked right-looking LU with partial
// pivoting, the trailing update on the matrix cores (v_mfma_f64_16x16x4_f64).
//
// The system is held as the augmented matrix [A | B], row-major, padded to whole
// panels of EK_LU_NB = 64 rows and columns (identity / zeros in the padding, so no
// kernel has a ragged edge and none reads outside the allocation).  Eliminating
// on [A | B] makes the forward substitution part of the factorisation: the row
// exchanges, the block-row solve and the trailing update run over the columns of
// B as well, and the columns left of a panel (L, which nothing reads again) are
// not exchanged.  What remains is the back substitution with U.
//
// Per panel, on one stream, none of which the host waits for:
//   panel   eight sub-panels of 8 columns, each three launches:
//           sub-panel  one workgroup, a thread per row with the row's 8 values in
//                      registers (rows past 4096 in memory): per column the pivot
//                      (largest |a|, lowest row on ties, NaN before everything), the
//                      exchange, l = a / pivot, the rank-one update of the columns
//                      right of it -- the block is read once and written once
//           columns    a thread per other column of the panel: the 8 exchanges, and
//                      right of the sub-panel the 8 x 8 triangular solve
//           update     the panel's columns right of the sub-panel, rows below it:
//                      minus the 8 products, in the order of the columns
//           (a single workgroup cannot stream a 64-column panel 64 times: measured at
//           n = 5000, that form spent 350 ms of a 395 ms call in the panel)
//   swap    the panel's 64 exchanges on every column right of it, one thread per
//           column
//   trsm    U12 = L11^-1 A12: L11 in the LDS, one thread per column, the column's
//           64 values in registers
//   gemm    A22 -= L21 U12: 64 x 64 tiles of C per workgroup, four waves of 32 x 32,
//           L21 (negated, which is exact) and U12 staged through the LDS in halves
//           of 32, 16 MFMAs of 16x16x4 per 16 x 16 tile; the 64 products are summed
//           from zero and added to C once
// Back substitution, per panel from the last: the diagonal block (U in the LDS, one
// thread per right-hand side), then the rows above through the same gemm kernel.
//
// Everything is float64.  FMAs are explicit (-ffp-contract=off); the order of
// every sum is the code's, there are no atomics: two runs give the same bits.
// A zero or NaN pivot is recorded (the first such column) and its column is left
// unscaled; the run goes on and the caller reads the status word at the end.
#include "ek_lu.h"

typedef double ek_v4d __attribute__((ext_vector_type(4)));

#define LU_PANEL_WG 1024
#define LU_PANEL_WAVES (LU_PANEL_WG / EK_WAVE)
#define LU_SUB 8            // columns of a sub-panel
#define LU_SUB_RPT 4        // rows of it a thread keeps in registers
#define LU_INNER_ROWS 64    // rows per workgroup of the update inside the panel
#define LU_COL_WG 256
#define LU_GEMM_WG 256
#define LU_AS_LD 36     // doubles per row of the A stage [64][32 + 4]: conflict-free b64 reads
#define LU_BS_LD 80     // ... of the B stage [32][64 + 16]

static_assert(EK_LU_NB == EK_WAVE && EK_LU_NB % LU_SUB == 0, "whole sub-panels; a wave per panel row");

// ---- timing (tools only; one call at a time) --------------------------------------
#define LU_MAX_MARKS 4096
static int g_lu_timing = 0;
static int g_lu_n_marks = 0;
static hipEvent_t g_lu_ev[LU_MAX_MARKS];
static int g_lu_kind[LU_MAX_MARKS];
static double g_lu_ms[EK_LU_T_COUNT];
static double g_lu_flops[2], g_lu_flops_run[2];     // trailing update, back substitution

void ek_lu_mark(int kind, hipStream_t s)
{
    if (!g_lu_timing || g_lu_n_marks >= LU_MAX_MARKS)
        return;
    hipEvent_t e;
    if (ek_event_create(&e) != hipSuccess)
        return;
    (void)hipEventRecord(e, s);
    g_lu_ev[g_lu_n_marks] = e;
    g_lu_kind[g_lu_n_marks++] = kind;
}

void ek_lu_collect(void)
{
    if (!g_lu_timing)
        return;
    for (int k = 0; k < EK_LU_T_COUNT; ++k)
        g_lu_ms[k] = 0.0;
    for (int i = 0; i + 1 < g_lu_n_marks; ++i) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, g_lu_ev[i], g_lu_ev[i + 1]) == hipSuccess)
            g_lu_ms[g_lu_kind[i]] += (double)ms;
    }
    for (int i = 0; i < g_lu_n_marks; ++i)
        (void)ek_event_destroy(g_lu_ev[i]);
    g_lu_n_marks = 0;
    for (int k = 0; k < 2; ++k) {
        g_lu_flops[k] = g_lu_flops_run[k];
        g_lu_flops_run[k] = 0.0;
    }
}

extern "C" int ek_lu_set_timing(int on)
{
    g_lu_timing = on != 0;
    return EK_OK;
}

extern "C" int ek_lu_last_timing(double *ms_out, double *gemm_flops_out)
{
    if (!ms_out || !gemm_flops_out)
        return EK_EARG;
    for (int k = 0; k < EK_LU_T_COUNT; ++k)
        ms_out[k] = g_lu_ms[k];
    gemm_flops_out[0] = g_lu_flops[0];
    gemm_flops_out[1] = g_lu_flops[1];
    return EK_OK;
}

// ---- the panel -----------------------------------------------------------------------
// the order of pivot candidates: NaN counts as +inf, larger first, lower row on ties
__device__ __forceinline__ double lu_key(double v)
{
    return (v != v) ? INFINITY : fabs(v);
}
__device__ __forceinline__ bool lu_better(double k, int32_t r, double bk, int32_t br)
{
    return (k > bk) || (k == bk && r < br);
}

__global__ void __launch_bounds__(LU_PANEL_WG)
lu_subpanel_kernel(double *__restrict__ a, size_t ld, int32_t npad, int32_t c0,
                   int32_t *__restrict__ piv, int32_t *__restrict__ status)
{
    __shared__ double s_key[LU_PANEL_WAVES];
    __shared__ int32_t s_row[LU_PANEL_WAVES];
    __shared__ double s_top[LU_SUB], s_piv[LU_SUB];     // rows c and p as the step finds them
    __shared__ int32_t s_p;
    const int tid = threadIdx.x, lane = tid & (EK_WAVE - 1), wave = tid / EK_WAVE;
    const int32_t tail0 = c0 + LU_SUB_RPT * LU_PANEL_WG;     // rows from here on stay in memory

    // this thread's rows c0 + tid + 1024 i: the first LU_SUB_RPT of them in registers
    double x[LU_SUB_RPT][LU_SUB];
#pragma unroll
    for (int i = 0; i < LU_SUB_RPT; ++i) {
        const int32_t r = c0 + tid + i * LU_PANEL_WG;
#pragma unroll
        for (int t = 0; t < LU_SUB; ++t)
            x[i][t] = (r < npad) ? a[(size_t)r * ld + c0 + t] : 0.0;
    }

#pragma unroll
    for (int j = 0; j < LU_SUB; ++j) {
        const int32_t c = c0 + j;
        // the pivot: largest key, lowest row on ties
        double key = -1.0;
        int32_t row = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < LU_SUB_RPT; ++i) {
            const int32_t r = c0 + tid + i * LU_PANEL_WG;
            if (r >= c && r < npad) {
                const double k = lu_key(x[i][j]);
                if (lu_better(k, r, key, row)) {
                    key = k;
                    row = r;
                }
            }
        }
        for (int32_t r = tail0 + tid; r < npad; r += LU_PANEL_WG) {
            const double k = lu_key(a[(size_t)r * ld + c]);
            if (lu_better(k, r, key, row)) {
                key = k;
                row = r;
            }
        }
#pragma unroll
        for (int o = EK_WAVE / 2; o >= 1; o >>= 1) {
            const double ok = __shfl_xor(key, o, EK_WAVE);
            const int32_t orow = __shfl_xor(row, o, EK_WAVE);
            if (lu_better(ok, orow, key, row)) {
                key = ok;
                row = orow;
            }
        }
        if (lane == 0) {
            s_key[wave] = key;
            s_row[wave] = row;
        }
        __syncthreads();
        if (tid == 0) {
            double bk = s_key[0];
            int32_t br = s_row[0];
            for (int w = 1; w < LU_PANEL_WAVES; ++w)
                if (lu_better(s_key[w], s_row[w], bk, br)) {
                    bk = s_key[w];
                    br = s_row[w];
                }
            if (br < c || br >= npad)       // (cannot happen: row c is always a candidate)
                br = c;
            piv[c] = br;
            s_p = br;
        }
        __syncthreads();
        const int32_t p = s_p;
        // rows c and p change places over the sub-panel's eight columns (the
        // multipliers already in them travel with their rows)
        const bool own_tail_p = p >= tail0 && (p - c0) % LU_PANEL_WG == tid;
#pragma unroll
        for (int i = 0; i < LU_SUB_RPT; ++i) {
            const int32_t r = c0 + tid + i * LU_PANEL_WG;
            if (r == c) {
#pragma unroll
                for (int t = 0; t < LU_SUB; ++t)
                    s_top[t] = x[i][t];
            }
            if (r == p) {
#pragma unroll
                for (int t = 0; t < LU_SUB; ++t)
                    s_piv[t] = x[i][t];
            }
        }
        if (own_tail_p) {
#pragma unroll
            for (int t = 0; t < LU_SUB; ++t)
                s_piv[t] = a[(size_t)p * ld + c0 + t];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < LU_SUB_RPT; ++i) {
            const int32_t r = c0 + tid + i * LU_PANEL_WG;
            if (r == c) {
#pragma unroll
                for (int t = 0; t < LU_SUB; ++t)
                    x[i][t] = s_piv[t];
            } else if (r == p) {
#pragma unroll
                for (int t = 0; t < LU_SUB; ++t)
                    x[i][t] = s_top[t];
            }
        }
        if (own_tail_p) {
#pragma unroll
            for (int t = 0; t < LU_SUB; ++t)
                a[(size_t)p * ld + c0 + t] = s_top[t];
        }
        const double pv = s_piv[j];
        const bool ok = (pv == pv) && (pv != 0.0);
        if (!ok && tid == 0 && *status < 0)
            *status = c;
        // l = a / pivot, then the rank-one update of the columns right of j (not with a
        // zero or NaN pivot: the column stays unscaled)
#pragma unroll
        for (int i = 0; i < LU_SUB_RPT; ++i) {
            const int32_t r = c0 + tid + i * LU_PANEL_WG;
            if (ok && r > c && r < npad) {
                const double l = x[i][j] / pv;
                x[i][j] = l;
#pragma unroll
                for (int t = j + 1; t < LU_SUB; ++t)
                    x[i][t] = fma(-l, s_piv[t], x[i][t]);
            }
        }
        for (int32_t r = tail0 + tid; ok && r < npad; r += LU_PANEL_WG) {
            double *xr = a + (size_t)r * ld + c0;
            const double l = xr[j] / pv;
            xr[j] = l;
#pragma unroll
            for (int t = j + 1; t < LU_SUB; ++t)
                xr[t] = fma(-l, s_piv[t], xr[t]);
        }
    }
#pragma unroll
    for (int i = 0; i < LU_SUB_RPT; ++i) {
        const int32_t r = c0 + tid + i * LU_PANEL_WG;
        if (r < npad) {
#pragma unroll
            for (int t = 0; t < LU_SUB; ++t)
                a[(size_t)r * ld + c0 + t] = x[i][t];
        }
    }
}

// the sub-panel's eight exchanges on the panel's other columns (left of it too: their
// multipliers travel with their rows), and U12 = L11^-1 A12 of the eight rows for the
// columns right of it; one thread per column of the panel
__global__ void __launch_bounds__(EK_LU_NB)
lu_inner_col_kernel(double *__restrict__ a, size_t ld, int32_t k0, int32_t c0,
                    const int32_t *__restrict__ piv)
{
    const int32_t col = k0 + threadIdx.x;
    if (col >= c0 && col < c0 + LU_SUB)
        return;
    for (int j = 0; j < LU_SUB; ++j) {
        const int32_t r = c0 + j, p = piv[r];
        if (p != r) {
            const double x = a[(size_t)r * ld + col], y = a[(size_t)p * ld + col];
            a[(size_t)r * ld + col] = y;
            a[(size_t)p * ld + col] = x;
        }
    }
    if (col < c0)
        return;
    double x[LU_SUB];
#pragma unroll
    for (int t = 0; t < LU_SUB; ++t)
        x[t] = a[(size_t)(c0 + t) * ld + col];
#pragma unroll
    for (int i = 0; i < LU_SUB; ++i)
#pragma unroll
        for (int r = i + 1; r < LU_SUB; ++r)
            x[r] = fma(-a[(size_t)(c0 + r) * ld + c0 + i], x[i], x[r]);
#pragma unroll
    for (int t = 0; t < LU_SUB; ++t)
        a[(size_t)(c0 + t) * ld + col] = x[t];
}

// A22 -= L21 U12 inside the panel: rows below the sub-panel's eight, the panel's
// columns right of it; the eight products of an element in the order of the columns
__global__ void __launch_bounds__(LU_COL_WG)
lu_inner_update_kernel(double *__restrict__ a, size_t ld, int32_t npad, int32_t k0,
                       int32_t c0)
{
    __shared__ double us[LU_SUB][EK_LU_NB];
    const int lane = threadIdx.x & (EK_WAVE - 1), wave = threadIdx.x / EK_WAVE;
    const int32_t col0 = c0 + LU_SUB, ncols = k0 + EK_LU_NB - col0;
    for (int i = threadIdx.x; i < LU_SUB * EK_LU_NB; i += LU_COL_WG) {
        const int t = i / EK_LU_NB, cc = i % EK_LU_NB;
        us[t][cc] = (cc < ncols) ? a[(size_t)(c0 + t) * ld + col0 + cc] : 0.0;
    }
    __syncthreads();
    if (lane >= ncols)
        return;
    const int32_t r0 = c0 + LU_SUB + blockIdx.x * LU_INNER_ROWS;
    for (int32_t r = r0 + wave; r < r0 + LU_INNER_ROWS && r < npad;
         r += LU_COL_WG / EK_WAVE) {
        const double *lr = a + (size_t)r * ld + c0;
        double v = a[(size_t)r * ld + col0 + lane];
#pragma unroll
        for (int t = 0; t < LU_SUB; ++t)
            v = fma(-lr[t], us[t][lane], v);
        a[(size_t)r * ld + col0 + lane] = v;
    }
}

// ---- the panel's exchanges on the columns right of it ------------------------------
__global__ void __launch_bounds__(LU_COL_WG)
lu_swap_kernel(double *__restrict__ a, size_t ld, int32_t k0, int32_t col0, int32_t ncols,
               const int32_t *__restrict__ piv)
{
    const int32_t t = blockIdx.x * LU_COL_WG + threadIdx.x;
    if (t >= ncols)
        return;
    const size_t col = (size_t)col0 + t;
    for (int j = 0; j < EK_LU_NB; ++j) {
        const int32_t r = k0 + j, p = piv[r];
        if (p != r) {
            const double x = a[(size_t)r * ld + col], y = a[(size_t)p * ld + col];
            a[(size_t)r * ld + col] = y;
            a[(size_t)p * ld + col] = x;
        }
    }
}

// ---- triangular solves with a 64 x 64 diagonal block -------------------------------
// UPPER = false: X = L^-1 X, L unit lower; UPPER = true: X = U^-1 X.  The block is
// rows and columns k0 .. k0 + 63 of a; X is rows k0 .. k0 + 63 of columns col0 ..
template <bool UPPER>
__global__ void __launch_bounds__(LU_COL_WG)
lu_trsm_kernel(double *__restrict__ a, size_t ld, int32_t k0, int32_t col0, int32_t ncols)
{
    __shared__ double tri[EK_LU_NB][EK_LU_NB];
    for (int i = threadIdx.x; i < EK_LU_NB * EK_LU_NB; i += LU_COL_WG)
        tri[i / EK_LU_NB][i % EK_LU_NB] =
            a[(size_t)(k0 + i / EK_LU_NB) * ld + k0 + i % EK_LU_NB];
    __syncthreads();
    const int32_t t = blockIdx.x * LU_COL_WG + threadIdx.x;
    if (t >= ncols)
        return;
    double *x0 = a + (size_t)k0 * ld + col0 + t;
    double x[EK_LU_NB];
#pragma unroll
    for (int r = 0; r < EK_LU_NB; ++r)
        x[r] = x0[(size_t)r * ld];
    if (UPPER) {
#pragma unroll
        for (int i = EK_LU_NB - 1; i >= 0; --i) {
            const double xi = x[i] / tri[i][i];
            x[i] = xi;
#pragma unroll
            for (int r = 0; r < i; ++r)
                x[r] = fma(-tri[r][i], xi, x[r]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < EK_LU_NB; ++i) {
            const double xi = x[i];
#pragma unroll
            for (int r = i + 1; r < EK_LU_NB; ++r)
                x[r] = fma(-tri[r][i], xi, x[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < EK_LU_NB; ++r)
        x0[(size_t)r * ld] = x[r];
}

// ---- C -= A B on the matrix cores ----------------------------------------------------
// C: rows crow0 + 64 by .., columns ccol0 + 64 bx ..; A: the same rows, columns acol0 ..
// acol0 + 63; B: rows brow0 .. brow0 + 63, the same columns as C.  All inside a, none
// of A or B is written by the launch.  v_mfma_f64_16x16x4_f64: lane l gives
// A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15] and holds, in register i,
// C[row (l >> 4) + 4 i][col l & 15].
__global__ void __launch_bounds__(LU_GEMM_WG)
lu_gemm_kernel(double *__restrict__ a, size_t ld, int32_t crow0, int32_t ccol0,
               int32_t acol0, int32_t brow0)
{
    __shared__ double As[EK_LU_NB][LU_AS_LD];
    __shared__ double Bs[EK_LU_NB / 2][LU_BS_LD];
    const int tid = threadIdx.x, lane = tid & (EK_WAVE - 1), w = tid / EK_WAVE;
    const int wm = (w >> 1) * 32, wn = (w & 1) * 32;
    const int l15 = lane & 15, l4 = lane >> 4;
    const size_t rbase = (size_t)crow0 + (size_t)blockIdx.y * EK_LU_NB;
    const size_t cbase = (size_t)ccol0 + (size_t)blockIdx.x * EK_LU_NB;

    // The products are summed from zero and added to C once.  Summed into C they were
    // rounded at C's magnitude 16 times per launch, n / 4 times over a factorisation:
    // eta_dev grew like sqrt(n) (11 eta_ref on a dominant matrix at n = 1100), where a
    // BLAS, which sums this way, stays flat.
    ek_v4d acc[2][2], cin[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                cin[mi][ni][i] = a[(rbase + wm + mi * 16 + l4 + 4 * i) * ld + cbase + wn +
                                   ni * 16 + l15];
                acc[mi][ni][i] = 0.0;
            }

    for (int kh = 0; kh < 2; ++kh) {
        if (kh)
            __syncthreads();
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int idx = tid + LU_GEMM_WG * e;
            const int ar = idx >> 5, ak = idx & 31;
            As[ar][ak] = -a[(rbase + ar) * ld + acol0 + kh * 32 + ak];
            const int bk = idx >> 6, bc = idx & 63;
            Bs[bk][bc] = a[((size_t)brow0 + kh * 32 + bk) * ld + cbase + bc];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const double a0 = As[wm + l15][kk * 4 + l4];
            const double a1 = As[wm + 16 + l15][kk * 4 + l4];
            const double b0 = Bs[kk * 4 + l4][wn + l15];
            const double b1 = Bs[kk * 4 + l4][wn + 16 + l15];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                a[(rbase + wm + mi * 16 + l4 + 4 * i) * ld + cbase + wn + ni * 16 + l15] =
                    cin[mi][ni][i] + acc[mi][ni][i];
}

static void lu_gemm(double *aug, size_t ld, int32_t crow0, int32_t nrows, int32_t ccol0,
                    int32_t ncols, int32_t acol0, int32_t brow0, int back,
                    hipStream_t s)
{
    hipLaunchKernelGGL(lu_gemm_kernel, dim3(ncols / EK_LU_NB, nrows / EK_LU_NB),
                       dim3(LU_GEMM_WG), 0, s, aug, ld, crow0, ccol0, acol0, brow0);
    g_lu_flops_run[back] += 2.0 * EK_LU_NB * (double)nrows * (double)ncols;
}

void ek_lu_solve_dev(double *aug, int32_t npad, int32_t nrp, int32_t *piv,
                     int32_t *status, hipStream_t s)
{
    const size_t ld = (size_t)npad + (size_t)nrp;
    const int nblk = npad / EK_LU_NB;
    g_lu_flops_run[0] = g_lu_flops_run[1] = 0.0;
    for (int kb = 0; kb < nblk; ++kb) {
        const int32_t k0 = kb * EK_LU_NB, right = k0 + EK_LU_NB;
        const int32_t ncols = (int32_t)(ld - right);        // >= nrp >= 64
        const int cblocks = (ncols + LU_COL_WG - 1) / LU_COL_WG;
        ek_lu_mark(EK_LU_T_PANEL, s);
        for (int32_t c0 = k0; c0 < right; c0 += LU_SUB) {
            hipLaunchKernelGGL(lu_subpanel_kernel, dim3(1), dim3(LU_PANEL_WG), 0, s, aug, ld,
                               npad, c0, piv, status);
            hipLaunchKernelGGL(lu_inner_col_kernel, dim3(1), dim3(EK_LU_NB), 0, s, aug, ld, k0,
                               c0, piv);
            const int32_t below = npad - (c0 + LU_SUB);
            if (c0 + LU_SUB < right && below > 0)
                hipLaunchKernelGGL(lu_inner_update_kernel,
                                   dim3((below + LU_INNER_ROWS - 1) / LU_INNER_ROWS),
                                   dim3(LU_COL_WG), 0, s, aug, ld, npad, k0, c0);
        }
        ek_lu_mark(EK_LU_T_SWAP, s);
        hipLaunchKernelGGL(lu_swap_kernel, dim3(cblocks), dim3(LU_COL_WG), 0, s, aug, ld, k0,
                           right, ncols, piv);
        ek_lu_mark(EK_LU_T_TRSM, s);
        hipLaunchKernelGGL(lu_trsm_kernel<false>, dim3(cblocks), dim3(LU_COL_WG), 0, s, aug,
                           ld, k0, right, ncols);
        if (right < npad) {
            ek_lu_mark(EK_LU_T_GEMM, s);
            lu_gemm(aug, ld, right, npad - right, right, ncols, k0, k0, 0, s);
        }
    }
    const int rblocks = (nrp + LU_COL_WG - 1) / LU_COL_WG;
    for (int kb = nblk - 1; kb >= 0; --kb) {
        const int32_t k0 = kb * EK_LU_NB;
        ek_lu_mark(EK_LU_T_BTRSM, s);
        hipLaunchKernelGGL(lu_trsm_kernel<true>, dim3(rblocks), dim3(LU_COL_WG), 0, s, aug, ld,
                           k0, npad, nrp);
        if (kb > 0) {
            ek_lu_mark(EK_LU_T_BGEMM, s);
            lu_gemm(aug, ld, 0, k0, npad, nrp, k0, k0, 1, s);
        }
    }
    ek_lu_mark(EK_LU_T_OTHER, s);
}
