// ek_lu.h -- the dense float64 solver of ek_lu.hip, as the rest of the library
// sees it (ek_tpt.hip).
#pragma once
#include "ek_common.h"

#define EK_LU_NB 64             // panel width; every padded size is a multiple of it
#define EK_LU_MAX_N 32768       // rows of a system (the augmented matrix has at most 2 n columns)

static inline int32_t ek_lu_pad(int32_t n)
{
    return (n + EK_LU_NB - 1) / EK_LU_NB * EK_LU_NB;
}

// what the launches between two marks are (ek_lu_last_timing)
enum {
    EK_LU_T_OTHER = 0,      // assembly and epilogues
    EK_LU_T_PANEL = 1,
    EK_LU_T_SWAP = 2,
    EK_LU_T_TRSM = 3,
    EK_LU_T_GEMM = 4,       // the trailing update (right-hand sides included)
    EK_LU_T_BTRSM = 5,      // back substitution: the diagonal blocks
    EK_LU_T_BGEMM = 6,      // ... the blocks above them, through the same kernel as 4
    EK_LU_T_COUNT = 7
};
// with ek_lu_set_timing(1): an event on s; what follows it is of kind `kind`
void ek_lu_mark(int kind, hipStream_t s);
// after the stream was synchronised: sum the intervals of the call
void ek_lu_collect(void);

// Gaussian elimination with partial pivoting of the augmented matrix [A | B],
// then back substitution: aug is row-major [npad][npad + nrp] on the device, npad
// and nrp multiples of EK_LU_NB, rows and columns past the system's own an
// identity (A) and zeros (B).  On return the B part holds X; piv[k] = the row
// exchanged with row k at step k; *status (set to -1 by the caller) = the first
// column whose pivot was zero or NaN.  Launches only; nothing is waited for.
void ek_lu_solve_dev(double *aug, int32_t npad, int32_t nrp, int32_t *piv,
                     int32_t *status, hipStream_t s);
