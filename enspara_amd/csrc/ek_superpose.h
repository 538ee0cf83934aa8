// ek_superpose.h -- the optimal rotation from the 3x3 inner-product matrix and the
// root ek_qcp.h's iteration ends at.  gfx950, and g++ for
// tests/test_rmsf_host.py: float64, every fused multiply-add explicit, no square
// root in float64.
//
// Replaces what the reference's enspara/geometry/rmsf.py takes from
// md.Trajectory.superpose.
//
// S[3 i + j] = sum_a x_ai y_aj (x the centred frame, y the centred reference), K
// the symmetric traceless 4x4 key matrix of ek_quartic_from_S.  The unit
// eigenvector of K's largest eigenvalue lam is the quaternion (w, x, y, z) of the
// rotation R that takes x onto y (Horn 1987); every non-zero row of adj(K - lam I)
// is a multiple of it.
//
//   1. everything is divided by m = max |S_ij| first: only ratios matter, and the
//      cubes and sixth powers below stay in range for coordinates of 1e-15 or 1e9;
//   2. THE GAP.  With singular values s1 >= s2 >= |s3| of S (s3 signed like det S)
//      the two largest eigenvalues of K are s1 + s2 + s3 and s1 - s2 - s3: g = 2 (s2 +
//      s3).  lam is NOT used for it: at a (nearly) double root the iteration ends in
//      rounding noise or jumps (ek_qcp.h, "Near a multiple root"), and anything
//      computed from K - lam I sees g + noise.  Instead s1^2, the largest root of the
//      characteristic cubic of S^T S, x^3 - q x^2 + b x - d^2 (q = sum S_ij^2, b = |cof
//      S|_F^2, d = det S), by Newton from q (from above, monotone), and
//          (s2 + s3)^2 = (q - s1^2) + 2 d / s1,
//      s1 from a float32 square root and two Heron steps.  The frame is flagged
//      iff (s2 + s3)^2 <= 1e-10 ((Gx + Gy) / m)^2, i.e. g <= 2e-5 (Gx + Gy): a factor
//      of 5 below where a flag is forbidden (1e-4) and 200 above where it is
//      required (1e-7); float32 roundings of S move g by ~1e-7 sqrt(n) of its scale.
//      Where s1^2 is itself a double root (s1 = s2) Newton is only linear and x is
//      good to ~1e-8 q; that matters only if also s3 = -s2 (S a multiple of an
//      improper rotation), where the verdict inside g < 2e-4 (Gx + Gy) may go
//      either way;
//   3. all four rows of adj(K - lam I) from the twelve 2x2 minors of its row pairs
//      (0,1) and (2,3); the row of largest norm (the first of equals) is q;
//   4. R = M(q) / |q|^2: dividing the quadratic form by the squared norm is the
//      normalisation, without a square root.
#pragma once
#include "ek_qcp.h"

#define EK_SUP_GAP2 1e-10       // on (s2 + s3)^2 / (Gx + Gy)^2, see 2.
#define EK_SUP_CUBIC_IT 60

// a b - c d
__device__ __forceinline__ double ek_sup_dm(double a, double b, double c, double d)
{
    return __builtin_fma(a, b, -(c * d));
}

// (s2 + s3)^2 of a 3x3 matrix whose largest entry is 1 in magnitude
__device__ __forceinline__ double ek_sup_gap2(const double (&s)[9])
{
    double q = s[0] * s[0];
    for (int j = 1; j < 9; ++j)
        q = __builtin_fma(s[j], s[j], q);
    double c[9];
    c[0] = ek_sup_dm(s[4], s[8], s[5], s[7]);
    c[1] = ek_sup_dm(s[5], s[6], s[3], s[8]);
    c[2] = ek_sup_dm(s[3], s[7], s[4], s[6]);
    c[3] = ek_sup_dm(s[2], s[7], s[1], s[8]);
    c[4] = ek_sup_dm(s[0], s[8], s[2], s[6]);
    c[5] = ek_sup_dm(s[1], s[6], s[0], s[7]);
    c[6] = ek_sup_dm(s[1], s[5], s[2], s[4]);
    c[7] = ek_sup_dm(s[2], s[3], s[0], s[5]);
    c[8] = ek_sup_dm(s[0], s[4], s[1], s[3]);
    double b = c[0] * c[0];
    for (int j = 1; j < 9; ++j)
        b = __builtin_fma(c[j], c[j], b);
    const double d = __builtin_fma(s[2], c[2], __builtin_fma(s[1], c[1], s[0] * c[0]));
    const double d2 = d * d;
    // s1^2: the cubic is convex and increasing beyond its largest root, every step
    // from above is positive and lands at or above the root; s1^2 >= q / 3
    double x = q;
    for (int it = 0; it < EK_SUP_CUBIC_IT; ++it) {
        const double f = __builtin_fma(__builtin_fma(x - q, x, b), x, -d2);
        const double fp = __builtin_fma(__builtin_fma(3.0, x, -2.0 * q), x, b);
        if (!(fp > 0.0))
            break;
        const double step = f / fp;
        const double nxt = x - step;
        if (!(step > 0.0 && 3.0 * nxt >= q))
            break;
        x = nxt;
        if (step <= 1e-16 * x)
            break;
    }
    // s1 in [1 / sqrt 3, 3]: float32 root, two Heron steps
    double r = (double)__builtin_sqrtf((float)x);
    r = 0.5 * (r + x / r);
    r = 0.5 * (r + x / r);
    return (q - x) + (2.0 * d) / r;
}

// R (row-major, aligned = R x_centred) of the frame whose inner products with the
// reference are S; returns 1 (and the identity) where the rotation is not determined
__device__ __forceinline__ int ek_superpose_from_S(const float (&S)[9], double Gx, double Gy,
                                                   double lam, double (&R)[9])
{
    for (int j = 0; j < 9; ++j)
        R[j] = (j % 4 == 0) ? 1.0 : 0.0;
    double m = 0.0;
    for (int j = 0; j < 9; ++j) {
        const double v = __builtin_fabs((double)S[j]);
        m = (v > m) ? v : m;
    }
    const double Gsum = Gx + Gy;
    if (!(m > 0.0 && Gsum > 0.0))
        return 1;
    double s[9];
    for (int j = 0; j < 9; ++j)
        s[j] = (double)S[j] / m;
    const double Gn = Gsum / m, ln = lam / m;
    if (!(ek_sup_gap2(s) > EK_SUP_GAP2 * (Gn * Gn)))
        return 1;

    // M = K - lam I, K as ek_quartic_from_S builds it
    const double m00 = ((s[0] + s[4]) + s[8]) - ln;
    const double m01 = s[5] - s[7];
    const double m02 = s[6] - s[2];
    const double m03 = s[1] - s[3];
    const double m11 = ((s[0] - s[4]) - s[8]) - ln;
    const double m12 = s[1] + s[3];
    const double m13 = s[6] + s[2];
    const double m22 = ((s[4] - s[0]) - s[8]) - ln;
    const double m23 = s[5] + s[7];
    const double m33 = ((s[8] - s[0]) - s[4]) - ln;
    // 2x2 minors of rows (0, 1) and of rows (2, 3); M is symmetric: m_ij = m_ji
    const double a0 = ek_sup_dm(m00, m11, m01, m01);
    const double a1 = ek_sup_dm(m00, m12, m01, m02);
    const double a2 = ek_sup_dm(m00, m13, m01, m03);
    const double a3 = ek_sup_dm(m01, m12, m11, m02);
    const double a4 = ek_sup_dm(m01, m13, m11, m03);
    const double a5 = ek_sup_dm(m02, m13, m12, m03);
    const double b5 = ek_sup_dm(m22, m33, m23, m23);
    const double b4 = ek_sup_dm(m12, m33, m13, m23);
    const double b3 = ek_sup_dm(m12, m23, m13, m22);
    const double b2 = ek_sup_dm(m02, m33, m03, m23);
    const double b1 = ek_sup_dm(m02, m23, m03, m22);
    const double b0 = ek_sup_dm(m02, m13, m03, m12);
    double adj[4][4];
    adj[0][0] = __builtin_fma(m13, b3, ek_sup_dm(m11, b5, m12, b4));
    adj[0][1] = -__builtin_fma(m03, b3, ek_sup_dm(m01, b5, m02, b4));
    adj[0][2] = __builtin_fma(m33, a3, ek_sup_dm(m13, a5, m23, a4));
    adj[0][3] = -__builtin_fma(m23, a3, ek_sup_dm(m12, a5, m22, a4));
    adj[1][0] = -__builtin_fma(m13, b1, ek_sup_dm(m01, b5, m12, b2));
    adj[1][1] = __builtin_fma(m03, b1, ek_sup_dm(m00, b5, m02, b2));
    adj[1][2] = -__builtin_fma(m33, a1, ek_sup_dm(m03, a5, m23, a2));
    adj[1][3] = __builtin_fma(m23, a1, ek_sup_dm(m02, a5, m22, a2));
    adj[2][0] = __builtin_fma(m13, b0, ek_sup_dm(m01, b4, m11, b2));
    adj[2][1] = -__builtin_fma(m03, b0, ek_sup_dm(m00, b4, m01, b2));
    adj[2][2] = __builtin_fma(m33, a0, ek_sup_dm(m03, a4, m13, a2));
    adj[2][3] = -__builtin_fma(m23, a0, ek_sup_dm(m02, a4, m12, a2));
    adj[3][0] = -__builtin_fma(m12, b0, ek_sup_dm(m01, b3, m11, b1));
    adj[3][1] = __builtin_fma(m02, b0, ek_sup_dm(m00, b3, m01, b1));
    adj[3][2] = -__builtin_fma(m23, a0, ek_sup_dm(m03, a3, m13, a1));
    adj[3][3] = __builtin_fma(m22, a0, ek_sup_dm(m02, a3, m12, a1));
    int best = 0;
    double n2 = 0.0;
    for (int i = 0; i < 4; ++i) {
        double v = adj[i][0] * adj[i][0];
        for (int j = 1; j < 4; ++j)
            v = __builtin_fma(adj[i][j], adj[i][j], v);
        if (v > n2) {
            n2 = v;
            best = i;
        }
    }
    if (!(n2 > 0.0))
        return 1;
    double qw = adj[0][0], qx = adj[0][1], qy = adj[0][2], qz = adj[0][3];
    for (int i = 1; i < 4; ++i)     // (a select per row: no runtime-indexed array)
        if (best == i) {
            qw = adj[i][0];
            qx = adj[i][1];
            qy = adj[i][2];
            qz = adj[i][3];
        }
    const double ww = qw * qw, xx = qx * qx, yy = qy * qy, zz = qz * qz;
    R[0] = (((ww + xx) - yy) - zz) / n2;
    R[1] = (2.0 * ek_sup_dm(qx, qy, qw, qz)) / n2;
    R[2] = (2.0 * __builtin_fma(qx, qz, qw * qy)) / n2;
    R[3] = (2.0 * __builtin_fma(qx, qy, qw * qz)) / n2;
    R[4] = (((ww - xx) + yy) - zz) / n2;
    R[5] = (2.0 * ek_sup_dm(qy, qz, qw, qx)) / n2;
    R[6] = (2.0 * ek_sup_dm(qx, qz, qw, qy)) / n2;
    R[7] = (2.0 * __builtin_fma(qy, qz, qw * qx)) / n2;
    R[8] = (((ww - xx) - yy) + zz) / n2;
    return 0;
}
