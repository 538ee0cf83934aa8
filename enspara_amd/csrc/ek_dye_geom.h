// ek_dye_geom.h -- the geometry of a donor and an acceptor conformation, the one function
// behind every k2, r and FE of the library (ek_dye_pair.hip: the pair table and the
// excitations; ek_dye_bursts.hip: the kappa-squared photons).
//
// A conformation is 9 doubles: emission centre, dipole origin, dipole vector.  r2 = |centre_D -
// centre_A|^2, r = sqrt(r2); rvec = origin_D - origin_A; cosT = A.D / (|A| |D|), cosD = rvec.D
// / (|rvec| |D|), cosA = A.rvec / (|A| |rvec|); k2 = (cosT - 3 cosD cosA)^2; R0^6 = c6 k2; r6 =
// r2 r2 r2; FE = R0^6 / (R0^6 + r6).  No root but the two norms' and r's; no sixth root.
#pragma once
#include "ek_common.h"

struct DpGeom {
    double k2, r, r06, r6, FE;
};

__device__ __forceinline__ double dp_dot(double ax, double ay, double az, double bx, double by,
                                         double bz)
{
    return ax * bx + ay * by + az * bz;
}

__device__ __forceinline__ void dp_geom(const double *__restrict__ d, const double *__restrict__ a,
                                        double c6, DpGeom &g)
{
    const double cx = d[0] - a[0], cy = d[1] - a[1], cz = d[2] - a[2];
    const double r2 = dp_dot(cx, cy, cz, cx, cy, cz);
    const double vx = d[3] - a[3], vy = d[4] - a[4], vz = d[5] - a[5];
    const double Dx = d[6], Dy = d[7], Dz = d[8], Ax = a[6], Ay = a[7], Az = a[8];
    const double nD = sqrt(dp_dot(Dx, Dy, Dz, Dx, Dy, Dz));
    const double nA = sqrt(dp_dot(Ax, Ay, Az, Ax, Ay, Az));
    const double nR = sqrt(dp_dot(vx, vy, vz, vx, vy, vz));
    const double cosT = dp_dot(Ax, Ay, Az, Dx, Dy, Dz) / (nA * nD);
    const double cosD = dp_dot(vx, vy, vz, Dx, Dy, Dz) / (nR * nD);
    const double cosA = dp_dot(Ax, Ay, Az, vx, vy, vz) / (nA * nR);
    const double k = cosT - 3.0 * cosD * cosA;
    g.k2 = k * k;
    g.r = sqrt(r2);
    g.r06 = c6 * g.k2;
    g.r6 = r2 * r2 * r2;
    g.FE = g.r06 / (g.r06 + g.r6);
}
