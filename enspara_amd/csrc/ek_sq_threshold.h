// ek_sq_threshold.h -- host only: the squared-distance threshold that stands for a
// comparison of a correctly rounded square root ("No square root on the
// device"; shared by ek_dyes.hip and ek_dye_map.hip).
#pragma once
#include <math.h>

// the smallest double s >= 0 with sqrt(s) >= e
static inline double dy_sq_at_least(double e)
{
    if (!(e > 0.0))
        return 0.0;
    double s = e * e;
    while (s > 0.0 && sqrt(nextafter(s, 0.0)) >= e)
        s = nextafter(s, 0.0);
    while (sqrt(s) < e)
        s = nextafter(s, INFINITY);
    return s;
}
