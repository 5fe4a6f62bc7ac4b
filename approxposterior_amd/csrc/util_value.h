// Acquisition utilities of the reference (utility.py:99-250) for one (mu, sigma^2): shared by the fused sweep
// (sweep.hip) and the device point search (nmsearch.hip).
#pragma once
#include "apgp_common.h"

__device__ __forceinline__ double util_value(int kind, double mu, double var, double zeta,
                                             double ybest) {
    if (kind == APGP_UTIL_AGP) {
        // utility.py:136  -(mu + 0.5*log(2*pi*e*var)); var < 0 -> NaN as in NumPy
        return -(mu + 0.5 * log(2.0 * M_PI * M_E * var));
    } else if (kind == APGP_UTIL_BAPE) {
        // utility.py:183 with logsubexp(var, 0) (utility.py:85-88):
        // var <= 0 -> -inf -> utility +inf; else var + log(1 - exp(-var))
        double lse = (var <= 0.0) ? -INFINITY : var + log(1.0 - exp(0.0 - var));
        return -((2.0 * mu + var) + lse);
    } else {
        // utility.py:229-244; std <= 0 or NaN -> 0.0
        double sd = sqrt(var);
        if (sd > 0.0) {
            double imp = mu - ybest - zeta;
            double z = imp / sd;
            double cdf = 0.5 * erfc(-z * M_SQRT1_2);
            double pdf = exp(-0.5 * z * z) * 0.3989422804014326779399461;
            return -(imp * cdf + sd * pdf);
        }
        return 0.0;
    }
}
