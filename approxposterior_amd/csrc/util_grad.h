// Derivatives of the acquisition utilities of util_value.h with respect to (mu, sigma^2), beside the value formulas
// they differentiate: what apgp_predict_grad (predgrad.hip) chains with d mu / dt and d sigma^2 / dt.
//   AGP    u = -(mu + 0.5 log(2 pi e var))                du/dmu = -1        du/dvar = -1 / (2 var)
//   BAPE   u = -((2 mu + var) + var + log(1 - exp(-var))) du/dmu = -2        du/dvar = -(2 + 1 / expm1(var))
//   JONES  u = -(imp Phi(z) + sd phi(z)), z = imp / sd    du/dmu = -Phi(z)   du/dvar = -phi(z) / (2 sd)
//   NEG_MEAN u = -mu (+inf where mu is not finite)        du/dmu = -1        du/dvar = 0
// Where the value formula leaves its smooth branch the gradient is defined as zero (`flat`): BAPE with var <= 0
// (u = +inf), JONES with sd not > 0 (u = 0), NEG_MEAN with a non-finite mu (u = +inf).  AGP with var < 0 is NaN in value
// and gradient, as NumPy's log of a negative number makes it.
#pragma once
#include "util_value.h"

struct UtilGrad {
    double u;        // the utility (util_value's bits for AGP / BAPE / JONES)
    double dmu;      // du / dmu
    double dvar;     // du / dvar
    int flat;        // 1: the gradient is zero whatever d mu / dt and d sigma^2 / dt are (NaN included)
};

__device__ __forceinline__ UtilGrad util_grad(int kind, double mu, double var, double zeta, double ybest) {
    UtilGrad g;
    g.flat = 0;
    if (kind == APGP_UTIL_NEG_MEAN) {
        g.u = isfinite(mu) ? -mu : INFINITY;
        g.dmu = -1.0;
        g.dvar = 0.0;
        g.flat = isfinite(mu) ? 0 : 1;
        return g;
    }
    g.u = util_value(kind, mu, var, zeta, ybest);
    if (kind == APGP_UTIL_AGP) {
        g.dmu = var < 0.0 ? NAN : -1.0;
        g.dvar = var < 0.0 ? NAN : -0.5 / var;
    } else if (kind == APGP_UTIL_BAPE) {
        if (var <= 0.0) {
            g.dmu = 0.0; g.dvar = 0.0; g.flat = 1;
        } else {
            g.dmu = -2.0;
            g.dvar = -(2.0 + 1.0 / expm1(var));
        }
    } else {
        const double sd = sqrt(var);
        if (sd > 0.0) {
            const double z = (mu - ybest - zeta) / sd;
            g.dmu = -(0.5 * erfc(-z * M_SQRT1_2));
            g.dvar = -(exp(-0.5 * z * z) * 0.3989422804014326779399461) / (2.0 * sd);
        } else {
            g.dmu = 0.0; g.dvar = 0.0; g.flat = 1;
        }
    }
    return g;
}
