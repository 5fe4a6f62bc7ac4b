// The Gaussian-mixture component log-density shared by the mixture passes (gmm.hip) and the mixture proposal of the
// evidence estimate (evidence.hip): one definition, so that a proposal density and a fitted mixture's score cannot drift apart.
#pragma once
#include "apgp_common.h"

// log N(x | mu_k, Sigma_k) + log w_k through the precision Cholesky factor
template <int DP>
__device__ __forceinline__ double gmm_logpdf(const double* x, const double* P, int D) {
    const double* c = P + 2;
    const double* U = P + 2 + DP;
    double z[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) z[i] = x[i] - c[i];
    double quad = 0.0;
#pragma unroll
    for (int j = 0; j < DP; ++j) {
        double y = 0.0;
#pragma unroll
        for (int i = 0; i <= j; ++i) y = fma(z[i], U[j * (j + 1) / 2 + i], y);
        quad = fma(y, y, quad);
    }
    const double log2pi = 1.8378770664093454836;
    return (-0.5 * ((double)D * log2pi + quad) + P[1]) + P[0];
}
