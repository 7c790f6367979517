// The squared distance and the neighbour order shared by project.hip (knn_k) and scores.hip: one definition, so no two
// kernels can disagree about which of two rows is nearer.
#pragma once
#include "common.h"

namespace rbvae {

// one coordinate of sum_l (a_l - b_l)^2: the difference of two f32 values is exact in f64, the square rounds once, the
// addition once (never contracted into an fma)
__device__ __forceinline__ void d2_step(double& s, double a, double b) {
#pragma clang fp contract(off)
    const double df = a - b;
    s += df * df;
}

// d2 of the query row xq (f64, L values) and the f32 row xr, l ascending
__device__ __forceinline__ double row_d2(const double* xq, const float* __restrict__ xr, int L) {
    double s = 0.0;
    for (int l = 0; l < L; ++l) d2_step(s, xq[l], (double)xr[l]);
    return s;
}

// the order of a row's neighbours: (d2, index) ascending
__device__ __forceinline__ bool key_less(double da, int ja, double db, int jb) {
    return da < db || (da == db && ja < jb);
}

}  // namespace rbvae
