// The diagonal-Gaussian quadratic form, its limits and the row-block partition shared by the mixture (gmm.hip), the hidden
// Markov model's emissions (hmm.hip) and k-means' update (kmeans.hip): one definition, so no two kernels can disagree about
// the order in which a log density rounds.
#pragma once
#include "common.h"

#include <float.h>

namespace rbvae {

constexpr int DG_MAX_L = 128;                               // latent values per row at most: a row sits in registers
constexpr long DG_MAX_NK = 1L << 26;                        // resp / logb are materialised: N K f64 values, 512 MB at most
constexpr int DG_CHUNK = 4096;                              // f64 values of means and precision roots per LDS chunk (32 KB)
constexpr double DG_NK_EPS = 10.0 * DBL_EPSILON;            // scikit-learn: 10 * np.finfo(float64).eps
constexpr double DG_LOG_2PI = 1.8378770664093453;           // np.log(2 * np.pi)
constexpr int RB_THREADS = 256, RB_BLOCKS = 256;            // row blocks of a two-stage sum: 256 rows at least, 256 blocks at most

// q = sum_l ((x_l - mu_l) s_l)^2 with l ascending in groups of eight, never contracted; xi holds DG_MAX_L values (zeros
// beyond L), p holds Lp = round_up(L, 8) means and then Lp precision roots
__device__ __forceinline__ double diag_gauss_q(const float* xi, const double* p, int L, int Lp) {
#pragma clang fp contract(off)
    double q = 0.0;
#pragma unroll
    for (int l0 = 0; l0 < DG_MAX_L; l0 += 8) {
        if (l0 < L) {
#pragma unroll
            for (int l = l0; l < l0 + 8; ++l) {
                const double t = ((double)xi[l] - p[l]) * p[Lp + l];       // padding: (0 - 0) * 0 adds an exact +0
                q += t * t;
            }
        }
    }
    return q;
}

// N rows in min(ceil(N / 256), 256) blocks of row_block_rows(N) consecutive rows; the partials are added in block order
static inline int row_blocks(int N) { const int b = cdiv(N, RB_THREADS); return b < RB_BLOCKS ? b : RB_BLOCKS; }
static inline int row_block_rows(int N) { return cdiv(N, row_blocks(N)); }

}  // namespace rbvae
