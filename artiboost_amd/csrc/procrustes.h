// The 3x3 pieces of the similarity (Procrustes) alignment shared by csrc/mesh_align.hip (ab_procrustes_loss) and csrc/mesh_metrics.hip
// (ab_mesh_metrics): both solve the same problem and must agree on the aligned cloud to rounding.
#pragma once
#include "common.h"

#define PR_SWEEPS 6            // cyclic Jacobi sweeps on the symmetric 3x3: converged to rounding after 4

__device__ __forceinline__ float dot3(const float* a, const float* b) { return __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0])); }

// One rotation of the one-sided (Hestenes) Jacobi iteration: columns p, q of W = M V are rotated until they are orthogonal.  It is the
// Jacobi rotation of W^T W = V^T (M^T M) V without ever forming the squared matrix, so the small singular directions keep their digits.
__device__ __forceinline__ void jacobi_rot(float W[3][3], float V[3][3], int p, int q) {
    const float alpha = __builtin_fmaf(W[2][p], W[2][p], __builtin_fmaf(W[1][p], W[1][p], W[0][p] * W[0][p]));
    const float beta = __builtin_fmaf(W[2][q], W[2][q], __builtin_fmaf(W[1][q], W[1][q], W[0][q] * W[0][q]));
    const float gamma = __builtin_fmaf(W[2][p], W[2][q], __builtin_fmaf(W[1][p], W[1][q], W[0][p] * W[0][q]));
    if (gamma == 0.f) return;
    const float zeta = (beta - alpha) / (2.f * gamma);                           // +-inf for a vanishing inner product: t = 0 below
    float t = 1.f / (fabsf(zeta) + sqrtf(__builtin_fmaf(zeta, zeta, 1.f)));
    if (zeta < 0.f) t = -t;
    if (!(fabsf(t) <= 1.f)) return;                                              // NaN guard: leave the pair alone
    const float c = 1.f / sqrtf(__builtin_fmaf(t, t, 1.f)), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float wp = W[k][p], wq = W[k][q], vp = V[k][p], vq = V[k][q];
        W[k][p] = c * wp - s * wq; W[k][q] = s * wp + c * wq;
        V[k][p] = c * vp - s * vq; V[k][q] = s * vp + c * vq;
    }
}
