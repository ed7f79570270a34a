// The similarity (Procrustes) alignment of one sample's cloud P onto X, one wave per sample: the one solve behind ab_procrustes_loss
// (csrc/mesh_align.hip) and the aligned metrics of ab_mesh_metrics (csrc/mesh_metrics.hip), which therefore agree on the aligned cloud bit
// for bit.
//
// With Xc = X - mean(X) (a root added to X cancels in the centred target: it enters the translation only), Pc = P - mean(P),
// c = |Xc|_F + 1e-8, p = |Pc|_F + 1e-8, Xh = Xc / c, Ph = Pc / p and M = Xh^T Ph = u w v^T:
//   R = u v^T (the orthogonal polar factor of M, no determinant correction: a mirrored cloud aligns by a reflection),  s = sum w,
//   aligned_i = s c R Ph_i + mean(X) + root.
// v comes from a cyclic Jacobi iteration on M^T M in registers, in its one-sided form (the columns of M V are rotated until orthogonal; the
// squared matrix is never formed, so the rotation keeps its digits in the flat direction of a hand -- a near-perfect prediction's gradient
// is a small difference that sees an error of R directly); the columns of u are M v_k, orthonormalised largest first, the last one the cross
// product with the sign of its M v_3, so a rank-deficient M (coplanar / collinear joints) gives an orthogonal R and finite numbers
// everywhere; s = sum u_k . M v_k.
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

// columns i, j of V and W = M V into descending order of the squared singular value
__device__ __forceinline__ void pr_sort2(float lam[3], float W[3][3], float V[3][3], int i, int j) {
    if (lam[i] < lam[j]) {
        float t = lam[i]; lam[i] = lam[j]; lam[j] = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t = V[k][i]; V[k][i] = V[k][j]; V[k][j] = t;
            t = W[k][i]; W[k][i] = W[k][j]; W[k][j] = t;
        }
    }
}

struct pr_fit { float mp[3], mx[3], c, p, s, R[3][3]; };                          // mean P, mean X, the two guarded norms, the scale, R = u v^T

// The fit of P [n,3] onto X [n,3] by the 64 lanes of one wave; every lane leaves with the same bits (the butterfly sums are lane-uniform).
__device__ __forceinline__ void procrustes_fit(const float* P, const float* X, int n, int lane, pr_fit& f) {
    const float inv_n = 1.f / (float)n;
    // centroids
    float *mp = f.mp, *mx = f.mx;
#pragma unroll
    for (int k = 0; k < 3; ++k) mp[k] = mx[k] = 0.f;
    for (int i = lane; i < n; i += 64)
#pragma unroll
        for (int k = 0; k < 3; ++k) { mp[k] += P[i * 3 + k]; mx[k] += X[i * 3 + k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { mp[k] = wave_sum(mp[k]) * inv_n; mx[k] = wave_sum(mx[k]) * inv_n; }
    // Frobenius norms and the raw correlation  C[a][b] = sum_i Xc_ia Pc_ib
    float pp = 0.f, xx = 0.f, C[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) C[a][k] = 0.f;
    for (int i = lane; i < n; i += 64) {
        float pc[3], xc[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { pc[k] = P[i * 3 + k] - mp[k]; xc[k] = X[i * 3 + k] - mx[k]; }
        pp += dot3(pc, pc); xx += dot3(xc, xc);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) C[a][k] = __builtin_fmaf(xc[a], pc[k], C[a][k]);
    }
    pp = wave_sum(pp); xx = wave_sum(xx);
    const float cs = sqrtf(xx) + 1e-8f, ps = sqrtf(pp) + 1e-8f;
    const float icp = 1.f / (cs * ps);
    // right singular vectors: W = M V with orthogonal columns, M = Xh^T Ph
    float W[3][3], V[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) { W[a][k] = wave_sum(C[a][k]) * icp; V[a][k] = a == k ? 1.f : 0.f; }
#pragma unroll 1
    for (int sweep = 0; sweep < PR_SWEEPS; ++sweep) { jacobi_rot(W, V, 0, 1); jacobi_rot(W, V, 0, 2); jacobi_rot(W, V, 1, 2); }
    float lam[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) lam[k] = __builtin_fmaf(W[2][k], W[2][k], __builtin_fmaf(W[1][k], W[1][k], W[0][k] * W[0][k]));
    pr_sort2(lam, W, V, 0, 1); pr_sort2(lam, W, V, 0, 2); pr_sort2(lam, W, V, 1, 2);
    // w_k = M v_k = w_k u_k; u: orthonormalised, largest first
    float w[3][3], u[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) w[k][a] = W[a][k];
    float n1 = sqrtf(dot3(w[0], w[0]));
    if (n1 > 1e-30f) { u[0][0] = w[0][0] / n1; u[0][1] = w[0][1] / n1; u[0][2] = w[0][2] / n1; }
    else { u[0][0] = 1.f; u[0][1] = 0.f; u[0][2] = 0.f; }
    float h = dot3(w[1], u[0]);
    float e[3] = {w[1][0] - h * u[0][0], w[1][1] - h * u[0][1], w[1][2] - h * u[0][2]};
    float n2 = sqrtf(dot3(e, e));
    if (!(n2 > 1e-30f)) {                                                        // rank <= 1: any unit vector orthogonal to u1
        const float a0 = fabsf(u[0][0]), a1 = fabsf(u[0][1]), a2 = fabsf(u[0][2]);
        float ax[3] = {0.f, 0.f, 0.f};
        ax[(a0 <= a1 && a0 <= a2) ? 0 : (a1 <= a2 ? 1 : 2)] = 1.f;
        h = dot3(ax, u[0]);
        e[0] = ax[0] - h * u[0][0]; e[1] = ax[1] - h * u[0][1]; e[2] = ax[2] - h * u[0][2];
        n2 = sqrtf(dot3(e, e));
    }
    u[1][0] = e[0] / n2; u[1][1] = e[1] / n2; u[1][2] = e[2] / n2;
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    if (dot3(u[2], w[2]) < 0.f) { u[2][0] = -u[2][0]; u[2][1] = -u[2][1]; u[2][2] = -u[2][2]; }     // a reflection when det M < 0
    f.c = cs; f.p = ps;
    f.s = (dot3(u[0], w[0]) + dot3(u[1], w[1])) + dot3(u[2], w[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int k = 0; k < 3; ++k) f.R[a][k] = __builtin_fmaf(u[2][a], V[k][2], __builtin_fmaf(u[1][a], V[k][1], u[0][a] * V[k][0]));
}
