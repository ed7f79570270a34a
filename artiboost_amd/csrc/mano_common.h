// MANO device code shared by mano_lbs.hip (ab_mano_lbs, ab_mano_pca_*) and mano_fit.hip (ab_mano_fit): the constants of
// the kinematic tree, Rodrigues through a quaternion and its exact reverse, the per-hand pose state (256-thread
// workgroups) and the skinning transform of one vertex.  The maths of anakin/postprocess/iknet/manolayer.py:135-276.
#pragma once
#include "common.h"

#define NV 778
#define NJ 16

static __constant__ int c_mano_parents[16] = {-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14};
static __constant__ int c_mano_tips[5] = {745, 317, 444, 556, 673};
static __constant__ int c_mano_reorder[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};

// manolayer.py:162-172 (_batch_rodrigues through a quaternion, +1e-8 inside the norm) and :135-160 (_quat2mat)
__device__ __forceinline__ void mano_rodrigues(const float a[3], float* r) {
    float e[3] = {a[0] + 1e-8f, a[1] + 1e-8f, a[2] + 1e-8f};
    float n = sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    float h = n * 0.5f, s = sinf(h), w = cosf(h);
    float x = s * (a[0] / n), y = s * (a[1] / n), z = s * (a[2] / n);
    float nq = sqrtf(((w * w + x * x) + y * y) + z * z);
    w /= nq; x /= nq; y /= nq; z /= nq;
    float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z, wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    r[0] = w2 + x2 - y2 - z2; r[1] = 2 * xy - 2 * wz; r[2] = 2 * wy + 2 * xz;
    r[3] = 2 * wz + 2 * xy; r[4] = w2 - x2 + y2 - z2; r[5] = 2 * yz - 2 * wx;
    r[6] = 2 * xz - 2 * wy; r[7] = 2 * wx + 2 * yz; r[8] = w2 - x2 - y2 + z2;
}

// reverse of mano_rodrigues: g (dL/dR, 9) -> ga (dL/da, 3), through the normalised quaternion and the +1e-8
__device__ __forceinline__ void mano_rodrigues_bwd(const float a[3], const float* g, float ga[3]) {
    float e[3] = {a[0] + 1e-8f, a[1] + 1e-8f, a[2] + 1e-8f};
    float n = sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    float h = n * 0.5f, s = sinf(h), c = cosf(h);
    float q0[4] = {c, s * (a[0] / n), s * (a[1] / n), s * (a[2] / n)};
    float nq = sqrtf(((q0[0] * q0[0] + q0[1] * q0[1]) + q0[2] * q0[2]) + q0[3] * q0[3]);
    float w = q0[0] / nq, x = q0[1] / nq, y = q0[2] / nq, z = q0[3] / nq;
    float gq[4];
    gq[0] = 2.f * (w * (g[0] + g[4] + g[8]) - z * g[1] + y * g[2] + z * g[3] - x * g[5] - y * g[6] + x * g[7]);
    gq[1] = 2.f * (x * (g[0] - g[4] - g[8]) + y * g[1] + z * g[2] + y * g[3] - w * g[5] + z * g[6] + w * g[7]);
    gq[2] = 2.f * (y * (-g[0] + g[4] - g[8]) + x * g[1] + w * g[2] + x * g[3] + z * g[5] - w * g[6] + z * g[7]);
    gq[3] = 2.f * (z * (-g[0] - g[4] + g[8]) - w * g[1] + x * g[2] + w * g[3] + y * g[5] + x * g[6] + y * g[7]);
    // q = q0 / |q0|
    float dot = ((w * gq[0] + x * gq[1]) + y * gq[2]) + z * gq[3];
    float g0[4] = {(gq[0] - w * dot) / nq, (gq[1] - x * dot) / nq, (gq[2] - y * dot) / nq, (gq[3] - z * dot) / nq};
    // q0 = (cos h, s a / n), h = n / 2, n = |a + 1e-8|
    float gs = 0.f, gn = 0.f;
    for (int i = 0; i < 3; ++i) {
        ga[i] = g0[1 + i] * (s / n);
        gs += g0[1 + i] * (a[i] / n);
        gn -= g0[1 + i] * (s * a[i] / (n * n));
    }
    gn += 0.5f * (gs * c - g0[0] * s);
    for (int i = 0; i < 3; ++i) ga[i] += gn * (e[i] / n);
}

// The pose-dependent state of one hand, shared by the kernels.  In (LDS, visible to all threads): fp[48] the full
// axis-angle pose, beta[10].  Out (LDS, visible to all threads on return): R, pmap, vs = v_posed, J, G (3x4 global
// transforms), G2 (G with the rest joint removed).  part: 256 floats of scratch.  Needs blockDim.x == 256.
__device__ __forceinline__ void mano_state(int tid, const float* fp, const float* beta, const float* __restrict__ v_template,
                                           const float* __restrict__ shapedirs, const float* __restrict__ posedirs,
                                           const float* __restrict__ J_regressor, float (*R)[9], float* pmap, float* vs,
                                           float (*J)[3], float (*G)[12], float (*G2)[12], float* part) {
    if (tid < NJ) {
        float a[3] = {fp[tid * 3], fp[tid * 3 + 1], fp[tid * 3 + 2]};
        mano_rodrigues(a, R[tid]);
    }
    // v_shaped = v_template + shapedirs . beta
    for (int i = tid; i < NV * 3; i += 256) {
        float s = v_template[i];
        const float* sd = shapedirs + (size_t)i * 10;
        for (int k = 0; k < 10; ++k) s += sd[k] * beta[k];
        vs[i] = s;
    }
    __syncthreads();
    if (tid < 135) { int j = tid / 9 + 1, k = tid % 9; pmap[tid] = R[j][k] - ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f); }
    // J = J_regressor . v_shaped   (16 x 778 x 3): 48 outputs, each reduced by 5 threads
    {
        const int o = tid / 5, l = tid % 5;      // 240 active threads
        float s = 0.f;
        if (o < 48) {
            int j = o / 3, c = o % 3;
            for (int v = l; v < NV; v += 5) s += J_regressor[j * NV + v] * vs[v * 3 + c];
        }
        part[tid] = s;
    }
    __syncthreads();
    if (tid < 48) { float s = 0.f; for (int l = 0; l < 5; ++l) s += part[tid * 5 + l]; J[tid / 3][tid % 3] = s; }
    __syncthreads();
    // v_posed = v_shaped + posedirs . pose_map
    for (int i = tid; i < NV * 3; i += 256) {
        float s = vs[i];
        const float* pd = posedirs + (size_t)i * 135;
        for (int k = 0; k < 135; ++k) s += pd[k] * pmap[k];
        vs[i] = s;
    }
    // kinematic chain (3 levels below the root; serial per finger, 5 fingers in parallel would also do)
    if (tid == 0) {
        for (int j = 0; j < NJ; ++j) {
            int par = c_mano_parents[j];
            float L[12];
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) L[r * 4 + c] = R[j][r * 3 + c];
                L[r * 4 + 3] = par < 0 ? J[0][r] : (J[j][r] - J[par][r]);
            }
            if (par < 0) { for (int k = 0; k < 12; ++k) G[j][k] = L[k]; }
            else {
                const float* P = G[par];
                for (int r = 0; r < 3; ++r) {
                    for (int c = 0; c < 4; ++c) {
                        float s = (P[r * 4] * L[c] + P[r * 4 + 1] * L[4 + c]) + P[r * 4 + 2] * L[8 + c];
                        if (c == 3) s += P[r * 4 + 3];
                        G[j][r * 4 + c] = s;
                    }
                }
            }
        }
        for (int j = 0; j < NJ; ++j)
            for (int r = 0; r < 3; ++r) {
                const float* g = G[j];
                float corr = (g[r * 4] * J[j][0] + g[r * 4 + 1] * J[j][1]) + g[r * 4 + 2] * J[j][2];
                G2[j][r * 4] = g[r * 4]; G2[j][r * 4 + 1] = g[r * 4 + 1]; G2[j][r * 4 + 2] = g[r * 4 + 2];
                G2[j][r * 4 + 3] = g[r * 4 + 3] - corr;
            }
    }
    __syncthreads();
}

// skinning transform of vertex v: T = sum_j w_vj G2_j (3x4)
__device__ __forceinline__ void mano_skin_T(const float* __restrict__ weights, const float (*G2)[12], int v, float T[12]) {
    for (int k = 0; k < 12; ++k) T[k] = 0.f;
    for (int j = 0; j < NJ; ++j) {
        float w = weights[v * NJ + j];
        if (w != 0.f) for (int k = 0; k < 12; ++k) T[k] += w * G2[j][k];
    }
}
