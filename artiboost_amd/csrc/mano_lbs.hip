// MANO linear-blend skinning, one workgroup per hand.
// replaces manotorch.ManoLayer.forward (un-vendored third party) at its ArtiBoost call sites
//   anakin/artiboost/preprocessor.py:25,62; refiner.py:138,193,216,265; grasp_engine.py:90-95
// following the in-tree statement of the same maths, anakin/postprocess/iknet/manolayer.py:182-276 (center_idx=None,
// flat_hand_mean, axis-angle input): Rodrigues x16 -> shape blend -> joint regression -> pose blend -> 3-level
// kinematic chain -> skinning -> 21 joints (16 + 5 fingertip vertices, reordered).
// The blend tables (posedirs 1.26 MB, shapedirs 93 KB, J_regressor 50 KB, weights 50 KB) are shared by the batch
// and stay L2-resident; per hand the kernel reads 232 B and writes 9.6 KB.
//
// The regression model's MANO layer (anakin/models/mano.py:46-137 ManoBranch, hpregnet.py:75-104) with a gradient:
// ab_mano_pca_fwd takes PCA coefficients (full pose = [root | hands_mean + pca . comps]) and centres on a joint;
// ab_mano_pca_bwd recomputes the forward state in LDS (nothing is saved between the two launches) and runs the exact
// reverse of every stage.  Every reduction (over the 778 vertices, over the 2334 posed coordinates) runs in a fixed order
// through LDS -- no atomics -- so the gradient is bit-reproducible.  Exact fp32 throughout.
#include "mano_common.h"

__global__ __launch_bounds__(256) void mano_lbs_kernel(const float* __restrict__ pose, const float* __restrict__ betas,
                                                       const float* __restrict__ v_template,   // [778,3]
                                                       const float* __restrict__ shapedirs,    // [778,3,10]
                                                       const float* __restrict__ posedirs,     // [778,3,135]
                                                       const float* __restrict__ J_regressor,  // [16,778]
                                                       const float* __restrict__ weights,      // [778,16]
                                                       const float* __restrict__ hands_mean,   // [45]
                                                       float* __restrict__ verts, float* __restrict__ joints,
                                                       float* __restrict__ T_abs) {
    const int b = blockIdx.x, tid = threadIdx.x;
    __shared__ float fp[48];
    __shared__ float R[NJ][9];
    __shared__ float pmap[135];
    __shared__ float beta[10];
    __shared__ float vs[NV * 3];        // v_shaped, later v_posed
    __shared__ float J[NJ][3];
    __shared__ float G[NJ][12];         // 3x4 global transforms
    __shared__ float G2[NJ][12];        // with rest-joint removed
    __shared__ float part[256];
    if (tid < 10) beta[tid] = betas[b * 10 + tid];
    if (tid < 48) fp[tid] = pose[b * 48 + tid] + (tid >= 3 ? hands_mean[tid - 3] : 0.f);
    __syncthreads();
    mano_state(tid, fp, beta, v_template, shapedirs, posedirs, J_regressor, R, pmap, vs, J, G, G2, part);
    if (T_abs && tid < NJ * 16) {
        int j = tid / 16, k = tid % 16, r = k / 4, c = k % 4;
        T_abs[((size_t)b * NJ + j) * 16 + k] = r < 3 ? G[j][r * 4 + c] : (c == 3 ? 1.f : 0.f);
    }
    // skinning
    float* vo = verts + (size_t)b * NV * 3;
    for (int v = tid; v < NV; v += 256) {
        float T[12];
        mano_skin_T(weights, G2, v, T);
        float x = vs[v * 3], y = vs[v * 3 + 1], z = vs[v * 3 + 2];
        for (int r = 0; r < 3; ++r) vo[v * 3 + r] = ((T[r * 4] * x + T[r * 4 + 1] * y) + T[r * 4 + 2] * z) + T[r * 4 + 3];
    }
    __syncthreads();
    if (tid < 63) {
        int k = tid / 3, c = tid % 3, src = c_mano_reorder[k];
        float val = src < 16 ? G[src][c * 4 + 3] : vo[c_mano_tips[src - 16] * 3 + c];
        joints[(size_t)b * 63 + tid] = val;
    }
}

extern "C" int ab_mano_lbs(const float* pose, const float* betas, const float* v_template, const float* shapedirs,
                           const float* posedirs, const float* J_regressor, const float* weights,
                           const float* hands_mean, int B, float* verts, float* joints, float* T_abs, void* stream) {
    if (!pose || !betas || !v_template || !shapedirs || !posedirs || !J_regressor || !weights || !hands_mean || !verts || !joints)
        return AB_EINVAL;
    if (B < 1) return AB_ESHAPE;
    mano_lbs_kernel<<<B, 256, 0, as_stream(stream)>>>(pose, betas, v_template, shapedirs, posedirs, J_regressor, weights,
                                                      hands_mean, verts, joints, T_abs);
    AB_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------- PCA pose + gradient
// full[0:3] = pc[0:3];  full[3+i] = (sum_c pc[3+c] comps[c][i]) + hands_mean[i]      (ManoLayer use_pca, mano.py:96-104)
__device__ __forceinline__ void mano_full_pose(int tid, const float* __restrict__ pc, const float* __restrict__ comps,
                                               const float* __restrict__ hands_mean, int ncomps, float* fp) {
    if (tid < 3) fp[tid] = pc[tid];
    else if (tid < 48) {
        const int i = tid - 3;
        float s = 0.f;
        for (int c = 0; c < ncomps; ++c) s += pc[3 + c] * comps[c * 45 + i];
        fp[tid] = s + hands_mean[i];
    }
}

__global__ __launch_bounds__(256) void mano_pca_fwd_kernel(const float* __restrict__ pose_coeffs, const float* __restrict__ betas,
                                                           const float* __restrict__ comps, const float* __restrict__ hands_mean,
                                                           const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                                                           const float* __restrict__ posedirs, const float* __restrict__ J_regressor,
                                                           const float* __restrict__ weights, int ncomps, int center_idx,
                                                           float* __restrict__ verts, float* __restrict__ joints,
                                                           float* __restrict__ full_pose) {
    const int b = blockIdx.x, tid = threadIdx.x, P = 3 + ncomps;
    __shared__ float fp[48];
    __shared__ float R[NJ][9];
    __shared__ float pmap[135];
    __shared__ float beta[10];
    __shared__ float vs[NV * 3];
    __shared__ float vo[NV * 3];        // skinned vertices before centring
    __shared__ float J[NJ][3];
    __shared__ float G[NJ][12];
    __shared__ float G2[NJ][12];
    __shared__ float part[256];
    __shared__ float jr[63];
    if (tid < 10) beta[tid] = betas[b * 10 + tid];
    mano_full_pose(tid, pose_coeffs + (size_t)b * P, comps, hands_mean, ncomps, fp);
    __syncthreads();
    if (full_pose && tid < 48) full_pose[(size_t)b * 48 + tid] = fp[tid];
    mano_state(tid, fp, beta, v_template, shapedirs, posedirs, J_regressor, R, pmap, vs, J, G, G2, part);
    for (int v = tid; v < NV; v += 256) {
        float T[12];
        mano_skin_T(weights, G2, v, T);
        float x = vs[v * 3], y = vs[v * 3 + 1], z = vs[v * 3 + 2];
        for (int r = 0; r < 3; ++r) vo[v * 3 + r] = ((T[r * 4] * x + T[r * 4 + 1] * y) + T[r * 4 + 2] * z) + T[r * 4 + 3];
    }
    __syncthreads();
    if (tid < 63) {
        int k = tid / 3, c = tid % 3, src = c_mano_reorder[k];
        jr[tid] = src < 16 ? G[src][c * 4 + 3] : vo[c_mano_tips[src - 16] * 3 + c];
    }
    __syncthreads();
    float* vg = verts + (size_t)b * NV * 3;
    for (int i = tid; i < NV * 3; i += 256) vg[i] = center_idx >= 0 ? vo[i] - jr[center_idx * 3 + i % 3] : vo[i];
    if (tid < 63) joints[(size_t)b * 63 + tid] = center_idx >= 0 ? jr[tid] - jr[center_idx * 3 + tid % 3] : jr[tid];
}

__global__ __launch_bounds__(256) void mano_pca_bwd_kernel(const float* __restrict__ pose_coeffs, const float* __restrict__ betas,
                                                           const float* __restrict__ comps, const float* __restrict__ hands_mean,
                                                           const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                                                           const float* __restrict__ posedirs, const float* __restrict__ J_regressor,
                                                           const float* __restrict__ weights, int ncomps, int center_idx,
                                                           const float* __restrict__ g_verts, const float* __restrict__ g_joints,
                                                           const float* __restrict__ g_full_pose, float* __restrict__ g_pose_coeffs,
                                                           float* __restrict__ g_betas) {
    const int b = blockIdx.x, tid = threadIdx.x, P = 3 + ncomps;
    __shared__ float fp[48];
    __shared__ float R[NJ][9];
    __shared__ float pmap[135];
    __shared__ float beta[10];
    __shared__ float vs[NV * 3];        // v_posed (recomputed)
    __shared__ float gv[NV * 3];        // dL/d verts (uncentred, tips added)
    __shared__ float gvp[NV * 3];       // dL/d v_posed, then dL/d v_shaped
    __shared__ float J[NJ][3];
    __shared__ float G[NJ][12];
    __shared__ float G2[NJ][12];
    __shared__ float part[256];
    __shared__ float red[256][10];      // fixed-order partial sums (centring: 3, shape blend: 10)
    __shared__ float gj[63];
    __shared__ float gGt[NJ][3];        // dL/d G[:, 3] from the joint outputs
    __shared__ float gG2[NJ][12];       // dL/d G2, then dL/d G
    __shared__ float gpmap[135];
    __shared__ float gR[NJ][9];
    __shared__ float gJ[NJ][3];
    __shared__ float gfull[48];
    const float* pc = pose_coeffs + (size_t)b * P;
    if (tid < 10) beta[tid] = betas[b * 10 + tid];
    mano_full_pose(tid, pc, comps, hands_mean, ncomps, fp);
    __syncthreads();
    mano_state(tid, fp, beta, v_template, shapedirs, posedirs, J_regressor, R, pmap, vs, J, G, G2, part);

    // ---- centring: verts' = verts - c, joints' = joints - c, c = joints[center_idx]
    {
        const float* gvb = g_verts + (size_t)b * NV * 3;
        float s[3] = {0.f, 0.f, 0.f};
        for (int v = tid; v < NV; v += 256)
            for (int c = 0; c < 3; ++c) { float g = gvb[v * 3 + c]; gv[v * 3 + c] = g; s[c] += g; }
        for (int c = 0; c < 3; ++c) red[tid][c] = s[c];
        if (tid < 63) gj[tid] = g_joints[(size_t)b * 63 + tid];
    }
    __syncthreads();
    if (center_idx >= 0 && tid < 3) {
        float s = 0.f;
        for (int t = 0; t < 256; ++t) s += red[t][tid];
        for (int k = 0; k < 21; ++k) s += gj[k * 3 + tid];
        gj[center_idx * 3 + tid] -= s;
    }
    __syncthreads();
    // ---- joint reordering: 16 transform translations + 5 fingertip vertices (a permutation: every target written once)
    if (tid < 63) {
        int k = tid / 3, c = tid % 3, src = c_mano_reorder[k];
        if (src < 16) gGt[src][c] = gj[tid];
        else gv[c_mano_tips[src - 16] * 3 + c] += gj[tid];
    }
    __syncthreads();
    // ---- skinning: verts_v = T_v [v_posed_v, 1]
    //   dL/dG2_j = sum_v w_vj g_v (x) [v_posed_v, 1]   (192 outputs, each a fixed-order sum over the vertices)
    //   dL/dv_posed_v = T_v[:, :3]^T g_v
    for (int v = tid; v < NV; v += 256) {
        float T[12];
        mano_skin_T(weights, G2, v, T);
        float g0 = gv[v * 3], g1 = gv[v * 3 + 1], g2 = gv[v * 3 + 2];
        for (int c = 0; c < 3; ++c) gvp[v * 3 + c] = (T[c] * g0 + T[4 + c] * g1) + T[8 + c] * g2;
    }
    if (tid < NJ * 12) {
        const int j = tid / 12, r = (tid % 12) / 4, c = tid % 4;
        float s = 0.f;
        for (int v = 0; v < NV; ++v) {
            float w = weights[v * NJ + j];
            if (w != 0.f) s += w * gv[v * 3 + r] * (c < 3 ? vs[v * 3 + c] : 1.f);
        }
        gG2[j][r * 4 + c] = s;
    }
    __syncthreads();
    // ---- pose blend: dL/dpmap = posedirs^T dL/dv_posed (135 outputs over 2334 rows, four interleaved partial sums)
    if (tid < 135) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        const float* pd = posedirs + tid;
        int i = 0;
        for (; i + 4 <= NV * 3; i += 4) {
            s0 += pd[(size_t)i * 135] * gvp[i];
            s1 += pd[(size_t)(i + 1) * 135] * gvp[i + 1];
            s2 += pd[(size_t)(i + 2) * 135] * gvp[i + 2];
            s3 += pd[(size_t)(i + 3) * 135] * gvp[i + 3];
        }
        for (; i < NV * 3; ++i) s0 += pd[(size_t)i * 135] * gvp[i];
        gpmap[tid] = (s0 + s1) + (s2 + s3);
    }
    // ---- rest-joint correction and kinematic chain in reverse (one thread; children have larger indices than parents)
    if (tid == 255) {
        for (int j = 0; j < NJ; ++j) {
            for (int c = 0; c < 3; ++c) gJ[j][c] = 0.f;
            for (int r = 0; r < 3; ++r) {
                // G2[:, 3] = G[:, 3] - G[:, :3] J_j
                const float gt = gG2[j][r * 4 + 3];
                for (int c = 0; c < 3; ++c) {
                    gJ[j][c] -= G[j][r * 4 + c] * gt;
                    gG2[j][r * 4 + c] -= gt * J[j][c];
                }
                gG2[j][r * 4 + 3] = gt + gGt[j][r];
            }
        }
        for (int j = NJ - 1; j >= 0; --j) {
            const int par = c_mano_parents[j];
            const float* gG = gG2[j];
            float gL[12];
            if (par < 0) { for (int k = 0; k < 12; ++k) gL[k] = gG[k]; }
            else {
                // G_j = G_par L_j (3x4 affine): dL/dL_j = G_par[:, :3]^T dL/dG_j;  dL/dG_par += dL/dG_j L_j^T (+ the translation)
                const float* Pm = G[par];
                float L[12];
                for (int r = 0; r < 3; ++r) {
                    for (int c = 0; c < 3; ++c) L[r * 4 + c] = R[j][r * 3 + c];
                    L[r * 4 + 3] = J[j][r] - J[par][r];
                }
                for (int k = 0; k < 3; ++k)
                    for (int c = 0; c < 4; ++c) gL[k * 4 + c] = (Pm[k] * gG[c] + Pm[4 + k] * gG[4 + c]) + Pm[8 + k] * gG[8 + c];
                for (int r = 0; r < 3; ++r) {
                    for (int k = 0; k < 3; ++k)
                        gG2[par][r * 4 + k] += ((gG[r * 4] * L[k * 4] + gG[r * 4 + 1] * L[k * 4 + 1]) + gG[r * 4 + 2] * L[k * 4 + 2]) +
                                               gG[r * 4 + 3] * L[k * 4 + 3];
                    gG2[par][r * 4 + 3] += gG[r * 4 + 3];
                }
            }
            for (int k = 0; k < 3; ++k) {
                for (int c = 0; c < 3; ++c) gR[j][k * 3 + c] = gL[k * 4 + c];
                gJ[j][k] += gL[k * 4 + 3];               // t_0 = J_0, t_j = J_j - J_par
                if (par >= 0) gJ[par][k] -= gL[k * 4 + 3];
            }
        }
    }
    __syncthreads();
    // ---- Rodrigues (+ the pose map R_j - I of joints 1..15) -> dL/d full pose
    if (tid < NJ) {
        float g[9];
        for (int k = 0; k < 9; ++k) g[k] = gR[tid][k] + (tid > 0 ? gpmap[(tid - 1) * 9 + k] : 0.f);
        float a[3] = {fp[tid * 3], fp[tid * 3 + 1], fp[tid * 3 + 2]}, ga[3];
        mano_rodrigues_bwd(a, g, ga);
        for (int i = 0; i < 3; ++i) gfull[tid * 3 + i] = ga[i] + (g_full_pose ? g_full_pose[(size_t)b * 48 + tid * 3 + i] : 0.f);
    }
    // ---- joint regression: dL/dv_shaped = dL/dv_posed + J_regressor^T dL/dJ
    for (int i = tid; i < NV * 3; i += 256) {
        const int v = i / 3, c = i % 3;
        float s = 0.f;
        for (int j = 0; j < NJ; ++j) s += J_regressor[j * NV + v] * gJ[j][c];
        gvp[i] += s;
    }
    __syncthreads();
    // ---- shape blend: dL/dbeta = shapedirs^T dL/dv_shaped;  PCA: dL/dpc[3+c] = sum_i dL/dfull[3+i] comps[c][i]
    {
        float s[10];
        for (int l = 0; l < 10; ++l) s[l] = 0.f;
        for (int i = tid; i < NV * 3; i += 256) {
            const float* sd = shapedirs + (size_t)i * 10;
            const float g = gvp[i];
            for (int l = 0; l < 10; ++l) s[l] += sd[l] * g;
        }
        for (int l = 0; l < 10; ++l) red[tid][l] = s[l];
    }
    if (tid < P) {
        float s;
        if (tid < 3) s = gfull[tid];
        else {
            s = 0.f;
            for (int i = 0; i < 45; ++i) s += gfull[3 + i] * comps[(tid - 3) * 45 + i];
        }
        g_pose_coeffs[(size_t)b * P + tid] = s;
    }
    __syncthreads();
    if (tid < 10) {
        float s = 0.f;
        for (int t = 0; t < 256; ++t) s += red[t][tid];
        g_betas[(size_t)b * 10 + tid] = s;
    }
}

extern "C" int ab_mano_pca_fwd(const float* pose_coeffs, const float* betas, const float* comps, const float* hands_mean,
                               const float* v_template, const float* shapedirs, const float* posedirs, const float* J_regressor,
                               const float* weights, int ncomps, int center_idx, int B, float* verts, float* joints,
                               float* full_pose, void* stream) {
    if (!pose_coeffs || !betas || !comps || !hands_mean || !v_template || !shapedirs || !posedirs || !J_regressor || !weights ||
        !verts || !joints)
        return AB_EINVAL;
    if (B < 1 || ncomps < 1 || ncomps > 45 || center_idx < -1 || center_idx > 20) return AB_ESHAPE;
    mano_pca_fwd_kernel<<<B, 256, 0, as_stream(stream)>>>(pose_coeffs, betas, comps, hands_mean, v_template, shapedirs, posedirs,
                                                          J_regressor, weights, ncomps, center_idx, verts, joints, full_pose);
    AB_LAUNCH_CHECK();
    return 0;
}

extern "C" int ab_mano_pca_bwd(const float* pose_coeffs, const float* betas, const float* comps, const float* hands_mean,
                               const float* v_template, const float* shapedirs, const float* posedirs, const float* J_regressor,
                               const float* weights, int ncomps, int center_idx, int B, const float* g_verts, const float* g_joints,
                               const float* g_full_pose, float* g_pose_coeffs, float* g_betas, void* stream) {
    if (!pose_coeffs || !betas || !comps || !hands_mean || !v_template || !shapedirs || !posedirs || !J_regressor || !weights ||
        !g_verts || !g_joints || !g_pose_coeffs || !g_betas)
        return AB_EINVAL;
    if (B < 1 || ncomps < 1 || ncomps > 45 || center_idx < -1 || center_idx > 20) return AB_ESHAPE;
    mano_pca_bwd_kernel<<<B, 256, 0, as_stream(stream)>>>(pose_coeffs, betas, comps, hands_mean, v_template, shapedirs, posedirs,
                                                          J_regressor, weights, ncomps, center_idx, g_verts, g_joints, g_full_pose,
                                                          g_pose_coeffs, g_betas);
    AB_LAUNCH_CHECK();
    return 0;
}
