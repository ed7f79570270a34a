// HoNet's recovery stage (anakin/models/honetMANO.py:113-253): the hand and the object are placed in the camera frame from a predicted
// pixel-space scale / translation, the object's canonical vertices are rotated by Rodrigues of the predicted axis-angle, and every point
// is projected.  ab_honet_recover_fwd writes all of the model's geometric outputs in one launch; ab_honet_recover_bwd is the exact reverse,
// reducing the [B, N, 3] gradients to the seven numbers per sample the two TransHeads produced.
//
// Grid: (object vertex chunks + 1, B), 256 threads.  Blocks x < nco take HR_CHUNK object vertices each; the last block of a sample takes
// the 799 hand points, the 8 corners and the per-sample outputs.  Every block recomputes the sample's placement (a few dozen flops, one
// sinf / cosf pair in thread 0) instead of reading it back from another launch.
// Backward: each block reduces its HR_NSUM sums in a fixed order (per thread in vertex order, wave butterfly, waves 0..3) into its own
// row of the workspace; ab_honet_recover_bwd's second launch adds the rows in chunk order and runs the reverse of Rodrigues and of the
// placement.  No float atomics anywhere: two calls on the same inputs give the same bits.
// Memory-bound: 12 B read + 32 B written per object vertex forward, 12 B + up to 32 B of gradients read backward; a thread reads its
// vertex's three floats itself -- the three loads of a wave cover the same 768 contiguous bytes, every fetched line is used in full.
#include "mano_common.h"

#define HR_CHUNK 512
#define HR_NSUM 16          // g_centre 3 | g_R 9 | g_root 3 | pad
#define HR_NHAND (21 + NV)  // joints, then vertices

struct hr_place {           // per-sample placement, in LDS
    float K[9];
    float R[9];
    float root[3];
    float centre[3];
};

__device__ __forceinline__ void hr_centre(const float* K, float scale, float t0, float t1, float tf, float sf, float iw, float ih, float off_z,
                                          float c[3]) {
    const float f = K[0];
    const float z0 = f * (scale * sf) + off_z;
    c[0] = ((t0 * tf + iw * 0.5f) - K[2]) * z0 / f;
    c[1] = ((t1 * tf + ih * 0.5f) - K[5]) * z0 / f;
    c[2] = z0;
}

// reverse of hr_centre: gc (dL/dcentre) -> g (dL/d(scale, t0, t1))
__device__ __forceinline__ void hr_centre_bwd(const float* K, float scale, float t0, float t1, float tf, float sf, float iw, float ih, float off_z,
                                              const float gc[3], float g[3]) {
    const float f = K[0];
    const float z0 = f * (scale * sf) + off_z;
    const float a0 = (t0 * tf + iw * 0.5f) - K[2], a1 = (t1 * tf + ih * 0.5f) - K[5];
    const float gz = (gc[2] + gc[0] * (a0 / f)) + gc[1] * (a1 / f);      // Z0 directly, and through XY0
    g[0] = gz * f * sf;
    g[1] = gc[0] * (z0 / f) * tf;
    g[2] = gc[1] * (z0 / f) * tf;
}

__device__ __forceinline__ void hr_load_place(hr_place* P, const float* hand_st, int hand_pitch, const float* obj_st, int obj_pitch,
                                              const float* cam_intr, int b, float tf, float sf, float iw, float ih, float off_z) {
    if (threadIdx.x == 0) {
        const float* K = cam_intr + (size_t)b * 9;
        for (int i = 0; i < 9; ++i) P->K[i] = K[i];
        const float* h = hand_st + (size_t)b * hand_pitch;
        const float* o = obj_st + (size_t)b * obj_pitch;
        hr_centre(K, h[0], h[1], h[2], tf, sf, iw, ih, off_z, P->root);
        hr_centre(K, o[0], o[1], o[2], tf, sf, iw, ih, off_z, P->centre);
        const float a[3] = {o[3], o[4], o[5]};
        mano_rodrigues(a, P->R);
    }
    __syncthreads();
}

__device__ __forceinline__ void hr_project(const float* K, const float p[3], float uv[2]) {
    const float hx = (K[0] * p[0] + K[1] * p[1]) + K[2] * p[2];
    const float hy = (K[3] * p[0] + K[4] * p[1]) + K[5] * p[2];
    const float hz = (K[6] * p[0] + K[7] * p[1]) + K[8] * p[2];
    uv[0] = hx / hz; uv[1] = hy / hz;
}

// adds the gradient of the projection of p (g2 = dL/duv) to gp
__device__ __forceinline__ void hr_project_bwd(const float* K, const float p[3], const float g2[2], float gp[3]) {
    const float hx = (K[0] * p[0] + K[1] * p[1]) + K[2] * p[2];
    const float hy = (K[3] * p[0] + K[4] * p[1]) + K[5] * p[2];
    const float hz = (K[6] * p[0] + K[7] * p[1]) + K[8] * p[2];
    const float gx = g2[0] / hz, gy = g2[1] / hz;
    const float gz = -(g2[0] * hx + g2[1] * hy) / (hz * hz);
    gp[0] += (K[0] * gx + K[3] * gy) + K[6] * gz;
    gp[1] += (K[1] * gx + K[4] * gy) + K[7] * gz;
    gp[2] += (K[2] * gx + K[5] * gy) + K[8] * gz;
}

__device__ __forceinline__ void hr_rotate(const float* R, const float c[3], float r[3]) {
    r[0] = (R[0] * c[0] + R[1] * c[1]) + R[2] * c[2];
    r[1] = (R[3] * c[0] + R[4] * c[1]) + R[5] * c[2];
    r[2] = (R[6] * c[0] + R[7] * c[1]) + R[8] * c[2];
}

__device__ __forceinline__ void add3(const float* p, size_t i, float v[3]) {
    if (p) { v[0] += p[i * 3]; v[1] += p[i * 3 + 1]; v[2] += p[i * 3 + 2]; }
}

__global__ __launch_bounds__(256) void honet_recover_fwd_kernel(
        const float* __restrict__ hand_st, int hand_pitch, const float* __restrict__ obj_st, int obj_pitch, const float* __restrict__ cam_intr,
        const float* __restrict__ joints_3d, const float* __restrict__ hand_verts_3d, const float* __restrict__ obj_verts_can,
        const float* __restrict__ corners_can, int N, int nco, float tf, float sf, float iw, float ih, float off_z,
        float* __restrict__ root_joint, float* __restrict__ joints_3d_abs, float* __restrict__ hand_verts_3d_abs, float* __restrict__ joints_2d,
        float* __restrict__ hand_verts_2d, float* __restrict__ obj_center, float* __restrict__ rotmat, float* __restrict__ obj_verts_3d_abs,
        float* __restrict__ obj_verts_2d, float* __restrict__ corners_3d_abs, float* __restrict__ corners_2d, float* __restrict__ corners_3d,
        float* __restrict__ obj_verts_3d) {
    __shared__ hr_place P;
    const int b = blockIdx.y, tid = threadIdx.x;
    hr_load_place(&P, hand_st, hand_pitch, obj_st, obj_pitch, cam_intr, b, tf, sf, iw, ih, off_z);
    if ((int)blockIdx.x < nco) {
        const int v1 = min(N, ((int)blockIdx.x + 1) * HR_CHUNK);
        for (int v = blockIdx.x * HR_CHUNK + tid; v < v1; v += 256) {
            const size_t i = (size_t)b * N + v;
            float c[3], p[3], uv[2];
            ld3(obj_verts_can, i, c);
            hr_rotate(P.R, c, p);
            for (int k = 0; k < 3; ++k) p[k] += P.centre[k];
            hr_project(P.K, p, uv);
            st3(obj_verts_3d_abs, i, p);
            obj_verts_2d[i * 2] = uv[0]; obj_verts_2d[i * 2 + 1] = uv[1];
            if (obj_verts_3d) {
                for (int k = 0; k < 3; ++k) p[k] -= P.root[k];
                st3(obj_verts_3d, i, p);
            }
        }
        return;
    }
    if (tid < 3) { root_joint[b * 3 + tid] = P.root[tid]; obj_center[b * 3 + tid] = P.centre[tid]; }
    if (tid < 9) rotmat[b * 9 + tid] = P.R[tid];
    for (int v = tid; v < HR_NHAND; v += 256) {
        const bool jt = v < 21;
        const size_t i = jt ? (size_t)b * 21 + v : (size_t)b * NV + (v - 21);
        float p[3], uv[2];
        ld3(jt ? joints_3d : hand_verts_3d, i, p);
        for (int k = 0; k < 3; ++k) p[k] += P.root[k];
        hr_project(P.K, p, uv);
        st3(jt ? joints_3d_abs : hand_verts_3d_abs, i, p);
        float* o2 = jt ? joints_2d : hand_verts_2d;
        o2[i * 2] = uv[0]; o2[i * 2 + 1] = uv[1];
    }
    if (corners_can && tid < 8) {
        const size_t i = (size_t)b * 8 + tid;
        float c[3], p[3], uv[2];
        ld3(corners_can, i, c);
        hr_rotate(P.R, c, p);
        for (int k = 0; k < 3; ++k) p[k] += P.centre[k];
        hr_project(P.K, p, uv);
        st3(corners_3d_abs, i, p);
        corners_2d[i * 2] = uv[0]; corners_2d[i * 2 + 1] = uv[1];
        for (int k = 0; k < 3; ++k) p[k] -= P.root[k];
        st3(corners_3d, i, p);
    }
}

// block-wide sums of acc[HR_NSUM] in the fixed order -> the block's row out[HR_NSUM]
__device__ __forceinline__ void hr_block_sums(float (&acc)[HR_NSUM], float (*red)[HR_NSUM], float* out) {
    const float s = block_sum4<HR_NSUM>(acc, red);
    if (threadIdx.x < HR_NSUM) out[threadIdx.x] = s;
}

// one rotated point of the object (vertex or corner): gp = dL/d(abs point) -> the sums
__device__ __forceinline__ void hr_acc_obj(float acc[HR_NSUM], const float gp[3], const float c[3]) {
    for (int r = 0; r < 3; ++r) {
        acc[r] += gp[r];
        for (int k = 0; k < 3; ++k) acc[3 + r * 3 + k] += gp[r] * c[k];
    }
}

__global__ __launch_bounds__(256) void honet_recover_bwd_kernel(
        const float* __restrict__ hand_st, int hand_pitch, const float* __restrict__ obj_st, int obj_pitch, const float* __restrict__ cam_intr,
        const float* __restrict__ joints_3d, const float* __restrict__ hand_verts_3d, const float* __restrict__ obj_verts_can,
        const float* __restrict__ corners_can, int N, int nco, float tf, float sf, float iw, float ih, float off_z,
        const float* __restrict__ g_joints_3d_abs, const float* __restrict__ g_hand_verts_3d_abs, const float* __restrict__ g_joints_2d,
        const float* __restrict__ g_hand_verts_2d, const float* __restrict__ g_obj_verts_3d_abs, const float* __restrict__ g_obj_verts_2d,
        const float* __restrict__ g_corners_3d_abs, const float* __restrict__ g_corners_2d, const float* __restrict__ g_corners_3d,
        const float* __restrict__ g_obj_verts_3d, float* __restrict__ g_joints_3d, float* __restrict__ g_hand_verts_3d,
        float* __restrict__ partial) {
    __shared__ hr_place P;
    __shared__ float red[4][HR_NSUM];
    const int b = blockIdx.y, tid = threadIdx.x;
    hr_load_place(&P, hand_st, hand_pitch, obj_st, obj_pitch, cam_intr, b, tf, sf, iw, ih, off_z);
    float acc[HR_NSUM];
    for (int k = 0; k < HR_NSUM; ++k) acc[k] = 0.f;
    float* out = partial + ((size_t)b * (nco + 1) + blockIdx.x) * HR_NSUM;
    if ((int)blockIdx.x < nco) {
        const int v1 = min(N, ((int)blockIdx.x + 1) * HR_CHUNK);
        for (int v = blockIdx.x * HR_CHUNK + tid; v < v1; v += 256) {
            const size_t i = (size_t)b * N + v;
            float c[3], gp[3] = {0.f, 0.f, 0.f};
            ld3(obj_verts_can, i, c);
            add3(g_obj_verts_3d_abs, i, gp);
            if (g_obj_verts_3d) {
                float gr[3] = {0.f, 0.f, 0.f};
                add3(g_obj_verts_3d, i, gr);
                for (int k = 0; k < 3; ++k) { gp[k] += gr[k]; acc[12 + k] -= gr[k]; }
            }
            if (g_obj_verts_2d) {
                float p[3];
                hr_rotate(P.R, c, p);
                for (int k = 0; k < 3; ++k) p[k] += P.centre[k];
                const float g2[2] = {g_obj_verts_2d[i * 2], g_obj_verts_2d[i * 2 + 1]};
                hr_project_bwd(P.K, p, g2, gp);
            }
            hr_acc_obj(acc, gp, c);
        }
        hr_block_sums(acc, red, out);
        return;
    }
    for (int v = tid; v < HR_NHAND; v += 256) {
        const bool jt = v < 21;
        const size_t i = jt ? (size_t)b * 21 + v : (size_t)b * NV + (v - 21);
        float gp[3] = {0.f, 0.f, 0.f};
        add3(jt ? g_joints_3d_abs : g_hand_verts_3d_abs, i, gp);
        const float* g2p = jt ? g_joints_2d : g_hand_verts_2d;
        if (g2p) {
            float p[3];
            ld3(jt ? joints_3d : hand_verts_3d, i, p);
            for (int k = 0; k < 3; ++k) p[k] += P.root[k];
            const float g2[2] = {g2p[i * 2], g2p[i * 2 + 1]};
            hr_project_bwd(P.K, p, g2, gp);
        }
        st3(jt ? g_joints_3d : g_hand_verts_3d, i, gp);
        for (int k = 0; k < 3; ++k) acc[12 + k] += gp[k];
    }
    if (corners_can && tid < 8) {
        const size_t i = (size_t)b * 8 + tid;
        float c[3], gp[3] = {0.f, 0.f, 0.f};
        ld3(corners_can, i, c);
        add3(g_corners_3d_abs, i, gp);
        if (g_corners_3d) {
            float gr[3] = {0.f, 0.f, 0.f};
            add3(g_corners_3d, i, gr);
            for (int k = 0; k < 3; ++k) { gp[k] += gr[k]; acc[12 + k] -= gr[k]; }
        }
        if (g_corners_2d) {
            float p[3];
            hr_rotate(P.R, c, p);
            for (int k = 0; k < 3; ++k) p[k] += P.centre[k];
            const float g2[2] = {g_corners_2d[i * 2], g_corners_2d[i * 2 + 1]};
            hr_project_bwd(P.K, p, g2, gp);
        }
        hr_acc_obj(acc, gp, c);
    }
    hr_block_sums(acc, red, out);
}

// one thread per sample: the rows of the workspace in chunk order, then Rodrigues' and the placements' reverse
__global__ __launch_bounds__(64) void honet_recover_fin_kernel(
        const float* __restrict__ hand_st, int hand_pitch, const float* __restrict__ obj_st, int obj_pitch, const float* __restrict__ cam_intr,
        int B, int nco, float tf, float sf, float iw, float ih, float off_z, const float* __restrict__ partial,
        const float* __restrict__ g_root_joint, const float* __restrict__ g_obj_center, const float* __restrict__ g_rotmat,
        float* __restrict__ g_hand_st, int g_hand_pitch, float* __restrict__ g_obj_st, int g_obj_pitch) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float s[HR_NSUM];
    sum_rows<HR_NSUM>(partial + (size_t)b * (nco + 1) * HR_NSUM, nco + 1, s);
    float K[9];
    for (int i = 0; i < 9; ++i) K[i] = cam_intr[(size_t)b * 9 + i];
    const float* h = hand_st + (size_t)b * hand_pitch;
    const float* o = obj_st + (size_t)b * obj_pitch;
    float gc[3] = {s[0], s[1], s[2]}, gR[9], groot[3] = {s[12], s[13], s[14]};
    for (int k = 0; k < 9; ++k) gR[k] = s[3 + k] + (g_rotmat ? g_rotmat[(size_t)b * 9 + k] : 0.f);
    for (int k = 0; k < 3; ++k) {
        if (g_obj_center) gc[k] += g_obj_center[b * 3 + k];
        if (g_root_joint) groot[k] += g_root_joint[b * 3 + k];
    }
    float gh[3], go[3], ga[3];
    hr_centre_bwd(K, h[0], h[1], h[2], tf, sf, iw, ih, off_z, groot, gh);
    hr_centre_bwd(K, o[0], o[1], o[2], tf, sf, iw, ih, off_z, gc, go);
    const float a[3] = {o[3], o[4], o[5]};
    mano_rodrigues_bwd(a, gR, ga);
    float* gho = g_hand_st + (size_t)b * g_hand_pitch;
    float* goo = g_obj_st + (size_t)b * g_obj_pitch;
    for (int k = 0; k < 3; ++k) { gho[k] = gh[k]; goo[k] = go[k]; goo[3 + k] = ga[k]; }
}

extern "C" int ab_honet_recover_chunks(int N) { return N <= 0 ? 0 : (N + HR_CHUNK - 1) / HR_CHUNK; }

extern "C" long ab_honet_recover_workspace(int B, int N) {
    return (B <= 0 || N <= 0) ? 0 : (long)B * (ab_honet_recover_chunks(N) + 1) * HR_NSUM * (long)sizeof(float);
}

extern "C" int ab_honet_recover_fwd(const float* hand_st, int hand_pitch, const float* obj_st, int obj_pitch, const float* cam_intr,
                                    const float* joints_3d, const float* hand_verts_3d, const float* obj_verts_can, const float* corners_can,
                                    int B, int N, float trans_factor, float scale_factor, float img_w, float img_h, float off_z,
                                    float* root_joint, float* joints_3d_abs, float* hand_verts_3d_abs, float* joints_2d, float* hand_verts_2d,
                                    float* obj_center, float* rotmat, float* obj_verts_3d_abs, float* obj_verts_2d, float* corners_3d_abs,
                                    float* corners_2d, float* corners_3d, float* obj_verts_3d, void* stream) {
    if (B <= 0 || B > 65535 || N <= 0 || hand_pitch < 3 || obj_pitch < 6) return AB_EINVAL;
    if (!hand_st || !obj_st || !cam_intr || !joints_3d || !hand_verts_3d || !obj_verts_can || !root_joint || !joints_3d_abs ||
        !hand_verts_3d_abs || !joints_2d || !hand_verts_2d || !obj_center || !rotmat || !obj_verts_3d_abs || !obj_verts_2d) return AB_EINVAL;
    if (corners_can && (!corners_3d_abs || !corners_2d || !corners_3d)) return AB_EINVAL;
    const int nco = ab_honet_recover_chunks(N);
    honet_recover_fwd_kernel<<<dim3(nco + 1, B), 256, 0, as_stream(stream)>>>(
        hand_st, hand_pitch, obj_st, obj_pitch, cam_intr, joints_3d, hand_verts_3d, obj_verts_can, corners_can, N, nco, trans_factor,
        scale_factor, img_w, img_h, off_z, root_joint, joints_3d_abs, hand_verts_3d_abs, joints_2d, hand_verts_2d, obj_center, rotmat,
        obj_verts_3d_abs, obj_verts_2d, corners_3d_abs, corners_2d, corners_3d, obj_verts_3d);
    AB_LAUNCH_CHECK();
    return 0;
}

extern "C" int ab_honet_recover_bwd(const float* hand_st, int hand_pitch, const float* obj_st, int obj_pitch, const float* cam_intr,
                                    const float* joints_3d, const float* hand_verts_3d, const float* obj_verts_can, const float* corners_can,
                                    int B, int N, float trans_factor, float scale_factor, float img_w, float img_h, float off_z,
                                    const float* g_root_joint, const float* g_joints_3d_abs, const float* g_hand_verts_3d_abs,
                                    const float* g_joints_2d, const float* g_hand_verts_2d, const float* g_obj_center, const float* g_rotmat,
                                    const float* g_obj_verts_3d_abs, const float* g_obj_verts_2d, const float* g_corners_3d_abs,
                                    const float* g_corners_2d, const float* g_corners_3d, const float* g_obj_verts_3d, float* g_hand_st,
                                    int g_hand_pitch, float* g_obj_st, int g_obj_pitch, float* g_joints_3d, float* g_hand_verts_3d,
                                    void* workspace, void* stream) {
    if (B <= 0 || B > 65535 || N <= 0 || hand_pitch < 3 || obj_pitch < 6 || g_hand_pitch < 3 || g_obj_pitch < 6) return AB_EINVAL;
    if (!hand_st || !obj_st || !cam_intr || !joints_3d || !hand_verts_3d || !obj_verts_can || !g_hand_st || !g_obj_st || !g_joints_3d ||
        !g_hand_verts_3d || !workspace) return AB_EINVAL;
    if (!corners_can && (g_corners_3d_abs || g_corners_2d || g_corners_3d)) return AB_EINVAL;
    const int nco = ab_honet_recover_chunks(N);
    honet_recover_bwd_kernel<<<dim3(nco + 1, B), 256, 0, as_stream(stream)>>>(
        hand_st, hand_pitch, obj_st, obj_pitch, cam_intr, joints_3d, hand_verts_3d, obj_verts_can, corners_can, N, nco, trans_factor,
        scale_factor, img_w, img_h, off_z, g_joints_3d_abs, g_hand_verts_3d_abs, g_joints_2d, g_hand_verts_2d, g_obj_verts_3d_abs,
        g_obj_verts_2d, g_corners_3d_abs, g_corners_2d, g_corners_3d, g_obj_verts_3d, g_joints_3d, g_hand_verts_3d, (float*)workspace);
    AB_LAUNCH_CHECK();
    honet_recover_fin_kernel<<<(B + 63) / 64, 64, 0, as_stream(stream)>>>(
        hand_st, hand_pitch, obj_st, obj_pitch, cam_intr, B, nco, trans_factor, scale_factor, img_w, img_h, off_z, (const float*)workspace,
        g_root_joint, g_obj_center, g_rotmat, g_hand_st, g_hand_pitch, g_obj_st, g_obj_pitch);
    AB_LAUNCH_CHECK();
    return 0;
}
