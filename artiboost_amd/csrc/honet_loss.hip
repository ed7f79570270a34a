// HoNet's training step around the network, as device work a hipGraph can hold:
//   ab_mesh_queries  the three mesh queries of a synthetic batch (synth.add_mesh_queries) in one launch
//   ab_honet_loss    ManoLoss (shape / pose regularisers, joint and hand-vertex MSE) + ObjLoss (object-vertex MSE) + the per-sample joint
//                    / corner EPE + the gradient of final_loss wrt the five predictions, in one launch + a finalize pass
// Both are streaming, latency-bound kernels (a few MB at B = 64, no MFMA): they exist to replace a few hundred eager torch launches per
// step by three, not to move bytes faster.  A thread reads its point's three floats itself, as the recovery kernels do -- the three loads of
// a wave cover the same 768 contiguous bytes.
//
// ab_honet_loss, grid (object vertex chunks + 1, B), 256 threads.  Block x = 0 of a sample takes the 21 joints, the 778 hand vertices, the 8
// corners and the two regularisers; blocks x >= 1 take HL_CHUNK object vertices each.  The gradients are element-wise (no reduction); the
// squared-error sums are reduced per block in a fixed order (per thread in point order, wave butterfly, waves 0..3) into the block's own row
// of the workspace.  The finalize launch adds a sample's rows in chunk order (-> sample_part) and the samples' columns in double, lane-strided
// + butterfly, as pose_loss_finalize<1> does.  No float atomics: two calls on the same inputs give the same bits, with or without gradients.
#include "mano_common.h"

#define HL_CHUNK 512
#define HL_NSUM 8           // shape^2 | pose[3:]^2 | joints | hand verts | object verts | joint EPE mm | corner EPE mm | pad
#define MQ_CHUNK 256        // points (object vertices, then hand vertices) per block of ab_mesh_queries

struct hl_weights {
    float lam_shape, lam_pose, lam_joints, lam_hand_verts, lam_obj_verts, w_mano, w_obj;
};

// one point of an MSE term: d = pred - (targ + root); -> |d|^2, and scale * d into the gradient (scale = 2 lambda / count; targ NULL: zeros)
__device__ __forceinline__ float hl_point(const float* __restrict__ pred, const float* __restrict__ targ, const float root[3], size_t i,
                                          float* __restrict__ grad, float scale, float d[3]) {
    float sq = 0.f;
    d[0] = d[1] = d[2] = 0.f;
    if (targ) {
        float p[3], t[3];
        ld3(pred, i, p);
        ld3(targ, i, t);
        for (int k = 0; k < 3; ++k) d[k] = p[k] - (t[k] + root[k]);
        sq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    }
    if (grad) st3(grad, i, scale * d[0], scale * d[1], scale * d[2]);
    return sq;
}

__global__ __launch_bounds__(256) void honet_loss_kernel(
        const float* __restrict__ joints_3d_abs, const float* __restrict__ hand_verts_3d_abs, const float* __restrict__ obj_verts_3d_abs,
        const float* __restrict__ corners_3d_abs, const float* __restrict__ mano_pca_pose, const float* __restrict__ mano_shape,
        const float* __restrict__ root_joint, const float* __restrict__ joints_3d, const float* __restrict__ hand_verts_3d,
        const float* __restrict__ obj_verts_3d, const float* __restrict__ corners_3d, int B, int N, int ncomps, int nco, hl_weights w,
        float* __restrict__ partial, float* __restrict__ g_joints_3d_abs, float* __restrict__ g_hand_verts_3d_abs,
        float* __restrict__ g_obj_verts_3d_abs, float* __restrict__ g_mano_pca_pose, float* __restrict__ g_mano_shape) {
    __shared__ float red[4][HL_NSUM];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float root[3] = {root_joint[(size_t)b * 3], root_joint[(size_t)b * 3 + 1], root_joint[(size_t)b * 3 + 2]};
    const float Bf = (float)B;
    float* out = partial + ((size_t)b * (nco + 1) + blockIdx.x) * HL_NSUM;
    float acc[HL_NSUM];
    for (int k = 0; k < HL_NSUM; ++k) acc[k] = 0.f;
    float d[3];
    if (blockIdx.x > 0) {                                   // a chunk of the object's vertices
        const float scale = obj_verts_3d ? w.w_obj * w.lam_obj_verts * 2.f / (Bf * (float)N * 3.f) : 0.f;
        const int v0 = ((int)blockIdx.x - 1) * HL_CHUNK, v1 = min(N, v0 + HL_CHUNK);
        for (int v = v0 + tid; v < v1; v += 256)
            acc[4] += hl_point(obj_verts_3d_abs, obj_verts_3d, root, (size_t)b * N + v, g_obj_verts_3d_abs, scale, d);
    } else {                                                // the hand, the corners, the regularisers
        const float sj = joints_3d ? w.w_mano * w.lam_joints * 2.f / (Bf * 63.f) : 0.f;
        const float sv = hand_verts_3d ? w.w_mano * w.lam_hand_verts * 2.f / (Bf * (float)(NV * 3)) : 0.f;
        for (int v = tid; v < 21 + NV; v += 256) {
            if (v < 21) {
                acc[2] += hl_point(joints_3d_abs, joints_3d, root, (size_t)b * 21 + v, g_joints_3d_abs, sj, d);
                acc[5] += sqrtf(((d[0] * 1000.f) * (d[0] * 1000.f) + (d[1] * 1000.f) * (d[1] * 1000.f)) + (d[2] * 1000.f) * (d[2] * 1000.f));
            } else {
                acc[3] += hl_point(hand_verts_3d_abs, hand_verts_3d, root, (size_t)b * NV + (v - 21), g_hand_verts_3d_abs, sv, d);
            }
        }
        if (corners_3d_abs && corners_3d && tid >= 64 && tid < 72) {      // (wave 1: its lanes hold fewer hand points than wave 0's)
            hl_point(corners_3d_abs, corners_3d, root, (size_t)b * 8 + (tid - 64), nullptr, 0.f, d);
            acc[6] += sqrtf(((d[0] * 1000.f) * (d[0] * 1000.f) + (d[1] * 1000.f) * (d[1] * 1000.f)) + (d[2] * 1000.f) * (d[2] * 1000.f));
        }
        if (tid < 10) {
            const float x = mano_shape[(size_t)b * 10 + tid];
            acc[0] += x * x;
            if (g_mano_shape) g_mano_shape[(size_t)b * 10 + tid] = (w.w_mano * w.lam_shape * 2.f / (Bf * 10.f)) * x;
        }
        const int P = 3 + ncomps;
        if (tid < P) {
            const float x = tid >= 3 ? mano_pca_pose[(size_t)b * P + tid] : 0.f;      // the root rotation is not regularised
            acc[1] += x * x;
            if (g_mano_pca_pose) g_mano_pca_pose[(size_t)b * P + tid] = (w.w_mano * w.lam_pose * 2.f / (Bf * (float)ncomps)) * x;
        }
    }
    float s = block_sum4<HL_NSUM>(acc, red);
    if (tid < HL_NSUM) {
        if (tid == 5) s /= 21.f;
        if (tid == 6) s /= 8.f;
        out[tid] = s;
    }
}

// losses[8]: mano_shape, mano_pca_pose, joints_3d_loss, hand_verts_3d_loss, obj_verts_3d_loss, final_loss, mean joint EPE, mean corner EPE
__global__ __launch_bounds__(64) void honet_loss_finalize(const float* __restrict__ partial, int B, int N, int ncomps, int nco, hl_weights w,
                                                          float* __restrict__ sample_part, float* __restrict__ losses) {
    const int lane = threadIdx.x;
    double col[HL_NSUM];
    for (int c = 0; c < HL_NSUM; ++c) col[c] = 0.0;
    for (int b = lane; b < B; b += 64) {
        float s[HL_NSUM];
        sum_rows<HL_NSUM>(partial + (size_t)b * (nco + 1) * HL_NSUM, nco + 1, s);
        for (int c = 0; c < HL_NSUM; ++c) { sample_part[(size_t)b * HL_NSUM + c] = s[c]; col[c] += (double)s[c]; }
    }
#pragma unroll
    for (int c = 0; c < HL_NSUM; ++c) col[c] = wave_sum(col[c]);
    if (lane != 0) return;
    const double Bd = (double)B;
    const float ms = (float)(col[0] / (Bd * 10.0)), mp = (float)(col[1] / (Bd * (double)ncomps));
    const float mj = (float)(col[2] / (Bd * 63.0)), mv = (float)(col[3] / (Bd * (double)(NV * 3)));
    const float mo = N > 0 ? (float)(col[4] / (Bd * (double)N * 3.0)) : 0.f;
    losses[0] = ms; losses[1] = mp; losses[2] = mj; losses[3] = mv; losses[4] = mo;
    losses[5] = w.w_mano * (((w.lam_shape * ms + w.lam_pose * mp) + w.lam_joints * mj) + w.lam_hand_verts * mv) + w.w_obj * (w.lam_obj_verts * mo);
    losses[6] = (float)(col[5] / Bd);
    losses[7] = (float)(col[6] / Bd);
}

extern "C" int ab_honet_loss_chunks(int N) { return N <= 0 ? 0 : (N + HL_CHUNK - 1) / HL_CHUNK; }

extern "C" long ab_honet_loss_workspace(int B, int N) {
    return B <= 0 ? 0 : (long)B * (ab_honet_loss_chunks(N) + 1) * HL_NSUM * (long)sizeof(float);
}

extern "C" int ab_honet_loss(const float* joints_3d_abs, const float* hand_verts_3d_abs, const float* obj_verts_3d_abs,
                             const float* corners_3d_abs, const float* mano_pca_pose, const float* mano_shape, const float* root_joint,
                             const float* joints_3d, const float* hand_verts_3d, const float* obj_verts_3d, const float* corners_3d, int B,
                             int N, int ncomps, const float* weights7_host, float* sample_part, float* losses, float* g_joints_3d_abs,
                             float* g_hand_verts_3d_abs, float* g_obj_verts_3d_abs, float* g_mano_pca_pose, float* g_mano_shape,
                             void* workspace, void* stream) {
    if (B <= 0 || B > 65535 || N < 0 || ncomps < 1 || ncomps > 45) return AB_EINVAL;
    if (!joints_3d_abs || !hand_verts_3d_abs || !mano_pca_pose || !mano_shape || !root_joint || !weights7_host || !sample_part || !losses ||
        !workspace) return AB_EINVAL;
    if ((N > 0) != (obj_verts_3d_abs != nullptr)) return AB_EINVAL;                  // no object term: N = 0 and no object pointers
    if (!obj_verts_3d_abs && (obj_verts_3d || g_obj_verts_3d_abs)) return AB_EINVAL;
    if (!corners_3d_abs && corners_3d) return AB_EINVAL;
    const int nco = ab_honet_loss_chunks(N);
    hl_weights w;
    w.lam_shape = weights7_host[0]; w.lam_pose = weights7_host[1]; w.lam_joints = weights7_host[2]; w.lam_hand_verts = weights7_host[3];
    w.lam_obj_verts = weights7_host[4]; w.w_mano = weights7_host[5]; w.w_obj = weights7_host[6];
    // a term without a target does not enter final_loss (the registry losses report None for it)
    if (!joints_3d) w.lam_joints = 0.f;
    if (!hand_verts_3d) w.lam_hand_verts = 0.f;
    if (!obj_verts_3d) w.lam_obj_verts = 0.f;
    honet_loss_kernel<<<dim3(nco + 1, B), 256, 0, as_stream(stream)>>>(
        joints_3d_abs, hand_verts_3d_abs, obj_verts_3d_abs, corners_3d_abs, mano_pca_pose, mano_shape, root_joint, joints_3d, hand_verts_3d,
        obj_verts_3d, corners_3d, B, N, ncomps, nco, w, (float*)workspace, g_joints_3d_abs, g_hand_verts_3d_abs, g_obj_verts_3d_abs,
        g_mano_pca_pose, g_mano_shape);
    AB_LAUNCH_CHECK();
    honet_loss_finalize<<<1, 64, 0, as_stream(stream)>>>((const float*)workspace, B, N, ncomps, nco, w, sample_part, losses);
    AB_LAUNCH_CHECK();
    return 0;
}

// ---- the mesh queries -------------------------------------------------------------------------------------------------------------------
// grid (ceil((n + 778) / MQ_CHUNK), B), 256 threads: point p < n is object vertex p, else hand vertex p - n.  Thread 0 of a block sets up the
// sample's R | t (OBJ_TRANSF), root and rm = R . Rpose^T (Rpose: the 3x3 of the record's row-major 4x4 obj_pose) in LDS.
struct mq_place {
    float R[9], t[3], root[3], rm[9];
    long row;               // the clamped table row of the sample's object
};

__global__ __launch_bounds__(256) void mesh_queries_kernel(
        const float* __restrict__ table, int n_obj, int n, const int64_t* __restrict__ obj_id, const float* __restrict__ obj_transf,
        const float* __restrict__ root_joint, const float* __restrict__ hand_verts, const uint8_t* __restrict__ samples, long sample_pitch,
        long pose_offset, float* __restrict__ obj_verts_can, float* __restrict__ obj_verts_3d, float* __restrict__ hand_verts_3d) {
    __shared__ mq_place P;
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) {
        const float* T = obj_transf + (size_t)b * 16;
        const float* pose = (const float*)(samples + (size_t)b * sample_pitch + pose_offset);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) P.R[r * 3 + c] = T[r * 4 + c];
            P.t[r] = T[r * 4 + 3];
            P.root[r] = root_joint[(size_t)b * 3 + r];
        }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)                     // rm[r][c] = sum_k R[r][k] Rpose[c][k]
                P.rm[r * 3 + c] = (T[r * 4] * pose[c * 4] + T[r * 4 + 1] * pose[c * 4 + 1]) + T[r * 4 + 2] * pose[c * 4 + 2];
        const int64_t id = obj_id[b];
        P.row = id < 0 ? 0 : (id >= n_obj ? (long)n_obj - 1 : (long)id);      // an id outside the table is clamped into it
    }
    __syncthreads();
    const int p = blockIdx.x * MQ_CHUNK + tid;
    if (p >= n + NV) return;
    float c[3];
    if (p < n) {
        const size_t i = (size_t)b * n + p;
        ld3(table, (size_t)P.row * n + p, c);
        st3(obj_verts_can, i, c[0], c[1], c[2]);
        st3(obj_verts_3d, i,
               ((((P.R[0] * c[0] + P.R[1] * c[1]) + P.R[2] * c[2]) + P.t[0]) - P.root[0]),
               ((((P.R[3] * c[0] + P.R[4] * c[1]) + P.R[5] * c[2]) + P.t[1]) - P.root[1]),
               ((((P.R[6] * c[0] + P.R[7] * c[1]) + P.R[8] * c[2]) + P.t[2]) - P.root[2]));
    } else {
        const size_t i = (size_t)b * NV + (p - n);
        ld3(hand_verts, i, c);
        st3(hand_verts_3d, i,
               (((P.rm[0] * c[0] + P.rm[1] * c[1]) + P.rm[2] * c[2]) - P.root[0]),
               (((P.rm[3] * c[0] + P.rm[4] * c[1]) + P.rm[5] * c[2]) - P.root[1]),
               (((P.rm[6] * c[0] + P.rm[7] * c[1]) + P.rm[8] * c[2]) - P.root[2]));
    }
}

extern "C" int ab_mesh_queries(const float* table, int n_obj, int n, const int64_t* obj_id, const float* obj_transf, const float* root_joint,
                               const float* hand_verts, const uint8_t* samples, long sample_pitch, long pose_offset, int B,
                               float* obj_verts_can, float* obj_verts_3d, float* hand_verts_3d, void* stream) {
    if (B <= 0 || B > 65535 || n < 1 || n_obj < 1) return AB_EINVAL;
    if (!table || !obj_id || !obj_transf || !root_joint || !hand_verts || !samples || !obj_verts_can || !obj_verts_3d || !hand_verts_3d)
        return AB_EINVAL;
    // the pose is read in place as floats: every record's field must be 4-byte aligned and lie inside its record
    if (pose_offset < 0 || sample_pitch < pose_offset + 64 || (sample_pitch & 3) || (pose_offset & 3) || ((uintptr_t)samples & 3)) return AB_EINVAL;
    mesh_queries_kernel<<<dim3((n + NV + MQ_CHUNK - 1) / MQ_CHUNK, B), 256, 0, as_stream(stream)>>>(
        table, n_obj, n, obj_id, obj_transf, root_joint, hand_verts, samples, sample_pitch, pose_offset, obj_verts_can, obj_verts_3d,
        hand_verts_3d);
    AB_LAUNCH_CHECK();
    return 0;
}

// ---- the mesh queries of REAL frames (realdata.RealBatcher) --------------------------------------------------------
// Same launch shape as mesh_queries_kernel.  The host composes, per sample, two row-major 3x4 affine maps in float64 (realdata.real_mesh_maps):
// obj_map places the canonical object vertices, hand_map the MANO vertices of ab_mano_lbs; thread 0 of a block stages both in LDS.  A point is
// ((m0 x + m1 y) + m2 z) + m3 per row, in that order (-ffp-contract=off: no fma), so the bits do not depend on the batch or the call.
struct rmq_place {
    float obj[12], hand[12];
    long row;               // the clamped table row of the sample's object
};

__device__ __forceinline__ void rmq_apply(const float* __restrict__ m, const float c[3], float* __restrict__ dst, size_t i) {
    st3(dst, i,
           (((m[0] * c[0] + m[1] * c[1]) + m[2] * c[2]) + m[3]),
           (((m[4] * c[0] + m[5] * c[1]) + m[6] * c[2]) + m[7]),
           (((m[8] * c[0] + m[9] * c[1]) + m[10] * c[2]) + m[11]));
}

__global__ __launch_bounds__(256) void real_mesh_queries_kernel(
        const float* __restrict__ table, int n_rows, int n, const int64_t* __restrict__ row, const float* __restrict__ obj_map,
        const float* __restrict__ hand_map, const float* __restrict__ mano_verts, float* __restrict__ obj_verts_can,
        float* __restrict__ obj_verts_3d, float* __restrict__ hand_verts_3d) {
    __shared__ rmq_place P;
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) {
        for (int k = 0; k < 12; ++k) {
            P.obj[k] = obj_map[(size_t)b * 12 + k];
            P.hand[k] = hand_map[(size_t)b * 12 + k];
        }
        const int64_t id = row[b];
        P.row = id < 0 ? 0 : (id >= n_rows ? (long)n_rows - 1 : (long)id);      // a row outside the table is clamped into it
    }
    __syncthreads();
    const int p = blockIdx.x * MQ_CHUNK + tid;
    if (p >= n + NV) return;
    float c[3];
    if (p < n) {
        const size_t i = (size_t)b * n + p;
        ld3(table, (size_t)P.row * n + p, c);
        st3(obj_verts_can, i, c[0], c[1], c[2]);
        rmq_apply(P.obj, c, obj_verts_3d, i);
    } else {
        const size_t i = (size_t)b * NV + (p - n);
        ld3(mano_verts, i, c);
        rmq_apply(P.hand, c, hand_verts_3d, i);
    }
}

extern "C" int ab_real_mesh_queries(const float* table, int n_rows, int n, const int64_t* row, const float* obj_map, const float* hand_map,
                                    const float* mano_verts, int B, float* obj_verts_can, float* obj_verts_3d, float* hand_verts_3d,
                                    void* stream) {
    if (B == 0) return 0;                                   // an empty real half: nothing to write, no launch
    if (B < 0 || B > 65535 || n < 1 || n_rows < 1) return AB_EINVAL;
    if (!table || !row || !obj_map || !hand_map || !mano_verts || !obj_verts_can || !obj_verts_3d || !hand_verts_3d) return AB_EINVAL;
    real_mesh_queries_kernel<<<dim3((n + NV + MQ_CHUNK - 1) / MQ_CHUNK, B), 256, 0, as_stream(stream)>>>(
        table, n_rows, n, row, obj_map, hand_map, mano_verts, obj_verts_can, obj_verts_3d, hand_verts_3d);
    AB_LAUNCH_CHECK();
    return 0;
}
