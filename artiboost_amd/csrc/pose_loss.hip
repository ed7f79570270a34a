// Fused pose assembly + criterion, forward AND backward, one wave per sample.
//
// replaces ~150 tiny torch kernels per step:
//   pose assembly   anakin/models/hybridbaseline.py:49-96 (batch_uvd2xyz utils/transform.py:512-546,
//                   compute_rotation_matrix_from_ortho6d utils/transform.py:578-618, corners = R*can + boxroot)
//   JointsLoss      anakin/criterions/jointloss.py:25-67      (vis-masked MSE, joints + 0.2 corners)
//   HandOrdLoss     anakin/criterions/ordinal.py:144-227      (joint-pair log(1+relu) + part-pair relu, 1+20 views)
//   SceneOrdLoss    anakin/criterions/ordinal.py:262-306      (joint-corner pairs, 1+40 views)
//   Criterion       anakin/criterions/criterion.py:57-67      (lambda-weighted sum)
//   per-sample EPE  anakin/metrics/val_metric.py:84-106       (mm, feeds the CCV re-weighting)
// and their autograd backward down to d(kp3d) and d(box6d).  The random draws (view vectors, pair subsets) are
// inputs, drawn on the host in the reference's RNG order.  Deterministic: no atomics; fixed reduction order.
#include "common.h"

#define PL_MAXPAIR 96
#define PL_MAXVIEW 48

struct PoseLossArgs {
    const float* kp3d;      // [B,22,3] uvd in [0,1)
    const float* box6d;     // [B,box_stride] first 6 valid
    int box_stride;
    const float* root_joint;   // [B,3]
    const float* cam_intr;     // [B,3,3]
    const float* corners_can;  // [B,8,3]
    const float* joints_3d;    // [B,21,3] root-relative targets
    const float* corners_3d;   // [B,8,3]
    const float* joints_vis;   // [B,21]
    const float* corners_vis;  // [B,8]
    const float* hand_views;   // [nvh,3]
    const float* scene_views;  // [nvs,3]
    const int64_t* j0; const int64_t* j1;   // [njp] joint pairs
    const int64_t* p0; const int64_t* p1;   // [npp] part pairs (indices into the 20 parts)
    const int64_t* s0; const int64_t* s1;   // [nsp] (joint, corner) pairs
    int nvh, nvs, njp, npp, nsp;
    int B, center_idx;
    float res_w, res_h, depth_range;
    float lam_joints, lam_corners;          // inside JointsLoss (1.0, 0.2)
    float lam_hand_joint, lam_hand_part, lam_scene;   // inside the ordinal losses (1,1,1)
    float w_jointsloss, w_handord, w_sceneord;        // Criterion LAMBDAS (0.5, 0.2, 0.1); 0 disables a loss
    // SymCornerLoss (symcornerloss.py:49-102): min over the object's symmetry set of the vis-masked corner MSE
    const float* sym_R;        // [nobj][symK][3][3]
    const float* sym_t;        // [nobj][symK][3]  (metres)
    const int64_t* obj_idx;    // [B] 1-based object index
    const float* obj_transf;   // [B][4][4]
    int symK;                  // 0: loss absent
    float lam_sym, w_sym;      // LAMBDA_SYM_CORNERS_3D, Criterion LAMBDA of the loss
    float* sym_loss;           // [1] output (mean over the batch)
    // outputs
    float* joints_abs;      // [B,21,3]
    float* corners_abs;     // [B,8,3]
    float* rotmat;          // [B,3,3]
    float* uvd2d;           // [B,30,3]  (2d_uvd: 21 joints uvd, 8 corners (u,v,0), boxroot uvd)
    float* sample_part;     // [B,8] per-sample loss partial sums + EPE: Lj, Lc, jo, po, so, epe_j_mm, epe_c_mm, -
    float* g_kp3d;          // [B,22,3]   (may be NULL: forward only)
    float* g_box6d;         // [B,6]
    // regression-based assembly (pose_loss_kernel<1>, ab_reg_pose_loss): kp3d = MANO's root-relative joints [B,21,3], box6d = transf rows
    // (translation 3 | 6-D rotation, pitch box_stride), g_kp3d = g_joints [B,21,3], g_box6d = g_transf (pitch box_stride)
    const float* mano_pose;    // [B,3+ncomps]
    const float* mano_shape;   // [B,10]
    int ncomps;
    float lam_shape_reg, lam_pose_reg, lam_mano_joints, w_mano;   // inside ManoLoss, and its Criterion LAMBDA
    float* g_pose;             // [B,3+ncomps]
    float* g_shape;            // [B,10]
};

// plain multiply-add, left to right (procrustes.h's dot3 is an fmaf chain: the same name, not the same arithmetic)
__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ float sgn(float x) { return (x > 0.f) ? 1.f : ((x < 0.f) ? -1.f : 0.f); }

__constant__ int c_parents[21] = {0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19};

// ---- the pose assembly of hybridbaseline.py:49-96, once for pose_loss_kernel<0>, pose_loss_kernel<1> (its corners and outputs) and
// pose_assemble_kernel.  The caller stages one sample's inputs in LDS and calls the steps on its first wave with a barrier between them:
// a `lane` of 64 or more (the other waves of the sixteen-wave kernel) takes no part in any of them.
struct PoseLds {                      // the caller's __shared__ arrays (separate arrays: each keeps the alignment the wide LDS reads want)
    const float *kp, *Kc, (*CAN)[3], *RJ;   // staged inputs: uvd predictions [66], intrinsics [9], canonical corners [8], root
    float (*P)[3], (*C)[3], (*R)[3];  // predicted abs positions (21 joints + boxroot), abs corners [8], rotation
};

// uvd -> xyz (transform.py:512-546)
__device__ __forceinline__ void uvd2xyz(const PoseLds& s, int lane, float res_w, float res_h, float depth_range) {
    const float fx = s.Kc[0], fy = s.Kc[4], cx = s.Kc[2], cy = s.Kc[5], rootz = s.RJ[2];
    if (lane < 22) {
        float u = s.kp[lane * 3], v = s.kp[lane * 3 + 1], d = s.kp[lane * 3 + 2];
        float z = (d - 0.5f) * depth_range + rootz;
        s.P[lane][0] = (u * res_w - cx) / fx * z;
        s.P[lane][1] = (v * res_h - cy) / fy * z;
        s.P[lane][2] = z;
    }
}

// ortho6d -> R (transform.py:578-618) and its reverse, one thread.  The forward leaves what the reverse needs.
struct Rot6d {
    alignas(16) float xh[3], zh[3], b[3];   // x = a / |a|, z = (x x b) / |x x b|, the second input vector
    float an, zn;                           // |a|, |x x b| (clamped)
};
__device__ __forceinline__ void rot6d_fwd(const float* a, const float* b, float (*R)[3], Rot6d& s) {
    float yh[3], zraw[3];
    float n = sqrtf(dot3(a, a)); n = fmaxf(n, 1e-8f); s.an = n;
    for (int i = 0; i < 3; ++i) { s.xh[i] = a[i] / n; s.b[i] = b[i]; }
    cross3(s.xh, b, zraw);
    float m = sqrtf(dot3(zraw, zraw)); m = fmaxf(m, 1e-8f); s.zn = m;
    for (int i = 0; i < 3; ++i) s.zh[i] = zraw[i] / m;
    cross3(s.zh, s.xh, yh);
    for (int i = 0; i < 3; ++i) { R[i][0] = s.xh[i]; R[i][1] = yh[i]; R[i][2] = s.zh[i]; }
}
// GR = dL/dR -> ga, gb = dL/d(a, b)
__device__ __forceinline__ void rot6d_bwd(const Rot6d& s, const float (*GR)[3], float* ga, float* gb) {
    float gx[3] = {GR[0][0], GR[1][0], GR[2][0]}, gy[3] = {GR[0][1], GR[1][1], GR[2][1]}, gz[3] = {GR[0][2], GR[1][2], GR[2][2]};
    float t[3];
    cross3(s.xh, gy, t); for (int i = 0; i < 3; ++i) gz[i] += t[i];        // y = z x x
    cross3(gy, s.zh, t); for (int i = 0; i < 3; ++i) gx[i] += t[i];
    float gzr[3]; float dz = dot3(s.zh, gz);
    for (int i = 0; i < 3; ++i) gzr[i] = (gz[i] - s.zh[i] * dz) / s.zn;    // z = zraw / |zraw|
    cross3(s.b, gzr, t); for (int i = 0; i < 3; ++i) gx[i] += t[i];        // zraw = x x b
    cross3(gzr, s.xh, gb);
    float dx = dot3(s.xh, gx);
    for (int i = 0; i < 3; ++i) ga[i] = (gx[i] - s.xh[i] * dx) / s.an;     // x = a / |a|
}

// corners = R * can + boxroot
__device__ __forceinline__ void box_corners(const PoseLds& s, int lane) {
    if (lane < 24) {
        int c = lane / 3, i = lane % 3;
        const float* can = s.CAN[c];
        s.C[c][i] = s.R[i][0] * can[0] + s.R[i][1] * can[1] + s.R[i][2] * can[2] + s.P[21][i];
    }
}

// what both callers write: joints_3d_abs, corners_3d_abs, box_rot_rotmat and (uvd2d may be NULL) the 2d_uvd rows
__device__ __forceinline__ void pose_write(const PoseLds& s, int lane, int b, float res_w, float res_h, float* joints_abs, float* corners_abs,
                                           float* rotmat, float* uvd2d) {
    if (lane < 63) joints_abs[(long)b * 63 + lane] = s.P[lane / 3][lane % 3];
    if (lane < 24) corners_abs[(long)b * 24 + lane] = s.C[lane / 3][lane % 3];
    if (lane < 9) rotmat[(long)b * 9 + lane] = s.R[lane / 3][lane % 3];
    if (uvd2d) {
        float* o = uvd2d + (long)b * 90;
        const float* kp = s.kp;
        if (lane < 21) { o[lane * 3] = kp[lane * 3]; o[lane * 3 + 1] = kp[lane * 3 + 1]; o[lane * 3 + 2] = kp[lane * 3 + 2]; }
        if (lane < 8) {
            const float* K = s.Kc;
            float X = s.C[lane][0], Y = s.C[lane][1], Z = s.C[lane][2];
            float hx = K[0] * X + K[1] * Y + K[2] * Z, hy = K[3] * X + K[4] * Y + K[5] * Z, hz = K[6] * X + K[7] * Y + K[8] * Z;
            o[(21 + lane) * 3] = hx / hz / res_w; o[(21 + lane) * 3 + 1] = hy / hz / res_h; o[(21 + lane) * 3 + 2] = 0.f;
        }
        if (lane < 3) o[29 * 3 + lane] = kp[21 * 3 + lane];
    }
}

// The joint-level and scene-level ordinal terms (ordinal.py:39-56 under log(1 + relu)): pair pi = (A[i0s[pi]], B[i1s[pi]]), its views spread
// over LPP lanes.  Thread t0 of the loss's wave range starts at pair t0 / LPP and steps `stride` pairs; g_pair[pi] receives the gradient
// wrt A_p - B_p (weight w included).  Returns the thread's sum of the terms.
template <int LPP>
__device__ __forceinline__ float ordinal_pairs(int t0, int stride, int npair, const uint8_t* i0s, const uint8_t* i1s, const float (*A_t)[3],
                                               const float (*B_t)[3], const float (*A_p)[3], const float (*B_p)[3], const float (*views)[3],
                                               int nv, float w, float (*g_pair)[3]) {
    const int sub = t0 & (LPP - 1);
    float sum = 0.f;
    for (int pi = t0 / LPP; pi < npair; pi += stride) {
        int i0 = (int)i0s[pi], i1 = (int)i1s[pi];
        float dt[3], dp[3], g[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < 3; ++i) { dt[i] = A_t[i0][i] - B_t[i1][i]; dp[i] = A_p[i0][i] - B_p[i1][i]; }
        for (int v = sub; v < nv; v += LPP) {
            float s = sgn(dot3(dt, views[v])), t = -s * dot3(dp, views[v]);
            if (t > 0.f) {
                sum += log1pf(t);
                float c = w * (-s) / (1.f + t);
                g[0] += c * views[v][0]; g[1] += c * views[v][1]; g[2] += c * views[v][2];
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int o = 1; o < LPP; o <<= 1) g[i] += __shfl_xor(g[i], o, 64);      // the fixed butterfly over the pair's lanes
        if (sub == 0) { g_pair[pi][0] = g[0]; g_pair[pi][1] = g[1]; g_pair[pi][2] = g[2]; }
    }
    return sum;
}

// One workgroup of sixteen waves per sample.  The short assembly phases run on wave 0 (`lane` is out of range on the other
// waves, so every `lane < N` guard excludes them).  The three ordinal losses run side by side on disjoint wave ranges with
// the views of a pair spread over 4 (hand) or 8 (scene) adjacent lanes, whose gradient partials are combined by a fixed
// butterfly; the deterministic gradient gathers split each pair list in sixteen fixed ranges, summed in wave order.  As a
// single wave the kernel was a 75 us chain of dependent LDS / transcendental latencies (~800 cycles per view).
// REG = 1: the regression-based assembly of HOPRegNet (anakin/models/hpregnet.py:112-147) in front of the same losses -- joints = MANO's
// joints + the TARGET's root, corners = R(transf[3:9]) * can + root + transf[0:3] -- plus ManoLoss (criterions/honetloss.py:12-73): the
// unmasked joint MSE per sample in sample_part[:, 7] and the gradients of the two regularisers; their sums are pose_loss_finalize<1>'s.
#define PL_WAVES 16
// the waves' partials p[w * stride], added in wave order
__device__ __forceinline__ float sum_waves(const float* p, int stride) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < PL_WAVES; ++w) s += p[w * stride];
    return s;
}
template <int REG>
__global__ __launch_bounds__(PL_WAVES * 64) void pose_loss_kernel(PoseLossArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, l64 = tid & 63;
    const int lane = wave == 0 ? tid : 1 << 20;
    __shared__ float P[22][3];        // predicted abs positions (21 joints + boxroot)
    __shared__ float C[8][3];         // predicted abs corners
    __shared__ float R[3][3], avec[3], bvec[3];
    __shared__ Rot6d rot;             // thread 0's, kept for the backward
    __shared__ float mP[21][3], mT[21][3], mC[8][3], mTC[8][3];   // vis-masked pred / target
    __shared__ float T[21][3], TC[8][3];
    __shared__ float part_p[20][3], part_t[20][3];
    __shared__ float vj[21], vc[8];
    __shared__ float hv[PL_MAXVIEW][3], sv[PL_MAXVIEW][3];
    __shared__ float gjp[PL_MAXPAIR][3];                 // gradient wrt (mP_a - mP_b) per joint pair
    __shared__ float gpp[PL_MAXPAIR][3], gpq[PL_MAXPAIR][3];   // gradient wrt part_p, part_q per part pair
    __shared__ float gsp[PL_MAXPAIR][3];                 // gradient wrt (mP_a - mC_c) per scene pair
    __shared__ float gpart[20][3];
    __shared__ float gP[22][3], gC[8][3];
    __shared__ float red[PL_WAVES][5];
    __shared__ float gpart_w[PL_WAVES][20][3], gP_w[PL_WAVES][21][3], gC_w[PL_WAVES][8][3];   // per-wave partial gathers
    // Every global input of the sample is requested in this first phase -- pair tables, view vectors, predictions and
    // targets -- with static (predicated) trip counts so the loads issue back to back and their latencies overlap: the kernel
    // is one wave per sample, and as ~30 dependent load -> wait -> use rounds it was a 75 us latency chain.
    __shared__ uint8_t ij0[PL_MAXPAIR], ij1[PL_MAXPAIR], ip0[PL_MAXPAIR], ip1[PL_MAXPAIR], is0[PL_MAXPAIR], is1[PL_MAXPAIR];
    __shared__ float kp[66], Kc[9], CAN[8][3], J3[63], C3[24], RJ[3];
    __shared__ float tvec[3];         // REG: the object's translation (transf[0:3])
    const PoseLds ps = {kp, Kc, CAN, RJ, P, C, R};
    float r_pose = 0.f, r_shape = 0.f;
    // unconditional loads (index clamped, absent tables redirected to a valid address), conditional LDS writes: branches
    // around the loads would put each one in its own basic block with its own s_waitcnt
    if (wave == 0) {
    const void* any = a.kp3d;
    auto ld = [&](auto* p, int i, int n) { p = n > 0 ? p : (decltype(p))any; return p[i < n ? i : 0]; };
    int64_t rj0[2], rj1[2], rp0[2], rp1[2], rs0[2], rs1[2];
    float rhv[3], rsv[3];
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int i = lane + it * 64;
        rj0[it] = ld(a.j0, i, a.njp); rj1[it] = ld(a.j1, i, a.njp);
        rp0[it] = ld(a.p0, i, a.npp); rp1[it] = ld(a.p1, i, a.npp);
        rs0[it] = ld(a.s0, i, a.nsp); rs1[it] = ld(a.s1, i, a.nsp);
    }
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        const int i = lane + it * 64;
        rhv[it] = ld(a.hand_views, i, a.nvh * 3); rsv[it] = ld(a.scene_views, i, a.nvs * 3);
    }
    const float r_kp = REG ? a.kp3d[(long)b * 63 + (lane < 63 ? lane : 0)] : a.kp3d[(long)b * 66 + lane];
    const float r_kp2 = REG ? 0.f : a.kp3d[(long)b * 66 + 64 + (lane & 1)];
    const float r_K = a.cam_intr[(long)b * 9 + (lane < 9 ? lane : 0)];
    const int l24 = lane < 24 ? lane : 0;
    const float r_can = a.corners_can[(long)b * 24 + l24], r_c3 = a.corners_3d[(long)b * 24 + l24];
    const float r_j3 = a.joints_3d[(long)b * 63 + (lane < 63 ? lane : 0)];
    const float r_rj = a.root_joint[b * 3 + (lane < 3 ? lane : 0)];
    const float r_vj = a.joints_vis[b * 21 + (lane < 21 ? lane : 0)], r_vc = a.corners_vis[b * 8 + (lane & 7)];
    const float r_box = a.box6d[(long)b * a.box_stride + (lane < (REG ? 9 : 6) ? lane : 0)];
    if constexpr (REG) {
        const int P_ = 3 + a.ncomps;
        r_pose = a.mano_pose[(long)b * P_ + (lane < P_ ? lane : 0)];
        r_shape = a.mano_shape[(long)b * 10 + (lane < 10 ? lane : 0)];
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int i = lane + it * 64;
        if (i < a.njp) { ij0[i] = (uint8_t)rj0[it]; ij1[i] = (uint8_t)rj1[it]; }
        if (i < a.npp) { ip0[i] = (uint8_t)rp0[it]; ip1[i] = (uint8_t)rp1[it]; }
        if (i < a.nsp) { is0[i] = (uint8_t)rs0[it]; is1[i] = (uint8_t)rs1[it]; }
    }
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        const int i = lane + it * 64;
        if (i < a.nvh * 3) (&hv[0][0])[i] = rhv[it];
        if (i < a.nvs * 3) (&sv[0][0])[i] = rsv[it];
    }
    kp[lane] = r_kp;
    if (lane < 2) kp[64 + lane] = r_kp2;
    if (lane < 9) Kc[lane] = r_K;
    if (lane < 24) { (&CAN[0][0])[lane] = r_can; C3[lane] = r_c3; }
    if (lane < 63) J3[lane] = r_j3;
    if constexpr (REG) {
        if (lane < 3) { RJ[lane] = r_rj; tvec[lane] = r_box; }
        else if (lane < 6) avec[lane - 3] = r_box;
        else if (lane < 9) bvec[lane - 6] = r_box;
    } else {
        if (lane < 3) { RJ[lane] = r_rj; avec[lane] = r_box; }
        else if (lane < 6) bvec[lane - 3] = r_box;
    }
    if (lane < 21) vj[lane] = r_vj;
    if (lane < 8) vc[lane] = r_vc;
    }
    __syncthreads();
    if constexpr (REG) {      // hpregnet.py:112-147: joints + the target's root; P[21] = the object's centre
        if (lane < 63) P[lane / 3][lane % 3] = kp[lane] + RJ[lane % 3];
        if (lane < 3) P[21][lane] = RJ[lane] + tvec[lane];
    } else {
        uvd2xyz(ps, lane, a.res_w, a.res_h, a.depth_range);
    }
    if (lane == 0) rot6d_fwd(avec, bvec, R, rot);
    __syncthreads();
    box_corners(ps, lane);
    if (lane < 63) {
        int k = lane / 3, i = lane % 3;
        float t = J3[k * 3 + i] + RJ[i];
        T[k][i] = t; mT[k][i] = t * vj[k]; mP[k][i] = P[k][i] * vj[k];
    }
    __syncthreads();
    if (lane < 24) {
        int c = lane / 3, i = lane % 3;
        float t = C3[c * 3 + i] + RJ[i];
        TC[c][i] = t; mTC[c][i] = t * vc[c]; mC[c][i] = C[c][i] * vc[c];
    }
    if (lane < 60) {
        int k = lane / 3 + 1, i = lane % 3;
        part_p[k - 1][i] = mP[k][i] - mP[c_parents[k]][i];
        part_t[k - 1][i] = mT[k][i] - mT[c_parents[k]][i];
    }
    __syncthreads();
    pose_write(ps, lane, b, a.res_w, a.res_h, a.joints_abs, a.corners_abs, a.rotmat, a.uvd2d);
    // ---- losses: per-lane partial sums   [Lj, Lc, jo, po, so]
    float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const float B_ = (float)a.B;
    const float nJ = B_ * 63.f, nC = B_ * 24.f;
    const float nJO = B_ * a.njp * a.nvh, nPO = B_ * a.npp * a.nvh, nSO = B_ * a.nsp * a.nvs;
    if (lane < 63) { float d = mP[lane / 3][lane % 3] - mT[lane / 3][lane % 3]; acc[0] = d * d; }
    if (lane < 24) { float d = mC[lane / 3][lane % 3] - mTC[lane / 3][lane % 3]; acc[1] = d * d; }
    // wave ranges of the three losses: 16 joint / part pairs or 8 scene pairs per wave when that fits, else a fixed split
    int wj = (a.njp + 15) / 16, wp = (a.npp + 15) / 16, ws = (a.nsp + 7) / 8;
    if (wj + wp + ws > PL_WAVES) { wj = 5; wp = 4; ws = PL_WAVES - 9; }
    const float wjo = a.w_handord * a.lam_hand_joint / nJO;
    const float wpo = a.w_handord * a.lam_hand_part / nPO;
    const float wso = a.w_sceneord * a.lam_scene / nSO;
    if (wave < wj) {                                    // joint-level ordinal: 4 lanes per pair
        acc[2] = ordinal_pairs<4>(tid, wj * 16, a.njp, ij0, ij1, mT, mT, mP, mP, hv, a.nvh, wjo, gjp);
    } else if (wave < wj + wp) {                        // part-level ordinal: 4 lanes per pair
        const int t0 = tid - wj * 64, sub = t0 & 3;
        for (int pi = t0 >> 2; pi < a.npp; pi += wp * 16) {
            int i0 = (int)ip0[pi], i1 = (int)ip1[pi];
            float ct[3], cp[3], gp[3] = {0.f, 0.f, 0.f}, gq[3] = {0.f, 0.f, 0.f};
            cross3(part_t[i0], part_t[i1], ct);
            cross3(part_p[i0], part_p[i1], cp);
            for (int v = sub; v < a.nvh; v += 4) {
                float s = sgn(dot3(ct, hv[v])), t = -s * dot3(cp, hv[v]);
                if (t > 0.f) {
                    acc[3] += t;
                    float c = wpo * (-s);
                    float qn[3], np_[3];
                    cross3(part_p[i1], hv[v], qn);       // d((p x q).n)/dp = q x n
                    cross3(hv[v], part_p[i0], np_);      // d((p x q).n)/dq = n x p
                    for (int i = 0; i < 3; ++i) { gp[i] += c * qn[i]; gq[i] += c * np_[i]; }
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                gp[i] += __shfl_xor(gp[i], 1, 64); gp[i] += __shfl_xor(gp[i], 2, 64);
                gq[i] += __shfl_xor(gq[i], 1, 64); gq[i] += __shfl_xor(gq[i], 2, 64);
            }
            if (sub == 0) for (int i = 0; i < 3; ++i) { gpp[pi][i] = gp[i]; gpq[pi][i] = gq[i]; }
        }
    } else if (wave < wj + wp + ws) {                   // scene ordinal: 8 lanes per pair
        acc[4] = ordinal_pairs<8>(tid - (wj + wp) * 64, ws * 8, a.nsp, is0, is1, mT, mTC, mP, mC, sv, a.nvs, wso, gsp);
    }
    // ---- SymCornerLoss: lanes scan the symmetry set, wave arg-min (ties -> lowest k), gradient from the winner only
    __shared__ float gsym[8][3];
    if (lane < 24) gsym[lane / 3][lane % 3] = 0.f;
    if (a.symK > 0) {
        const long obj = (long)a.obj_idx[b] - 1;
        const float* Tm = a.obj_transf + (long)b * 16;
        auto sym_gt = [&](int k, int c, float* gt) {           // vis-masked transformed canonical corner c under symmetry k
            const float* Rk = a.sym_R + (obj * a.symK + k) * 9;
            const float* tk = a.sym_t + (obj * a.symK + k) * 3;
            const float* can = CAN[c];
            float sc[3];
            for (int i = 0; i < 3; ++i) sc[i] = (Rk[i * 3] * can[0] + Rk[i * 3 + 1] * can[1] + Rk[i * 3 + 2] * can[2]) + tk[i];
            for (int i = 0; i < 3; ++i) gt[i] = ((Tm[i * 4] * sc[0] + Tm[i * 4 + 1] * sc[1] + Tm[i * 4 + 2] * sc[2]) + Tm[i * 4 + 3]) * vc[c];
        };
        float best = INFINITY; int bk = 0x7fffffff;
        for (int k = lane; k < a.symK; k += 64) {
            float e = 0.f;
#pragma unroll 1
            for (int c = 0; c < 8; ++c) {
                float gt[3]; sym_gt(k, c, gt);
                float per = 0.f;
                for (int i = 0; i < 3; ++i) { float d = gt[i] - mC[c][i]; per += d * d; }
                e += per / 3.f;                                 // .mean(-1) over xyz, then .mean(-1) over corners
            }
            e /= 8.f;
            if (e < best) { best = e; bk = k; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            float ob = __shfl_xor(best, o, 64); int ok = __shfl_xor(bk, o, 64);
            if (ob < best || (ob == best && ok < bk)) { best = ob; bk = ok; }
        }
        if (lane == 0) a.sample_part[(long)b * 8 + 7] = best;
        if (lane < 8 && a.g_kp3d) {
            float gt[3]; sym_gt(bk, lane, gt);
            const float wS = a.w_sym * a.lam_sym * 2.f / (24.f * B_);
            for (int i = 0; i < 3; ++i) gsym[lane][i] = wS * (mC[lane][i] - gt[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const float v = wave_sum(acc[i]);
        if (l64 == 0) red[wave][i] = v;
    }
    __syncthreads();
    if (lane < 5) a.sample_part[(long)b * 8 + lane] = sum_waves(&red[0][lane], 5);
    auto epe_mm = [](const float (*A)[3], const float (*B)[3], int n) {      // per-sample EPE in mm (unmasked, absolute), val_metric.py:96-104
        float s = 0.f;
        for (int k = 0; k < n; ++k) { float d[3] = {A[k][0] - B[k][0], A[k][1] - B[k][1], A[k][2] - B[k][2]}; s += sqrtf(dot3(d, d)); }
        return s / (float)n * 1000.f;
    };
    if (lane == 5) a.sample_part[(long)b * 8 + 5] = epe_mm(P, T, 21);
    if (lane == 6) a.sample_part[(long)b * 8 + 6] = epe_mm(C, TC, 8);
    if constexpr (REG) {      // ManoLoss's joint term: unmasked squared error of the sample (honetloss.py:49-53)
        if (wave == 0) {
            const float d = l64 < 63 ? P[l64 / 3][l64 % 3] - T[l64 / 3][l64 % 3] : 0.f;
            const float v = wave_sum(d * d);
            if (l64 == 0) a.sample_part[(long)b * 8 + 7] = v;
        }
    }
    if (!a.g_kp3d) return;
    // ---- backward, deterministic gather
    // every wave scans its sixteenth of each pair list, branch-free (selects, so the LDS loads pipeline); partials are summed
    // in wave order
    const int qpp = (a.npp + PL_WAVES - 1) / PL_WAVES, qjp = (a.njp + PL_WAVES - 1) / PL_WAVES, qsp = (a.nsp + PL_WAVES - 1) / PL_WAVES;
    if (l64 < 60) {      // part gradients: gpart[k] = sum over part pairs containing k
        int k = l64 / 3, i = l64 % 3;
        float s = 0.f;
        for (int pi = wave * qpp; pi < min((wave + 1) * qpp, a.npp); ++pi) {
            const float u = gpp[pi][i], w = gpq[pi][i];
            s += ((int)ip0[pi] == k ? u : 0.f) + ((int)ip1[pi] == k ? w : 0.f);
        }
        gpart_w[wave][k][i] = s;
    }
    if (l64 < 63) {
        int k = l64 / 3, i = l64 % 3;
        float s = 0.f;
        for (int pi = wave * qjp; pi < min((wave + 1) * qjp, a.njp); ++pi) {
            const float u = gjp[pi][i];
            s += ((int)ij0[pi] == k ? u : 0.f) - ((int)ij1[pi] == k ? u : 0.f);
        }
        for (int pi = wave * qsp; pi < min((wave + 1) * qsp, a.nsp); ++pi) s += ((int)is0[pi] == k ? gsp[pi][i] : 0.f);
        gP_w[wave][k][i] = s;
    }
    if (l64 < 24) {
        int c = l64 / 3, i = l64 % 3;
        float s = 0.f;
        for (int pi = wave * qsp; pi < min((wave + 1) * qsp, a.nsp); ++pi) s -= ((int)is1[pi] == c ? gsp[pi][i] : 0.f);
        gC_w[wave][c][i] = s;
    }
    __syncthreads();
    if (lane < 60) (&gpart[0][0])[lane] = sum_waves(&gpart_w[0][0][0] + lane, 60);
    __syncthreads();
    const float wJ = a.w_jointsloss * a.lam_joints * 2.f / nJ, wC = a.w_jointsloss * a.lam_corners * 2.f / nC;
    if (lane < 63) {      // gradient wrt masked joint mP[k][i], then * vis
        int k = lane / 3, i = lane % 3;
        float s = sum_waves(&gP_w[0][k][i], 63);
        s += wJ * (mP[k][i] - mT[k][i]);
        if (k >= 1) s += gpart[k - 1][i];
        for (int c = 1; c < 21; ++c) if (c_parents[c] == k) s -= gpart[c - 1][i];
        gP[k][i] = s * vj[k];
        if constexpr (REG) gP[k][i] += a.w_mano * a.lam_mano_joints * 2.f / nJ * (P[k][i] - T[k][i]);
    }
    if (lane < 24) {
        int c = lane / 3, i = lane % 3;
        float s = sum_waves(&gC_w[0][c][i], 24);
        s += wC * (mC[c][i] - mTC[c][i]) + gsym[c][i];
        gC[c][i] = s * vc[c];
    }
    __syncthreads();
    if (lane < 3) {      // boxroot receives every corner gradient
        float s = 0.f;
        for (int c = 0; c < 8; ++c) s += gC[c][lane];
        gP[21][lane] = s;
    }
    __syncthreads();
    if constexpr (REG) {
        const int P_ = 3 + a.ncomps;
        if (lane < 63) a.g_kp3d[(long)b * 63 + lane] = gP[lane / 3][lane % 3];       // joints_3d_abs = joints_3d + root
        if (lane < 3) a.g_box6d[(long)b * a.box_stride + lane] = gP[21][lane];       // centre = root + transf[0:3]
        if (lane < P_) a.g_pose[(long)b * P_ + lane] = lane < 3 ? 0.f : a.w_mano * a.lam_pose_reg * 2.f / (B_ * (float)a.ncomps) * r_pose;
        if (lane < 10) a.g_shape[(long)b * 10 + lane] = a.w_mano * a.lam_shape_reg * 2.f / (B_ * 10.f) * r_shape;
    } else if (lane < 22) {     // xyz -> uvd
        const float fx = Kc[0], fy = Kc[4], cx = Kc[2], cy = Kc[5];
        float u = kp[lane * 3], v = kp[lane * 3 + 1];
        float z = P[lane][2];
        float gx = gP[lane][0], gy = gP[lane][1], gz = gP[lane][2];
        float* o = a.g_kp3d + (long)b * 66 + lane * 3;
        o[0] = gx * a.res_w / fx * z;
        o[1] = gy * a.res_h / fy * z;
        o[2] = a.depth_range * (gx * (u * a.res_w - cx) / fx + gy * (v * a.res_h - cy) / fy + gz);
    }
    if (lane == 0) {     // R -> 6D
        float GR[3][3];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) {
            float s = 0.f;
            for (int c = 0; c < 8; ++c) s += gC[c][i] * CAN[c][j];
            GR[i][j] = s;
        }
        float ga[3], gb[3];
        rot6d_bwd(rot, GR, ga, gb);
        float* o = REG ? a.g_box6d + (long)b * a.box_stride + 3 : a.g_box6d + (long)b * 6;
        o[0] = ga[0]; o[1] = ga[1]; o[2] = ga[2]; o[3] = gb[0]; o[4] = gb[1]; o[5] = gb[2];
    }
}

// losses[8]: joints_3d_loss, corners_3d_loss, joint_ord_loss, part_ord_loss, scene_ord_loss, final_loss, mean epe_j, mean epe_c
// REG: losses[16], + [8] mano_shape, [9] mano_pca_pose, [10] ManoLoss's joints_3d_loss, [11] joints_loss_output, [12] hand_ord_loss_output
template <int REG>
__global__ __launch_bounds__(64) void pose_loss_finalize(const float* __restrict__ sample_part, PoseLossArgs a, float* __restrict__ losses) {
    const int lane = threadIdx.x;
    // column sums over the batch in double: lane-strided partials (independent loads), then a butterfly in fixed order
    double col[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        double s = 0.0;
        for (int b = lane; b < a.B; b += 64) s += (double)sample_part[(long)b * 8 + c];
        col[c] = wave_sum(s);
    }
    double reg_s = 0.0, reg_p = 0.0;
    if constexpr (REG) {      // the two regularisers: mean(shape^2), mean(pose[:, 3:]^2), same fixed order
        const int P_ = 3 + a.ncomps;
        for (int i = lane; i < a.B * 10; i += 64) { const double x = (double)a.mano_shape[i]; reg_s += x * x; }
        for (int i = lane; i < a.B * P_; i += 64) { const double x = (i % P_) >= 3 ? (double)a.mano_pose[i] : 0.0; reg_p += x * x; }
        reg_s = wave_sum(reg_s); reg_p = wave_sum(reg_p);
    }
    if (lane != 0) return;
    const float B_ = (float)a.B;
    float v[7];
    v[0] = (float)(col[0] / (B_ * 63.f));
    v[1] = (float)(col[1] / (B_ * 24.f));
    v[2] = (float)(col[2] / (B_ * a.njp * a.nvh));
    v[3] = (float)(col[3] / (B_ * a.npp * a.nvh));
    v[4] = (float)(col[4] / (B_ * a.nsp * a.nvs));
    v[5] = (float)(col[5] / B_);
    v[6] = (float)(col[6] / B_);
    float symv = 0.f;
    if (a.symK > 0) {
        symv = (float)(col[7] / (double)a.B);
        if (a.sym_loss) a.sym_loss[0] = symv;
    }
    for (int i = 0; i < 5; ++i) losses[i] = v[i];
    losses[6] = v[5]; losses[7] = v[6];
    losses[5] = a.w_jointsloss * (a.lam_joints * v[0] + a.lam_corners * v[1]) +
                a.w_handord * (a.lam_hand_joint * v[2] + a.lam_hand_part * v[3]) +
                a.w_sceneord * (a.lam_scene * v[4]) + a.w_sym * (a.lam_sym * symv);
    if constexpr (REG) {
        const float ms = (float)(reg_s / (double)(B_ * 10.f)), mp = (float)(reg_p / (double)(B_ * (float)a.ncomps));
        const float mj = (float)(col[7] / (double)(B_ * 63.f));
        losses[8] = ms; losses[9] = mp; losses[10] = mj;
        losses[11] = a.lam_joints * v[0] + a.lam_corners * v[1];
        losses[12] = a.lam_hand_joint * v[2] + a.lam_hand_part * v[3];
        losses[13] = losses[14] = losses[15] = 0.f;
        losses[5] += a.w_mano * (a.lam_shape_reg * ms + a.lam_pose_reg * mp + a.lam_mano_joints * mj);
    }
}

// The fields both criteria set.  w: the first six entries of either weight table.  An ordinal loss the caller found absent (hand / scene
// false) keeps NULL tables and zero counts, which is how the kernel knows it.
static PoseLossArgs pl_args(const float* kp3d, const float* box6d, int box_stride, const float* root_joint, const float* cam_intr,
                            const float* corners_can, const float* joints_3d, const float* corners_3d, const float* joints_vis,
                            const float* corners_vis, bool hand, const float* hand_views, int nvh, const int64_t* j0, const int64_t* j1,
                            int njp, const int64_t* p0, const int64_t* p1, int npp, bool scene, const float* scene_views, int nvs,
                            const int64_t* s0, const int64_t* s1, int nsp, int B, const float* w, float* joints_abs, float* corners_abs,
                            float* rotmat, float* sample_part, float* g_kp3d, float* g_box6d) {
    PoseLossArgs a = {};
    a.kp3d = kp3d; a.box6d = box6d; a.box_stride = box_stride; a.root_joint = root_joint; a.cam_intr = cam_intr;
    a.corners_can = corners_can; a.joints_3d = joints_3d; a.corners_3d = corners_3d; a.joints_vis = joints_vis; a.corners_vis = corners_vis;
    if (hand) { a.hand_views = hand_views; a.j0 = j0; a.j1 = j1; a.p0 = p0; a.p1 = p1; a.nvh = nvh; a.njp = njp; a.npp = npp; }
    if (scene) { a.scene_views = scene_views; a.s0 = s0; a.s1 = s1; a.nvs = nvs; a.nsp = nsp; }
    a.B = B; a.depth_range = 0.4f;
    a.lam_joints = w[0]; a.lam_corners = w[1]; a.lam_hand_joint = w[2]; a.lam_hand_part = w[3]; a.lam_scene = w[4]; a.w_jointsloss = w[5];
    a.joints_abs = joints_abs; a.corners_abs = corners_abs; a.rotmat = rotmat; a.sample_part = sample_part;
    a.g_kp3d = g_kp3d; a.g_box6d = g_box6d;
    return a;
}

// The kernel, then the finalize pass on a copy whose normalisers of absent losses are guarded.  The two criteria's guards differ and both
// are kept: the classification-based one replaces all of a loss's counts when its first pair list is empty (an empty part list beside a
// non-empty joint list is left alone), the regression-based one every zero count on its own (a present loss may have no pairs).
template <int REG>
static int pl_run(const PoseLossArgs& a, float* losses, void* stream) {
    pose_loss_kernel<REG><<<a.B, PL_WAVES * 64, 0, as_stream(stream)>>>(a);
    AB_LAUNCH_CHECK();
    PoseLossArgs f = a;
    if (REG) {
        for (int* n : {&f.njp, &f.npp, &f.nvh, &f.nsp, &f.nvs}) *n = *n ? *n : 1;
    } else {
        if (f.njp == 0) { f.njp = 1; f.npp = 1; f.nvh = 1; }
        if (f.nsp == 0) { f.nsp = 1; f.nvs = 1; }
    }
    pose_loss_finalize<REG><<<1, 64, 0, as_stream(stream)>>>(a.sample_part, f, losses);
    AB_LAUNCH_CHECK();
    return 0;
}

// ---- M4 alone (eval-mode forwards: no targets, no criterion): hybridbaseline.py:49-96 for one sample per wave -- the assembly steps
// pose_loss_kernel<0> calls, plus the root-relative outputs and the box root that only this kernel writes.
__global__ __launch_bounds__(64) void pose_assemble_kernel(const float* __restrict__ kp3d, const float* __restrict__ box6d, int box_stride,
                                                           const float* __restrict__ root_joint, const float* __restrict__ cam_intr,
                                                           const float* __restrict__ corners_can, int center_idx, float res_w, float res_h,
                                                           float depth_range, float* __restrict__ joints_abs, float* __restrict__ corners_abs,
                                                           float* __restrict__ rotmat, float* __restrict__ uvd2d, float* __restrict__ joints_rel,
                                                           float* __restrict__ corners_rel, float* __restrict__ boxroot) {
    const int b = blockIdx.x, lane = threadIdx.x;
    __shared__ float kp[66], Kc[9], CAN[8][3], RJ[3], avec[3], bvec[3], P[22][3], C[8][3], R[3][3];
    const PoseLds s = {kp, Kc, CAN, RJ, P, C, R};
    kp[lane] = kp3d[(long)b * 66 + lane];
    if (lane < 2) kp[64 + lane] = kp3d[(long)b * 66 + 64 + lane];
    if (lane < 9) Kc[lane] = cam_intr[(long)b * 9 + lane];
    if (lane < 24) (&CAN[0][0])[lane] = corners_can[(long)b * 24 + lane];
    if (lane < 3) { RJ[lane] = root_joint[b * 3 + lane]; avec[lane] = box6d[(long)b * box_stride + lane]; }
    else if (lane < 6) bvec[lane - 3] = box6d[(long)b * box_stride + lane];
    __syncthreads();
    uvd2xyz(s, lane, res_w, res_h, depth_range);
    if (lane == 0) { Rot6d rot; rot6d_fwd(avec, bvec, R, rot); }
    __syncthreads();
    box_corners(s, lane);
    __syncthreads();
    pose_write(s, lane, b, res_w, res_h, joints_abs, corners_abs, rotmat, uvd2d);
    if (lane < 63 && joints_rel) joints_rel[(long)b * 63 + lane] = P[lane / 3][lane % 3] - P[center_idx][lane % 3];
    if (lane < 24 && corners_rel) corners_rel[(long)b * 24 + lane] = C[lane / 3][lane % 3] - P[center_idx][lane % 3];
    if (lane < 3 && boxroot) boxroot[b * 3 + lane] = P[21][lane];
}

extern "C" int ab_pose_assemble(const float* kp3d, const float* box6d, int box_stride, const float* root_joint, const float* cam_intr,
                                const float* corners_can, int B, int center_idx, float res_w, float res_h, float* joints_abs,
                                float* corners_abs, float* rotmat, float* uvd2d, float* joints_rel, float* corners_rel, float* boxroot,
                                void* stream) {
    if (!kp3d || !box6d || !root_joint || !cam_intr || !corners_can || !joints_abs || !corners_abs || !rotmat) return AB_EINVAL;
    if (B <= 0 || center_idx < 0 || center_idx > 20 || box_stride < 6) return AB_ESHAPE;
    pose_assemble_kernel<<<B, 64, 0, as_stream(stream)>>>(kp3d, box6d, box_stride, root_joint, cam_intr, corners_can, center_idx, res_w, res_h,
                                                          0.4f, joints_abs, corners_abs, rotmat, uvd2d, joints_rel, corners_rel, boxroot);
    AB_LAUNCH_CHECK(); return 0;
}

extern "C" int ab_pose_loss(const float* kp3d, const float* box6d, int box_stride, const float* root_joint,
                            const float* cam_intr, const float* corners_can, const float* joints_3d,
                            const float* corners_3d, const float* joints_vis, const float* corners_vis,
                            const float* hand_views, int nvh, const int64_t* j0, const int64_t* j1, int njp,
                            const int64_t* p0, const int64_t* p1, int npp, const float* scene_views, int nvs,
                            const int64_t* s0, const int64_t* s1, int nsp, int B, int center_idx, float res_w,
                            float res_h, const float* weights8_host, float* joints_abs, float* corners_abs, float* rotmat,
                            float* uvd2d, float* sample_part, float* losses, float* g_kp3d, float* g_box6d,
                            void* stream) {
    return ab_pose_loss_sym(kp3d, box6d, box_stride, root_joint, cam_intr, corners_can, joints_3d, corners_3d, joints_vis,
                            corners_vis, hand_views, nvh, j0, j1, njp, p0, p1, npp, scene_views, nvs, s0, s1, nsp, B, center_idx,
                            res_w, res_h, weights8_host, nullptr, joints_abs, corners_abs, rotmat, uvd2d, sample_part, losses,
                            g_kp3d, g_box6d, stream);
}

// the classification-based model's criterion: pose_loss_kernel<0>, with SymCornerLoss (sym may be NULL) in the final loss (losses[5]) and
// the corner gradients.  weights8_host = {lam_joints, lam_corners, lam_hand_joint, lam_hand_part, lam_scene, w_JointsLoss, w_HandOrdLoss,
// w_SceneOrdLoss}
extern "C" int ab_pose_loss_sym(const float* kp3d, const float* box6d, int box_stride, const float* root_joint,
                                const float* cam_intr, const float* corners_can, const float* joints_3d,
                                const float* corners_3d, const float* joints_vis, const float* corners_vis,
                                const float* hand_views, int nvh, const int64_t* j0, const int64_t* j1, int njp,
                                const int64_t* p0, const int64_t* p1, int npp, const float* scene_views, int nvs,
                                const int64_t* s0, const int64_t* s1, int nsp, int B, int center_idx, float res_w,
                                float res_h, const float* weights8_host, const ab_symcorner* sym, float* joints_abs,
                                float* corners_abs, float* rotmat, float* uvd2d, float* sample_part, float* losses,
                                float* g_kp3d, float* g_box6d, void* stream) {
    if (!kp3d || !box6d || !root_joint || !cam_intr || !corners_can || !joints_3d || !corners_3d || !joints_vis ||
        !corners_vis || !weights8_host || !joints_abs || !corners_abs || !rotmat || !sample_part || !losses)
        return AB_EINVAL;
    if (njp > PL_MAXPAIR || npp > PL_MAXPAIR || nsp > PL_MAXPAIR || nvh > PL_MAXVIEW || nvs > PL_MAXVIEW || B < 1) return AB_ESHAPE;
    const float* w = weights8_host;
    if ((w[5] != 0.f || w[6] != 0.f) && (!hand_views || !j0 || !j1 || !p0 || !p1)) return AB_EINVAL;
    if (w[7] != 0.f && (!scene_views || !s0 || !s1)) return AB_EINVAL;
    // an ordinal loss without views has no pairs either
    const bool hand = (w[5] != 0.f || w[6] != 0.f) && nvh != 0, scene = w[7] != 0.f && nvs != 0;
    PoseLossArgs a = pl_args(kp3d, box6d, box_stride, root_joint, cam_intr, corners_can, joints_3d, corners_3d, joints_vis, corners_vis, hand,
                             hand_views, nvh, j0, j1, njp, p0, p1, npp, scene, scene_views, nvs, s0, s1, nsp, B, w, joints_abs, corners_abs,
                             rotmat, sample_part, g_kp3d, g_box6d);
    a.center_idx = center_idx; a.res_w = res_w; a.res_h = res_h; a.uvd2d = uvd2d;
    a.w_handord = w[6]; a.w_sceneord = w[7];
    if (sym && sym->K > 0 && sym->weight != 0.f && sym->lambda != 0.f) {
        if (!sym->R || !sym->t || !sym->obj_idx || !sym->obj_transf) return AB_EINVAL;
        a.sym_R = sym->R; a.sym_t = sym->t; a.obj_idx = sym->obj_idx; a.obj_transf = sym->obj_transf;
        a.symK = sym->K; a.lam_sym = sym->lambda; a.w_sym = sym->weight; a.sym_loss = sym->loss_out;
    }
    return pl_run<0>(a, losses, stream);
}

// ---- the regression-based model's criterion (HOPRegNet + [ManoLoss, JointsLoss, HandOrdLoss, SceneOrdLoss]): pose_loss_kernel<1>
// weights12_host = {LAMBDA_JOINTS_3D, LAMBDA_CORNERS_3D, LAMBDA_JOINTS_LEVEL, LAMBDA_PART_LEVEL, LAMBDA_SCENE_LEVEL, LAMBDAS[JointsLoss],
// LAMBDAS[HandOrdLoss], LAMBDAS[SceneOrdLoss], LAMBDA_SHAPE_REG, LAMBDA_POSE_REG, ManoLoss.LAMBDA_JOINTS_3D, LAMBDAS[ManoLoss]}.  An ordinal
// loss is present exactly when its draw buffers are passed (its scalars are reported even under a zero weight, as the registry does).
extern "C" int ab_reg_pose_loss(const float* joints_pred, const float* mano_pca_pose, const float* mano_shape, const float* transf,
                                int transf_stride, const float* root_joint, const float* cam_intr, const float* corners_can,
                                const float* joints_3d, const float* corners_3d, const float* joints_vis, const float* corners_vis,
                                const float* hand_views, int nvh, const int64_t* j0, const int64_t* j1, int njp, const int64_t* p0,
                                const int64_t* p1, int npp, const float* scene_views, int nvs, const int64_t* s0, const int64_t* s1,
                                int nsp, int B, int ncomps, const float* weights12_host, float* joints_abs, float* corners_abs,
                                float* rotmat, float* sample_part, float* losses, float* g_joints, float* g_pose, float* g_shape,
                                float* g_transf, void* stream) {
    if (!joints_pred || !mano_pca_pose || !mano_shape || !transf || !root_joint || !cam_intr || !corners_can || !joints_3d || !corners_3d ||
        !joints_vis || !corners_vis || !weights12_host || !joints_abs || !corners_abs || !rotmat || !sample_part || !losses)
        return AB_EINVAL;
    if (g_joints && (!g_pose || !g_shape || !g_transf)) return AB_EINVAL;
    if (B < 1 || ncomps < 1 || ncomps > 45 || transf_stride < 9) return AB_ESHAPE;
    const bool hand = hand_views && j0 && j1 && p0 && p1 && nvh > 0, scene = scene_views && s0 && s1 && nvs > 0;
    if (hand && (njp < 0 || npp < 0 || njp > PL_MAXPAIR || npp > PL_MAXPAIR || nvh > PL_MAXVIEW)) return AB_ESHAPE;
    if (scene && (nsp < 0 || nsp > PL_MAXPAIR || nvs > PL_MAXVIEW)) return AB_ESHAPE;
    const float* w = weights12_host;
    PoseLossArgs a = pl_args(joints_pred, transf, transf_stride, root_joint, cam_intr, corners_can, joints_3d, corners_3d, joints_vis,
                             corners_vis, hand, hand_views, nvh, j0, j1, njp, p0, p1, npp, scene, scene_views, nvs, s0, s1, nsp, B, w,
                             joints_abs, corners_abs, rotmat, sample_part, g_joints, g_transf);
    a.res_w = a.res_h = 1.f;
    a.w_handord = hand ? w[6] : 0.f; a.w_sceneord = scene ? w[7] : 0.f;
    a.lam_shape_reg = w[8]; a.lam_pose_reg = w[9]; a.lam_mano_joints = w[10]; a.w_mano = w[11];
    a.mano_pose = mano_pca_pose; a.mano_shape = mano_shape; a.ncomps = ncomps;
    a.g_pose = g_pose; a.g_shape = g_shape;
    return pl_run<1>(a, losses, stream);
}
