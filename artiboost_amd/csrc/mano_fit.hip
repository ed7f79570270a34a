// Hand-mesh fitting of the submission pass (anakin/postprocess/iknet/fittingunit.py:112-225), all B hands in ONE launch.
//
// The reference runs, per hand and in a Python loop, 20 JAX Adam steps (lr 0.03, b1 = b2 = 0.5, eps 1e-8, step index
// i = n = 1..20) on the objective `residuals` (fittingunit.py:63-80) over so3 [48], beta [10] and bone [1], then skins the
// fitted hand (`mano_de`, :83-97).  Here one 256-thread workgroup owns one hand:
//   prologue   normalise the raw IKNet quaternions and convert them to axis-angle (utils.py:13-41) for EVERY hand of the
//              batch, summed per component in a fixed order (no atomics): the pose regulariser pulls towards the batch mean
//              (`so3_init` is the whole batch, :190); root, bone and target from the predicted joints (:157-163)
//   loop       per step: the 21 model joints (16 Rodrigues, J = J_template + J_shapedirs . beta, 3-level chain, the 5
//              fingertip vertices only), the objective, its exact reverse and the Adam update -- the state stays in LDS
//   epilogue   the full 778-vertex MANO skinning of the fitted parameters (mano_state), scaled by the predicted bone and
//              moved to the predicted root
// Every reduction runs in a fixed order: the result is bit-reproducible.  Exact fp32 throughout (the reference's own
// precision: JAX's default).
//
// Ties of the two non-smooth terms follow JAX: d|t|/dt = sign(t) (0 at t == 0); -min(S, 0) passes -1 where S < 0, none
// where S > 0 and -1/2 at S == 0 (jnp.clip is lax.max then lax.min, whose gradient splits a tie evenly).
#include "mano_common.h"

#define NP 59          // parameters per hand: so3 [48] | beta [10] | bone [1]

// utils.py:13-41: F.normalize(eps=1e-12), then quaternion_to_angle_axis with its my_atan2 and the sin^2 == 0 -> k = 2 branch
__device__ __forceinline__ void fit_quat_to_aa(const float* __restrict__ q, float aa[3]) {
    const float n = fmaxf(sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]), 1e-12f);
    const float q0 = q[0] / n, q1 = q[1] / n, q2 = q[2] / n, q3 = q[3] / n;
    const float s2 = (q1 * q1 + q2 * q2) + q3 * q3;
    const float s = sqrtf(s2);
    const float y = q0 < 0.f ? -s : s, x = q0 < 0.f ? -q0 : q0;
    float t = atanf(y / x);
    if (y > 0.f && x < 0.f) t += 3.14159265358979f;
    if (y < 0.f && x < 0.f) t += 3.14159265358979f;
    const float k = s2 > 0.f ? (2.f * t) / s : 2.f;
    aa[0] = q1 * k; aa[1] = q2 * k; aa[2] = q3 * k;
}

__global__ __launch_bounds__(256) void mano_fit_kernel(const float* __restrict__ quat, const float* __restrict__ pred_joints,
                                                       const float* __restrict__ v_template, const float* __restrict__ shapedirs,
                                                       const float* __restrict__ posedirs, const float* __restrict__ J_regressor,
                                                       const float* __restrict__ weights, const float* __restrict__ J_template,
                                                       const float* __restrict__ J_shapedirs, int B, int n_iter, int step0, int init,
                                                       float* __restrict__ params, float* __restrict__ adam_m, float* __restrict__ adam_v,
                                                       float* __restrict__ verts, float* __restrict__ joints, float* __restrict__ loss,
                                                       float* __restrict__ grad) {
    const int b = blockIdx.x, tid = threadIdx.x;
    // per-hand constants
    __shared__ float mu[48], spread[48], own[48];   // batch mean of so3_init, sum_b (so3_init_b - mu)^2, this hand's so3_init
    __shared__ float root[3], tgt[63], bone0;
    __shared__ float tpd[15][135], tsd[15][10], tvt[15], tw[5][16];   // posedirs / shapedirs / v_template / weights of the tips
    __shared__ float jsd[48][10], jt[48];
    // optimiser state
    __shared__ float x[NP], am[NP], av[NP], g[NP];
    // step scratch
    __shared__ float R[NJ][9], J[NJ][3], G[NJ][12], G2[NJ][12];
    __shared__ float tvs[15], tvp[15], tpart[15][9];
    __shared__ float jr[63], gjr[63], gtip[15], gvp[15], gpmap[135];
    __shared__ float ou[63], ogu[63], oP[63], ogP[63];               // the objective's per-joint terms (thread 0)
    __shared__ float gGt[NJ][3], gG2[NJ][12], gR[NJ][9], gJ[NJ][3];
    __shared__ float lossv;
    // epilogue
    __shared__ float pmap[135], vs[NV * 3], vo[NV * 3], part[256], bpe;

    // ---------------------------------------------------------------- prologue
    // so3_init of every hand of the batch: 16 lanes per joint, lane l takes the hands h = l, l + 16, ... in order; the 16 partial
    // sums of each component are then added in lane order (vs serves as scratch until the epilogue).  Two passes: mean, spread.
    {
        const int j = tid >> 4, l = tid & 15;
        float s[3] = {0.f, 0.f, 0.f};
        for (int h = l; h < B; h += 16) {
            float aa[3];
            fit_quat_to_aa(quat + ((size_t)h * NJ + j) * 4, aa);
            for (int c = 0; c < 3; ++c) s[c] += aa[c];
            if (h == b) for (int c = 0; c < 3; ++c) own[j * 3 + c] = aa[c];
        }
        for (int c = 0; c < 3; ++c) vs[tid * 3 + c] = s[c];
        __syncthreads();
        if (tid < 48) {
            const int jj = tid / 3, c = tid % 3;
            float m = 0.f;
            for (int p = 0; p < 16; ++p) m += vs[(jj * 16 + p) * 3 + c];
            mu[tid] = m / (float)B;
        }
        __syncthreads();
        float d[3] = {0.f, 0.f, 0.f};
        for (int h = l; h < B; h += 16) {
            float aa[3];
            fit_quat_to_aa(quat + ((size_t)h * NJ + j) * 4, aa);
            for (int c = 0; c < 3; ++c) d[c] += (aa[c] - mu[j * 3 + c]) * (aa[c] - mu[j * 3 + c]);
        }
        for (int c = 0; c < 3; ++c) vo[tid * 3 + c] = d[c];
        __syncthreads();
        if (tid < 48) {
            const int jj = tid / 3, c = tid % 3;
            float m = 0.f;
            for (int p = 0; p < 16; ++p) m += vo[(jj * 16 + p) * 3 + c];
            spread[tid] = m;
        } else if (tid == 64) {
            // root = j[9]; bone = |(j[0] - root) - (j[9] - root)| = |j[0] - j[9]| (fittingunit.py:158-161)
            const float* pj = pred_joints + (size_t)b * 63;
            const float d0 = pj[0] - pj[27], d1 = pj[1] - pj[28], d2 = pj[2] - pj[29];
            root[0] = pj[27]; root[1] = pj[28]; root[2] = pj[29];
            bone0 = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
        }
    }
    for (int i = tid; i < 15 * 135; i += 256) {
        const int r = i / 135, k = i % 135;
        tpd[r][k] = posedirs[((size_t)c_mano_tips[r / 3] * 3 + r % 3) * 135 + k];
    }
    if (tid < 150) tsd[tid / 10][tid % 10] = shapedirs[((size_t)c_mano_tips[tid / 30] * 3 + (tid / 10) % 3) * 10 + tid % 10];
    else if (tid < 165) tvt[tid - 150] = v_template[c_mano_tips[(tid - 150) / 3] * 3 + (tid - 150) % 3];
    else if (tid < 245) tw[(tid - 165) / 16][(tid - 165) % 16] = weights[c_mano_tips[(tid - 165) / 16] * NJ + (tid - 165) % 16];
    for (int i = tid; i < 480; i += 256) jsd[i / 10][i % 10] = J_shapedirs[i];
    if (tid < 48) jt[tid] = J_template[tid];
    __syncthreads();
    if (tid < 63) tgt[tid] = (pred_joints[(size_t)b * 63 + tid] - root[tid % 3]) / bone0;
    if (tid < NP) {
        const size_t o = (size_t)b * NP + tid;
        x[tid] = init ? (tid < 48 ? own[tid] : (tid < 58 ? 0.f : bone0)) : params[o];
        am[tid] = init ? 0.f : adam_m[o];
        av[tid] = init ? 0.f : adam_v[o];
    }
    __syncthreads();

    // ---------------------------------------------------------------- Adam steps
    for (int it = 0; it < n_iter; ++it) {
        // -- forward: Rodrigues x16, rest joints, rest fingertips
        if (tid < NJ) {
            const float a[3] = {x[tid * 3], x[tid * 3 + 1], x[tid * 3 + 2]};
            mano_rodrigues(a, R[tid]);
        } else if (tid >= 64 && tid < 112) {
            const int o = tid - 64;
            float s = jt[o];
            for (int l = 0; l < 10; ++l) s += jsd[o][l] * x[48 + l];
            J[o / 3][o % 3] = s;
        } else if (tid >= 128 && tid < 143) {
            const int i = tid - 128;
            float s = tvt[i];
            for (int l = 0; l < 10; ++l) s += tsd[i][l] * x[48 + l];
            tvs[i] = s;
        }
        __syncthreads();
        // -- pose blend of the tips (15 rows x 135 as 9 partial sums of 15 terms) || kinematic chain (thread 255)
        if (tid < 135) {
            const int i = tid / 9, p = tid % 9;
            float s = 0.f;
            for (int k = p * 15; k < p * 15 + 15; ++k) {
                const int kk = k % 9;
                s += tpd[i][k] * (R[k / 9 + 1][kk] - ((kk == 0 || kk == 4 || kk == 8) ? 1.f : 0.f));
            }
            tpart[i][p] = s;
        } else if (tid == 255) {
            for (int j = 0; j < NJ; ++j) {
                const int par = c_mano_parents[j];
                float L[12];
                for (int r = 0; r < 3; ++r) {
                    for (int c = 0; c < 3; ++c) L[r * 4 + c] = R[j][r * 3 + c];
                    L[r * 4 + 3] = par < 0 ? J[0][r] : (J[j][r] - J[par][r]);
                }
                if (par < 0) { for (int k = 0; k < 12; ++k) G[j][k] = L[k]; }
                else {
                    const float* P = G[par];
                    for (int r = 0; r < 3; ++r)
                        for (int c = 0; c < 4; ++c) {
                            float s = (P[r * 4] * L[c] + P[r * 4 + 1] * L[4 + c]) + P[r * 4 + 2] * L[8 + c];
                            if (c == 3) s += P[r * 4 + 3];
                            G[j][r * 4 + c] = s;
                        }
                }
            }
            for (int j = 0; j < NJ; ++j)
                for (int r = 0; r < 3; ++r) {
                    const float* gg = G[j];
                    const float corr = (gg[r * 4] * J[j][0] + gg[r * 4 + 1] * J[j][1]) + gg[r * 4 + 2] * J[j][2];
                    for (int c = 0; c < 3; ++c) G2[j][r * 4 + c] = gg[r * 4 + c];
                    G2[j][r * 4 + 3] = gg[r * 4 + 3] - corr;
                }
        }
        __syncthreads();
        if (tid < 15) {
            float s = tvs[tid];
            for (int p = 0; p < 9; ++p) s += tpart[tid][p];
            tvp[tid] = s;
        }
        __syncthreads();
        // -- 21 joints: 16 transform translations + 5 skinned fingertips, reordered
        if (tid < 63) {
            const int k = tid / 3, c = tid % 3, src = c_mano_reorder[k];
            float val;
            if (src < 16) val = G[src][c * 4 + 3];
            else {
                const int t = src - 16;
                float T[4] = {0.f, 0.f, 0.f, 0.f};
                for (int j = 0; j < NJ; ++j) {
                    const float w = tw[t][j];
                    if (w != 0.f) for (int q = 0; q < 4; ++q) T[q] += w * G2[j][c * 4 + q];
                }
                val = ((T[0] * tvp[t * 3] + T[1] * tvp[t * 3 + 1]) + T[2] * tvp[t * 3 + 2]) + T[3];
            }
            jr[tid] = val;
        }
        __syncthreads();
        // -- objective (thread 0): centring on joint 9, errkp, geo; its gradient w.r.t. the 21 joints and the bone
        if (tid == 0) {
            // jm = jr - jr[9];  bone_pred = |jm[0] - jm[9]|
            const float d0 = (jr[0] - jr[27]) - (jr[27] - jr[27]), d1 = (jr[1] - jr[28]) - (jr[28] - jr[28]);
            const float d2 = (jr[2] - jr[29]) - (jr[29] - jr[29]);
            const float bp = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
            const float bone = x[58];
            float errkp = 0.f;
            for (int i = 0; i < 63; ++i) {
                const float u = (jr[i] - jr[27 + i % 3]) / bp;
                const float e = u - tgt[i];
                errkp += e * e;
                ou[i] = u;
                ogu[i] = (2.f / 63.f) * e;
                oP[i] = u * bone + root[i % 3];
                ogP[i] = 0.f;
            }
            errkp /= 63.f;
            float l1 = 0.f, S = 0.f;
            float tf[5], vab[5][3], vbc[5][3], vcd[5][3], c1[5][3], c2[5][3];
            for (int f = 0; f < 5; ++f) {
                const int a = 1 + 4 * f;
                for (int c = 0; c < 3; ++c) {
                    vab[f][c] = oP[a * 3 + c] - oP[(a + 1) * 3 + c];
                    vbc[f][c] = oP[(a + 1) * 3 + c] - oP[(a + 2) * 3 + c];
                    vcd[f][c] = oP[(a + 2) * 3 + c] - oP[(a + 3) * 3 + c];
                }
                cross3(vab[f], vbc[f], c1[f]);
                cross3(vbc[f], vcd[f], c2[f]);
                tf[f] = (c1[f][0] * vcd[f][0] + c1[f][1] * vcd[f][1]) + c1[f][2] * vcd[f][2];
                l1 += fabsf(tf[f]);
                for (int c = 0; c < 3; ++c) S += c1[f][c] * c2[f][c];
            }
            l1 /= 5.f;
            const float l2 = -fminf(S, 0.f);
            const float geo = 10000.f * l1 + 100000.f * l2;
            const float gS = 100.f * 100000.f * (S < 0.f ? -1.f : (S == 0.f ? -0.5f : 0.f));
            for (int f = 0; f < 5; ++f) {
                const float gt = 100.f * 10000.f * (tf[f] > 0.f ? 1.f : (tf[f] < 0.f ? -1.f : 0.f)) / 5.f;
                float t_ab[3], t_bc[3], s_ab[3], s_bc1[3], s_bc2[3], s_cd[3], ga[3], gb[3], gc[3];
                cross3(vbc[f], vcd[f], t_ab);     // dt/dvab
                cross3(vcd[f], vab[f], t_bc);     // dt/dvbc       (dt/dvcd = c1)
                cross3(vbc[f], c2[f], s_ab);      // dS/dvab
                cross3(c2[f], vab[f], s_bc1);     // dS/dvbc through c1
                cross3(vcd[f], c1[f], s_bc2);     // dS/dvbc through c2
                cross3(c1[f], vbc[f], s_cd);      // dS/dvcd
                for (int c = 0; c < 3; ++c) {
                    ga[c] = gt * t_ab[c] + gS * s_ab[c];
                    gb[c] = gt * t_bc[c] + gS * (s_bc1[c] + s_bc2[c]);
                    gc[c] = gt * c1[f][c] + gS * s_cd[c];
                }
                const int a = 1 + 4 * f;
                for (int c = 0; c < 3; ++c) {
                    ogP[a * 3 + c] += ga[c];
                    ogP[(a + 1) * 3 + c] += gb[c] - ga[c];
                    ogP[(a + 2) * 3 + c] += gc[c] - gb[c];
                    ogP[(a + 3) * 3 + c] -= gc[c];
                }
            }
            // P = u bone + root;  u = jm / bone_pred
            float gbone = 0.f, gbp = 0.f;
            for (int i = 0; i < 63; ++i) {
                gbone += ogP[i] * ou[i];
                const float gu = ogu[i] + ogP[i] * bone;
                ogu[i] = gu;
                gbp -= gu * ou[i];
            }
            gbp /= bp;
            g[58] = gbone;
            const float dd[3] = {d0 / bp, d1 / bp, d2 / bp};
            float cs[3] = {0.f, 0.f, 0.f};
            for (int i = 0; i < 63; ++i) {
                float gjm = ogu[i] / bp;
                if (i < 3) gjm += gbp * dd[i];
                else if (i >= 27 && i < 30) gjm -= gbp * dd[i - 27];
                gjr[i] = gjm;
                cs[i % 3] += gjm;
            }
            for (int c = 0; c < 3; ++c) gjr[27 + c] -= cs[c];     // centring on joint 9
            if (loss) {
                float reg = 0.f, regb = 0.f;
                for (int k = 0; k < 48; ++k) { const float e = x[k] - mu[k]; reg += (float)B * (e * e) + spread[k]; }
                reg /= (float)B * 48.f;
                for (int l = 0; l < 10; ++l) regb += x[48 + l] * x[48 + l];
                lossv = ((0.01f * reg + 0.01f * regb) + errkp) + 100.f * geo;
            }
        }
        __syncthreads();
        // -- reverse of the joint reordering (a permutation: every target written once)
        if (tid < 63) {
            const int k = tid / 3, c = tid % 3, src = c_mano_reorder[k];
            if (src < 16) gGt[src][c] = gjr[tid];
            else gtip[(src - 16) * 3 + c] = gjr[tid];
        }
        __syncthreads();
        // -- reverse of the tip skinning: dL/dG2_j = sum_t w_tj g_t (x) [vp_t, 1];  dL/dvp_t = T_t[:, :3]^T g_t
        if (tid < NJ * 12) {
            const int j = tid / 12, r = (tid % 12) / 4, c = tid % 4;
            float s = 0.f;
            for (int t = 0; t < 5; ++t) {
                const float w = tw[t][j];
                if (w != 0.f) s += w * gtip[t * 3 + r] * (c < 3 ? tvp[t * 3 + c] : 1.f);
            }
            gG2[j][r * 4 + c] = s;
        } else if (tid >= 192 && tid < 207) {
            const int i = tid - 192, t = i / 3, c = i % 3;
            float T[3] = {0.f, 0.f, 0.f};      // column c of T_t
            for (int j = 0; j < NJ; ++j) {
                const float w = tw[t][j];
                if (w != 0.f) for (int r = 0; r < 3; ++r) T[r] += w * G2[j][r * 4 + c];
            }
            gvp[i] = (T[0] * gtip[t * 3] + T[1] * gtip[t * 3 + 1]) + T[2] * gtip[t * 3 + 2];
        }
        __syncthreads();
        // -- reverse of the pose blend (135 outputs over the 15 tip rows) || the chain in reverse (thread 255)
        if (tid < 135) {
            float s = 0.f;
            for (int i = 0; i < 15; ++i) s += tpd[i][tid] * gvp[i];
            gpmap[tid] = s;
        } else if (tid == 255) {
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
                    gJ[j][k] += gL[k * 4 + 3];
                    if (par >= 0) gJ[par][k] -= gL[k * 4 + 3];
                }
            }
        }
        __syncthreads();
        // -- Rodrigues reverse (+ the pose regulariser) -> dL/dso3;  rest joints and tip shape blend reverse -> dL/dbeta
        if (tid < NJ) {
            float gr[9];
            for (int k = 0; k < 9; ++k) gr[k] = gR[tid][k] + (tid > 0 ? gpmap[(tid - 1) * 9 + k] : 0.f);
            const float a[3] = {x[tid * 3], x[tid * 3 + 1], x[tid * 3 + 2]};
            float ga[3];
            mano_rodrigues_bwd(a, gr, ga);
            for (int c = 0; c < 3; ++c) {
                const int k = tid * 3 + c;
                g[k] = ga[c] + 0.01f * (2.f * (x[k] - mu[k]) / 48.f);
            }
        } else if (tid >= 64 && tid < 74) {
            const int l = tid - 64;
            float s = 0.f;
            for (int o = 0; o < 48; ++o) s += jsd[o][l] * gJ[o / 3][o % 3];
            for (int i = 0; i < 15; ++i) s += tsd[i][l] * gvp[i];
            g[48 + l] = s + 0.01f * (2.f * x[48 + l]);
        }
        __syncthreads();
        // -- Adam (jax.experimental.optimizers.adam(0.03, b1=0.5, b2=0.5), eps 1e-8), step index n = step0 + it
        if (tid < NP) {
            const float gg = g[tid];
            const float m = 0.5f * gg + 0.5f * am[tid];
            const float v = 0.5f * (gg * gg) + 0.5f * av[tid];
            const float bc = 1.f - ldexpf(1.f, -(step0 + it + 1));      // 1 - 0.5^(n+1), exact
            const float mhat = m / bc, vhat = v / bc;
            x[tid] = x[tid] - (0.03f * mhat) / (sqrtf(vhat) + 1e-8f);
            am[tid] = m; av[tid] = v;
            if (grad && it == n_iter - 1) grad[(size_t)b * NP + tid] = gg;
        }
        if (tid == 0 && loss) loss[(size_t)b * n_iter + it] = lossv;
        __syncthreads();
    }
    if (tid < NP) {
        const size_t o = (size_t)b * NP + tid;
        params[o] = x[tid]; adam_m[o] = am[tid]; adam_v[o] = av[tid];
    }
    if (!verts && !joints) return;

    // ---------------------------------------------------------------- epilogue: mano_de (fittingunit.py:83-97)
    mano_state(tid, x, x + 48, v_template, shapedirs, posedirs, J_regressor, R, pmap, vs, J, G, G2, part);
    for (int v = tid; v < NV; v += 256) {
        float T[12];
        mano_skin_T(weights, G2, v, T);
        const float px = vs[v * 3], py = vs[v * 3 + 1], pz = vs[v * 3 + 2];
        for (int r = 0; r < 3; ++r) vo[v * 3 + r] = ((T[r * 4] * px + T[r * 4 + 1] * py) + T[r * 4 + 2] * pz) + T[r * 4 + 3];
    }
    __syncthreads();
    if (tid < 63) {
        const int k = tid / 3, c = tid % 3, src = c_mano_reorder[k];
        jr[tid] = src < 16 ? G[src][c * 4 + 3] : vo[c_mano_tips[src - 16] * 3 + c];
    }
    __syncthreads();
    if (tid == 0) {
        const float d0 = jr[0] - jr[27], d1 = jr[1] - jr[28], d2 = jr[2] - jr[29];
        bpe = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
    }
    __syncthreads();
    // x / bone_pred * bone + root with the PREDICTED bone (bone_this, :202), not the optimised one
    if (verts) {
        float* vg = verts + (size_t)b * NV * 3;
        for (int i = tid; i < NV * 3; i += 256) vg[i] = ((vo[i] - jr[27 + i % 3]) / bpe) * bone0 + root[i % 3];
    }
    if (joints && tid < 63) joints[(size_t)b * 63 + tid] = ((jr[tid] - jr[27 + tid % 3]) / bpe) * bone0 + root[tid % 3];
}

extern "C" int ab_mano_fit(const float* quat, const float* pred_joints, const float* v_template, const float* shapedirs,
                           const float* posedirs, const float* J_regressor, const float* weights, const float* J_template,
                           const float* J_shapedirs, int B, int n_iter, int step0, int init, float* params, float* adam_m,
                           float* adam_v, float* verts, float* joints, float* loss, float* grad, void* stream) {
    if (!quat || !pred_joints || !v_template || !shapedirs || !posedirs || !J_regressor || !weights || !J_template || !J_shapedirs ||
        !params || !adam_m || !adam_v)
        return AB_EINVAL;
    if (B < 1 || n_iter < 0 || step0 < 0 || step0 + n_iter > 120) return AB_ESHAPE;
    mano_fit_kernel<<<B, 256, 0, as_stream(stream)>>>(quat, pred_joints, v_template, shapedirs, posedirs, J_regressor, weights,
                                                      J_template, J_shapedirs, B, n_iter, step0, init, params, adam_m, adam_v,
                                                      verts, joints, n_iter > 0 ? loss : nullptr, n_iter > 0 ? grad : nullptr);
    AB_LAUNCH_CHECK();
    return 0;
}
