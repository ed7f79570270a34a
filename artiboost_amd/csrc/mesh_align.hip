// Mesh-level registry losses on the device, eager route only:
//   ab_chamfer_rigid    anakin/criterions/chamferloss.py:11-52 over the brute-force nearest neighbour of criterions.chamfer_distance_torch
//   ab_procrustes_loss  anakin/criterions/alignloss.py:52-80 plus the MSE
//
// Chamfer.  x_i = keep (R can_i + t), y_j = keep (targ_j + root), keep = any(corners_vis != 0), formed here.  One workgroup per (sample,
// chunk of 256 query points); the first ceil(N/256) chunks of a sample own points of x and scan y, the other ceil(M/256) own points of y and
// scan x.  The scan is nn_tile_scan (csrc/nn_tile.h), with the winner's index kept (the first minimum wins, as argmin does).
// x_i is the same fused-multiply-add chain wherever it is formed (staged tile or query register), so both directions
// see the same bits.  The gradient needs no scatter: a query of x adds d = x_i - y_i* to the sums  sum d,  sum d can_i^T;  a query of y
// adds d = x_j* - y_j with can_j* gathered once.  A chunk's 13 sums (distance, 3, 9) are reduced in a fixed order (wave butterfly, then the
// four waves in turn) into the workspace, and a second small launch adds the chunks of a sample in turn, scales, and sums the batch in a
// fixed order.  No atomics: two calls give the same bits, and a sample's distances and (x B) gradients do not depend on the batch around it.
//
// Procrustes.  One wave per sample solves procrustes_fit (csrc/procrustes.h: c, p, s, R and the notation are defined there), then
//   sample_loss = c^2 sum_i |s R Ph_i - Xh_i|^2 / (3n)   -- from the residual itself: 1 - s^2 has no digits left when s -> 1.
// R is the optimum, so no SVD backward: d loss / d M = -2 c^2 s R / (3 n B), d loss / d Ph_i = -2 c^2 s (R^T Xh_i - s Ph_i) / (3 n B) up to
// the 1e-8 of the norm (see the kernel), then through Ph = Pc / p (the radial part, -s Ph_i included, drops out) and the centring.
#include "common.h"
#include "nn_tile.h"
#include "procrustes.h"

#define CH_THREADS 256         // one query point per thread
#define CH_TILE 1024           // scanned points staged per round: 12 KiB SoA
#define CH_PART 16             // floats per (sample, chunk) partial: distance | sum d [3] | sum d can^T [9] | unused [3]

__device__ __forceinline__ float rigid1(const float* r, float t, float cx, float cy, float cz) {
    return __builtin_fmaf(r[2], cz, __builtin_fmaf(r[1], cy, r[0] * cx)) + t;
}

__global__ __launch_bounds__(CH_THREADS) void chamfer_rigid_kernel(const float* __restrict__ can, const float* __restrict__ rot,
                                                                    const float* __restrict__ tsl, const float* __restrict__ targ,
                                                                    const float* __restrict__ root, const float* __restrict__ corners_vis,
                                                                    int N, int M, int cx, float* __restrict__ dist_xy,
                                                                    float* __restrict__ dist_yx, int32_t* __restrict__ idx_xy,
                                                                    int32_t* __restrict__ idx_yx, int want_grad, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float vs[3 * CH_TILE];
    __shared__ float s_red[4][13];
    const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const bool own_x = chunk < cx;                                               // block-uniform: this chunk's queries are points of x
    const int nq = own_x ? N : M, ns = own_x ? M : N;                            // queries / scanned points of this direction
    const int q0 = (own_x ? chunk : chunk - cx) * CH_THREADS;
    const int q = q0 + (int)threadIdx.x;
    const bool live = q < nq;
    float* dist = own_x ? dist_xy : dist_yx;
    int32_t* idx = own_x ? idx_xy : idx_yx;
    float* pout = part + ((size_t)b * nchunks + chunk) * CH_PART;

    bool keep = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) keep = keep || (corners_vis[(size_t)b * 8 + k] != 0.f);
    if (!keep) {                                                                 // block-uniform: both clouds collapse to the origin
        if (live) {
            if (dist) dist[(size_t)b * nq + q] = 0.f;
            if (idx) idx[(size_t)b * nq + q] = 0;
        }
        if (threadIdx.x < CH_PART) pout[threadIdx.x] = 0.f;
        return;
    }
    float R[9], t[3], rt[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = rot[(size_t)b * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) { t[k] = tsl[(size_t)b * 3 + k]; rt[k] = root[(size_t)b * 3 + k]; }
    const float* cb = can + (size_t)b * N * 3;
    const float* tb = targ + (size_t)b * M * 3;

    const int qc = live ? q : nq - 1;                                            // lanes past the end recompute the last point (masked below)
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, px, py, pz;                              // the query point (and its canonical vertex when it is of x)
    if (own_x) {
        c0 = cb[(size_t)qc * 3]; c1 = cb[(size_t)qc * 3 + 1]; c2 = cb[(size_t)qc * 3 + 2];
        px = rigid1(R, t[0], c0, c1, c2); py = rigid1(R + 3, t[1], c0, c1, c2); pz = rigid1(R + 6, t[2], c0, c1, c2);
    } else {
        px = tb[(size_t)qc * 3] + rt[0]; py = tb[(size_t)qc * 3 + 1] + rt[1]; pz = tb[(size_t)qc * 3 + 2] + rt[2];
    }
    const nn_hit hit = nn_tile_scan<CH_TILE, CH_THREADS, true>(vs, ns, px, py, pz, [&](size_t src, float& a0, float& a1, float& a2) {
        if (own_x) { a0 = tb[src] + rt[0]; a1 = tb[src + 1] + rt[1]; a2 = tb[src + 2] + rt[2]; }
        else {
            const float s0 = cb[src], s1 = cb[src + 1], s2 = cb[src + 2];
            a0 = rigid1(R, t[0], s0, s1, s2); a1 = rigid1(R + 3, t[1], s0, s1, s2); a2 = rigid1(R + 6, t[2], s0, s1, s2);
        }
    });
    const float best = hit.d2;
    const int besti = hit.idx >= ns ? ns - 1 : hit.idx;                          // (cannot happen for finite inputs; keeps the gather in bounds)
    if (live) {
        if (dist) dist[(size_t)b * nq + q] = best;
        if (idx) idx[(size_t)b * nq + q] = besti;
    }
    float acc[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) acc[k] = 0.f;
    if (live) {
        acc[0] = best;
        if (want_grad) {
            float d0, d1, d2;                                                    // x - y of the matched pair, and the canonical vertex of its x
            if (own_x) {
                const size_t src = (size_t)besti * 3;
                d0 = px - (tb[src] + rt[0]); d1 = py - (tb[src + 1] + rt[1]); d2 = pz - (tb[src + 2] + rt[2]);
            } else {
                const size_t src = (size_t)besti * 3;
                c0 = cb[src]; c1 = cb[src + 1]; c2 = cb[src + 2];
                d0 = rigid1(R, t[0], c0, c1, c2) - px; d1 = rigid1(R + 3, t[1], c0, c1, c2) - py; d2 = rigid1(R + 6, t[2], c0, c1, c2) - pz;
            }
            acc[1] = d0; acc[2] = d1; acc[3] = d2;
            acc[4] = d0 * c0; acc[5] = d0 * c1; acc[6] = d0 * c2;
            acc[7] = d1 * c0; acc[8] = d1 * c1; acc[9] = d1 * c2;
            acc[10] = d2 * c0; acc[11] = d2 * c1; acc[12] = d2 * c2;
        }
    }
    const float tot = block_sum4<13>(acc, s_red);
    if (threadIdx.x < CH_PART) pout[threadIdx.x] = threadIdx.x < 13 ? tot : 0.f;
}

// One thread per sample adds its chunks in turn; the batch sum of the distances is a fixed tree (thread-serial, wave butterfly, waves in turn).
__global__ __launch_bounds__(256) void chamfer_rigid_finalize_kernel(const float* __restrict__ part, int B, int N, int M, int cx, int cy,
                                                                     float* __restrict__ loss, float* __restrict__ g_rot,
                                                                     float* __restrict__ g_tsl) {
    __shared__ float s_red[4][2];
    const int nchunks = cx + cy;
    const float sxy = (2.f / (float)N) / (float)B, syx = (2.f / (float)M) / (float)B;   // 1/B last: exact when B is a power of two
    float a[2] = {0.f, 0.f};                                                     // distances x -> y | y -> x
    for (int b = threadIdx.x; b < B; b += 256) {
        float sx[13], sy[13];
#pragma unroll
        for (int k = 0; k < 13; ++k) sx[k] = sy[k] = 0.f;
        const float* p = part + (size_t)b * nchunks * CH_PART;
        for (int c = 0; c < cx; ++c)
#pragma unroll
            for (int k = 0; k < 13; ++k) sx[k] += p[(size_t)c * CH_PART + k];
        for (int c = cx; c < nchunks; ++c)
#pragma unroll
            for (int k = 0; k < 13; ++k) sy[k] += p[(size_t)c * CH_PART + k];
        a[0] += sx[0]; a[1] += sy[0];
        if (g_rot) {
#pragma unroll
            for (int k = 0; k < 3; ++k) g_tsl[(size_t)b * 3 + k] = sxy * sx[1 + k] + syx * sy[1 + k];
#pragma unroll
            for (int k = 0; k < 9; ++k) g_rot[(size_t)b * 9 + k] = sxy * sx[4 + k] + syx * sy[4 + k];
        }
    }
    const float txy = block_sum4<2>(a, s_red), tyx = __shfl(txy, 1, 64);          // thread 0 takes thread 1's column
    if (threadIdx.x == 0) loss[0] = txy / ((float)B * (float)N) + tyx / ((float)B * (float)M);
}

extern "C" long ab_chamfer_rigid_workspace(int B, int N, int M) {
    if (B < 1 || N < 1 || M < 1) return 0;
    const long nchunks = ((long)N + CH_THREADS - 1) / CH_THREADS + ((long)M + CH_THREADS - 1) / CH_THREADS;
    return (long)B * nchunks * CH_PART * (long)sizeof(float);
}

extern "C" int ab_chamfer_rigid(const float* can, const float* rot, const float* tsl, const float* targ, const float* root,
                                const float* corners_vis, int B, int N, int M, float* loss, float* dist_xy, float* dist_yx,
                                int32_t* idx_xy, int32_t* idx_yx, float* g_rot, float* g_tsl, void* workspace, void* stream) {
    if (!can || !rot || !tsl || !targ || !root || !corners_vis || !loss || !workspace) return AB_EINVAL;
    if (B < 1 || B > 65535 || N < 1 || M < 1) return AB_EINVAL;
    if ((g_rot == nullptr) != (g_tsl == nullptr)) return AB_EINVAL;
    const int cx = (N + CH_THREADS - 1) / CH_THREADS, cy = (M + CH_THREADS - 1) / CH_THREADS;
    float* part = (float*)workspace;
    chamfer_rigid_kernel<<<dim3(cx + cy, B), CH_THREADS, 0, as_stream(stream)>>>(can, rot, tsl, targ, root, corners_vis, N, M, cx, dist_xy,
                                                                                dist_yx, idx_xy, idx_yx, g_rot ? 1 : 0, part);
    AB_LAUNCH_CHECK();
    chamfer_rigid_finalize_kernel<<<1, 256, 0, as_stream(stream)>>>(part, B, N, M, cx, cy, loss, g_rot, g_tsl);
    AB_LAUNCH_CHECK();
    return 0;
}

// ---- Procrustes-aligned MSE ------------------------------------------------------------------------------------------------------------------
#define PR_THREADS 256         // four waves, one sample each
__global__ __launch_bounds__(PR_THREADS) void procrustes_kernel(const float* __restrict__ pred, const float* __restrict__ targ,
                                                                 const float* __restrict__ root, int B, int n, float* __restrict__ sample_loss,
                                                                 float* __restrict__ aligned, float* __restrict__ g_pred) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * (PR_THREADS / 64) + (threadIdx.x >> 6);
    if (b >= B) return;                                                          // wave-uniform; no barrier below
    const float* P = pred + (size_t)b * n * 3;
    const float* X = targ + (size_t)b * n * 3;
    const float inv_n = 1.f / (float)n;
    pr_fit f;
    procrustes_fit(P, X, n, lane, f);
    const float *mp = f.mp, *mx = f.mx, cs = f.c, ps = f.p, s = f.s;
    const float(&Rm)[3][3] = f.R;
    // residual, loss, and the gradient's two inner products
    const float ic = 1.f / cs, ip = 1.f / ps;
    const float k0 = (-2.f * (cs * cs) * s) / (3.f * (float)n);
    const float kb = k0 / (float)B;                                             // 1/B last: exact when B is a power of two
    const float sc = s * cs;
    // the 1e-8 of the prediction's norm, kept: |Ph|^2 = q = 1 - 2e-8 / p, and d loss / d Ph_i = kb ((2 - q) R^T Xh_i - s Ph_i).  Against a
    // gradient that is itself a difference of nearly equal vectors (a near-perfect prediction) it is a 1e-4 relative term, not a rounding
    // error; 2 - q = 1 + eq is not representable, so eq enters as its own addend.  (The same 1e-8 in d Ph / d Pc scales the radial part by
    // 1 + 1e-8 / |Pc|; that part is ~1e-7 of the gradient to begin with.)
    const float eq = 2e-8f * ip;
    float rr = 0.f, gdot = 0.f, gs[3] = {0.f, 0.f, 0.f};
    for (int i = lane; i < n; i += 64) {
        float ph[3], xh[3], rp[3], g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { ph[k] = (P[i * 3 + k] - mp[k]) * ip; xh[k] = (X[i * 3 + k] - mx[k]) * ic; }
#pragma unroll
        for (int a = 0; a < 3; ++a) rp[a] = dot3(Rm[a], ph);
        const float r0 = __builtin_fmaf(s, rp[0], -xh[0]), r1 = __builtin_fmaf(s, rp[1], -xh[1]), r2 = __builtin_fmaf(s, rp[2], -xh[2]);
        rr += __builtin_fmaf(r2, r2, __builtin_fmaf(r1, r1, r0 * r0));
        if (aligned) {
#pragma unroll
            for (int k = 0; k < 3; ++k) aligned[((size_t)b * n + i) * 3 + k] = __builtin_fmaf(sc, rp[k], mx[k] + root[(size_t)b * 3 + k]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float rtx = __builtin_fmaf(Rm[2][k], xh[2], __builtin_fmaf(Rm[1][k], xh[1], Rm[0][k] * xh[0]));
            g[k] = kb * __builtin_fmaf(eq, rtx, __builtin_fmaf(-s, ph[k], rtx));
        }
        gdot += dot3(g, ph);
#pragma unroll
        for (int k = 0; k < 3; ++k) gs[k] += g[k];
    }
    rr = wave_sum(rr);
    if (lane == 0) sample_loss[b] = (cs * cs) * rr / (3.f * (float)n);
    if (!g_pred) return;
    gdot = wave_sum(gdot);
    float gm[3];                                                                  // mean of d loss / d Pc: sum g - gdot sum Ph, over p n
    float sph[3] = {0.f, 0.f, 0.f};
    for (int i = lane; i < n; i += 64)
#pragma unroll
        for (int k = 0; k < 3; ++k) sph[k] += (P[i * 3 + k] - mp[k]) * ip;
#pragma unroll
    for (int k = 0; k < 3; ++k) gm[k] = (wave_sum(gs[k]) - gdot * wave_sum(sph[k])) * ip * inv_n;
    for (int i = lane; i < n; i += 64) {
        float ph[3], xh[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { ph[k] = (P[i * 3 + k] - mp[k]) * ip; xh[k] = (X[i * 3 + k] - mx[k]) * ic; }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float rtx = __builtin_fmaf(Rm[2][k], xh[2], __builtin_fmaf(Rm[1][k], xh[1], Rm[0][k] * xh[0]));
            const float g = kb * __builtin_fmaf(eq, rtx, __builtin_fmaf(-s, ph[k], rtx));
            g_pred[((size_t)b * n + i) * 3 + k] = (g - gdot * ph[k]) * ip - gm[k];
        }
    }
}

// the batch mean of the per-sample losses: thread-serial, wave butterfly, waves in turn (block_sum4's order, spelled out: through the helper
// this one-column kernel measured slower, profiles/criterion_bodies.md)
__global__ __launch_bounds__(256) void procrustes_finalize_kernel(const float* __restrict__ sample_loss, int B, float* __restrict__ loss) {
    __shared__ float s_red[4];
    float a = 0.f;
    for (int b = threadIdx.x; b < B; b += 256) a += sample_loss[b];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = (((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) / (float)B;
}

extern "C" int ab_procrustes_loss(const float* pred, const float* targ, const float* root, int B, int n, float* sample_loss, float* loss,
                                  float* aligned, float* g_pred, void* stream) {
    if (!pred || !targ || !root || !sample_loss || !loss) return AB_EINVAL;
    if (B < 1 || n < 3 || n > (1 << 24)) return AB_EINVAL;
    const int per = PR_THREADS / 64;
    procrustes_kernel<<<(B + per - 1) / per, PR_THREADS, 0, as_stream(stream)>>>(pred, targ, root, B, n, sample_loss, aligned, g_pred);
    AB_LAUNCH_CHECK();
    procrustes_finalize_kernel<<<1, 256, 0, as_stream(stream)>>>(sample_loss, B, loss);
    AB_LAUNCH_CHECK();
    return 0;
}
