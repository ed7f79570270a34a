// Leaderboard mesh metrics of the evaluator on the device, eager only:
//   ab_mesh_metrics   per sample, with P = pred[b] and G = targ[b] + root[b]: the paired errors (epe, ra_epe), the similarity alignment of P
//                     onto G (pa_epe, scale) and the two-way nearest-neighbour distances of P and of the aligned P' against G (their means --
//                     mean_gp is ADD-S -- and the precision / recall counts and F-scores per threshold).
//
// Stage 1 (AB_MM_PAIRED | AB_MM_PROCRUSTES), one wave per sample: procrustes_fit (csrc/procrustes.h), the solve ab_procrustes_loss calls
// too.  It leaves the similarity in the workspace as the numbers `aligned` is formed from there,
//   P'_i = fma(s c, R ((P_i - mean P) / p), mean(targ) + root),
// not as one folded 3x4 map: A P_i + t would subtract two half-metre vectors to get a centimetre one.  The paired sums are wave butterflies.
// Stage 2 (AB_MM_NN), one workgroup per (sample, pass, direction, chunk of 256 query points): pass 0 scans P against G, pass 1 (with
// AB_MM_PROCRUSTES) P' against G; the first ceil(N/256) chunks of a pass own points of the prediction and scan G, the other ceil(M/256) own
// points of G and scan the prediction.  The scan is nn_tile_scan (csrc/nn_tile.h), the one ab_chamfer_rigid runs, without the index: squared
// lengths compared, one square root per query at the end.  P' is the same chain wherever it is formed (query register, staged tile,
// stage 1), so every direction sees the same bits and no aligned [B,N,3] is written.  A chunk leaves its distance sum (wave butterfly, the
// four waves in turn) and its counts below each threshold (ballot + popcount) in the workspace.
// Stage 3, one thread per sample: adds the sample's chunks in turn, writes the means, the integer counts and the F-scores.
// No atomics of any kind; two calls give the same bits, and a sample's row, counts and distances do not depend on the batch around it.
#include "common.h"
#include "nn_tile.h"
#include "procrustes.h"

#define MM_THREADS 256         // one query point per thread
#define MM_TILE 1024           // scanned points staged per round: 12 KiB SoA
#define MM_PART 8              // words per (sample, chunk) partial: distance sum (float) | counts below threshold t (int32) [4] | unused [3]
#define MM_SIM 20              // floats per sample: mean P [3] | 1/p | R [9] | s c | mean(targ) + root [3] | unused [3]
#define MM_WAVES 4             // stage 1: four waves per workgroup, one sample each

struct mm_thresholds { float t[AB_MM_MAX_THRESHOLDS]; };

// P'_i from the sample's similarity record: the statements ab_procrustes_loss forms `aligned` with.
__device__ __forceinline__ void mm_align1(const float* sim, float p0, float p1, float p2, float& o0, float& o1, float& o2) {
    const float ph[3] = {(p0 - sim[0]) * sim[3], (p1 - sim[1]) * sim[3], (p2 - sim[2]) * sim[3]};
    o0 = __builtin_fmaf(sim[13], dot3(sim + 4, ph), sim[14]);
    o1 = __builtin_fmaf(sim[13], dot3(sim + 7, ph), sim[15]);
    o2 = __builtin_fmaf(sim[13], dot3(sim + 10, ph), sim[16]);
}

__device__ __forceinline__ float mm_len(float d0, float d1, float d2) { return sqrtf(__builtin_fmaf(d2, d2, __builtin_fmaf(d1, d1, d0 * d0))); }

// ---- stage 1: paired errors and the similarity, one wave per sample ---------------------------------------------------------------------------
__global__ __launch_bounds__(MM_WAVES * 64) void mesh_metrics_align_kernel(const float* __restrict__ pred, const float* __restrict__ targ,
                                                                             const float* __restrict__ root, int B, int n, int center_idx,
                                                                             int flags, float* __restrict__ rows, float* __restrict__ simws) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * MM_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;                                                          // wave-uniform; no barrier below
    const float* P = pred + (size_t)b * n * 3;
    const float* X = targ + (size_t)b * n * 3;
    float rt[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) rt[k] = root ? root[(size_t)b * 3 + k] : 0.f;
    float* row = rows + (size_t)b * AB_MM_ROW;
    float epe = ab_nan(), ra_epe = ab_nan(), pa_epe = ab_nan(), scale = ab_nan();
    if (flags & AB_MM_PAIRED) {
        float pc[3] = {0.f, 0.f, 0.f}, gc[3] = {0.f, 0.f, 0.f};
        if (center_idx >= 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { pc[k] = P[(size_t)center_idx * 3 + k]; gc[k] = X[(size_t)center_idx * 3 + k] + rt[k]; }
        }
        float a = 0.f, r = 0.f;
        for (int i = lane; i < n; i += 64) {
            float p[3], g[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) { p[k] = P[i * 3 + k]; g[k] = X[i * 3 + k] + rt[k]; }
            a += mm_len(p[0] - g[0], p[1] - g[1], p[2] - g[2]);
            r += mm_len((p[0] - pc[0]) - (g[0] - gc[0]), (p[1] - pc[1]) - (g[1] - gc[1]), (p[2] - pc[2]) - (g[2] - gc[2]));
        }
        epe = wave_sum(a) / (float)n;
        if (center_idx >= 0) ra_epe = wave_sum(r) / (float)n;
    }
    if (flags & AB_MM_PROCRUSTES) {
        pr_fit f;
        procrustes_fit(P, X, n, lane, f);
        float sim[MM_SIM];
        sim[0] = f.mp[0]; sim[1] = f.mp[1]; sim[2] = f.mp[2]; sim[3] = 1.f / f.p;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) sim[4 + a * 3 + k] = f.R[a][k];
        sim[13] = f.s * f.c;
#pragma unroll
        for (int k = 0; k < 3; ++k) sim[14 + k] = f.mx[k] + rt[k];
        sim[17] = sim[18] = sim[19] = 0.f;
        float a = 0.f;
        for (int i = lane; i < n; i += 64) {
            float q0, q1, q2;
            mm_align1(sim, P[i * 3], P[i * 3 + 1], P[i * 3 + 2], q0, q1, q2);
            a += mm_len(q0 - (X[i * 3] + rt[0]), q1 - (X[i * 3 + 1] + rt[1]), q2 - (X[i * 3 + 2] + rt[2]));
        }
        pa_epe = wave_sum(a) * (1.f / (float)n);
        scale = sim[13] * sim[3];                                                // tr Sigma / |Pc|^2 = s c / p
        if (lane == 0) {                                                         // every lane holds the same bits
#pragma unroll
            for (int k = 0; k < MM_SIM; ++k) simws[(size_t)b * MM_SIM + k] = sim[k];
        }
    }
    if (lane == 0) { row[AB_MM_EPE] = epe; row[AB_MM_RA_EPE] = ra_epe; row[AB_MM_PA_EPE] = pa_epe; row[AB_MM_SCALE] = scale; }
}

// ---- stage 2: the nearest-neighbour scans -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MM_THREADS) void mesh_metrics_scan_kernel(const float* __restrict__ pred, const float* __restrict__ targ,
                                                                        const float* __restrict__ root, int N, int M, int cx, int cy,
                                                                        mm_thresholds thr, int T, const float* __restrict__ simws,
                                                                        float* __restrict__ d_pg, float* __restrict__ d_gp,
                                                                        float* __restrict__ pa_d_pg, float* __restrict__ pa_d_gp,
                                                                        float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float vs[3 * MM_TILE];
    __shared__ float s_sum[4];
    __shared__ int s_cnt[4][AB_MM_MAX_THRESHOLDS];
    const int b = blockIdx.y, nchunks = gridDim.x;
    const int pass = (int)blockIdx.x / (cx + cy), chunk = (int)blockIdx.x - pass * (cx + cy);   // pass 1: the aligned prediction
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool own_p = chunk < cx;                                               // block-uniform: this chunk's queries are points of the prediction
    const int nq = own_p ? N : M, ns = own_p ? M : N;
    const int q = (own_p ? chunk : chunk - cx) * MM_THREADS + (int)threadIdx.x;
    const bool live = q < nq;
    float* dist = pass ? (own_p ? pa_d_pg : pa_d_gp) : (own_p ? d_pg : d_gp);
    float rt[3], sim[MM_SIM];
#pragma unroll
    for (int k = 0; k < 3; ++k) rt[k] = root ? root[(size_t)b * 3 + k] : 0.f;
#pragma unroll
    for (int k = 0; k < MM_SIM; ++k) sim[k] = pass ? simws[(size_t)b * MM_SIM + k] : 0.f;
    const float* pb = pred + (size_t)b * N * 3;
    const float* tb = targ + (size_t)b * M * 3;

    const int qc = live ? q : nq - 1;                                            // lanes past the end recompute the last point (masked below)
    float px, py, pz;
    if (own_p) {
        px = pb[(size_t)qc * 3]; py = pb[(size_t)qc * 3 + 1]; pz = pb[(size_t)qc * 3 + 2];
        if (pass) mm_align1(sim, px, py, pz, px, py, pz);
    } else {
        px = tb[(size_t)qc * 3] + rt[0]; py = tb[(size_t)qc * 3 + 1] + rt[1]; pz = tb[(size_t)qc * 3 + 2] + rt[2];
    }
    const nn_hit hit = nn_tile_scan<MM_TILE, MM_THREADS, false>(vs, ns, px, py, pz, [&](size_t src, float& a0, float& a1, float& a2) {
        if (own_p) { a0 = tb[src] + rt[0]; a1 = tb[src + 1] + rt[1]; a2 = tb[src + 2] + rt[2]; }
        else {
            a0 = pb[src]; a1 = pb[src + 1]; a2 = pb[src + 2];
            if (pass) mm_align1(sim, a0, a1, a2, a0, a1, a2);
        }
    });
    const float d = sqrtf(hit.d2);
    if (live && dist) dist[(size_t)b * nq + q] = d;
    const float a = wave_sum(live ? d : 0.f);
    int cnt[AB_MM_MAX_THRESHOLDS];
#pragma unroll
    for (int t = 0; t < AB_MM_MAX_THRESHOLDS; ++t) cnt[t] = t < T ? (int)__popcll(__ballot(live && d < thr.t[t])) : 0;
    if (lane == 0) {
        s_sum[wave] = a;
#pragma unroll
        for (int t = 0; t < AB_MM_MAX_THRESHOLDS; ++t) s_cnt[wave][t] = cnt[t];
    }
    __syncthreads();
    if (threadIdx.x < MM_PART) {
        const int k = threadIdx.x;
        float v = 0.f;
        if (k == 0) v = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        else if (k <= AB_MM_MAX_THRESHOLDS) v = __int_as_float(((s_cnt[0][k - 1] + s_cnt[1][k - 1]) + s_cnt[2][k - 1]) + s_cnt[3][k - 1]);
        part[((size_t)b * nchunks + blockIdx.x) * MM_PART + k] = v;
    }
}

// ---- stage 3: one thread per sample adds its chunks in turn -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_metrics_finalize_kernel(const float* __restrict__ part, int B, int N, int M, int cx, int cy,
                                                                    int passes, int T, int flags, float* __restrict__ rows,
                                                                    int32_t* __restrict__ counts) {
    const int b = blockIdx.x * 256 + (int)threadIdx.x;
    if (b >= B) return;
    float* row = rows + (size_t)b * AB_MM_ROW;
    if (!(flags & (AB_MM_PAIRED | AB_MM_PROCRUSTES))) row[AB_MM_EPE] = row[AB_MM_RA_EPE] = row[AB_MM_PA_EPE] = row[AB_MM_SCALE] = ab_nan();
    const int per = cx + cy;
    const float* p = part + (size_t)b * passes * per * MM_PART;
    for (int pass = 0; pass < 2; ++pass) {
        float mean[2] = {ab_nan(), ab_nan()};
        int cnt[2][AB_MM_MAX_THRESHOLDS] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        const bool have = pass < passes;                                         // passes = 0: no scan was asked for
        if (have) {
            for (int dir = 0; dir < 2; ++dir) {
                float a = 0.f;
                const int c0 = pass * per + (dir ? cx : 0), c1 = c0 + (dir ? cy : cx);
                for (int c = c0; c < c1; ++c) {
                    a += p[(size_t)c * MM_PART];
#pragma unroll
                    for (int t = 0; t < AB_MM_MAX_THRESHOLDS; ++t) cnt[dir][t] += __float_as_int(p[(size_t)c * MM_PART + 1 + t]);
                }
                mean[dir] = a / (float)(dir ? M : N);
            }
        }
        row[pass ? AB_MM_PA_MEAN_PG : AB_MM_MEAN_PG] = mean[0];
        row[pass ? AB_MM_PA_MEAN_GP : AB_MM_MEAN_GP] = mean[1];
#pragma unroll
        for (int t = 0; t < AB_MM_MAX_THRESHOLDS; ++t) {
            float f = ab_nan();
            if (have && t < T) {
                const float pr = (float)cnt[0][t] / (float)N, rc = (float)cnt[1][t] / (float)M;
                f = pr + rc > 0.f ? 2.f * pr * rc / (pr + rc) : 0.f;
            }
            row[(pass ? AB_MM_PA_F : AB_MM_F) + t] = f;
            if (t < T) { counts[((size_t)b * T + t) * 4 + pass * 2] = cnt[0][t]; counts[((size_t)b * T + t) * 4 + pass * 2 + 1] = cnt[1][t]; }
        }
    }
}

static inline long mm_chunks(int N, int M) { return ((long)N + MM_THREADS - 1) / MM_THREADS + ((long)M + MM_THREADS - 1) / MM_THREADS; }

extern "C" long ab_mesh_metrics_workspace(int B, int N, int M) {
    if (B < 1 || N < 1 || M < 1) return 0;
    return (long)B * (MM_SIM + 2 * mm_chunks(N, M) * MM_PART) * (long)sizeof(float);
}

extern "C" int ab_mesh_metrics(const float* pred, const float* targ, const float* root, int B, int N, int M, int center_idx,
                               const float* thresholds_host, int T, int flags, float* rows, int32_t* counts, float* d_pg, float* d_gp,
                               float* pa_d_pg, float* pa_d_gp, void* workspace, void* stream) {
    if (!pred || !targ || !rows || !workspace) return AB_EINVAL;
    if (B < 1 || B > 65535 || N < 1 || M < 1 || N > (1 << 24) || M > (1 << 24)) return AB_EINVAL;
    if (T < 0 || T > AB_MM_MAX_THRESHOLDS || (T > 0 && (!thresholds_host || !counts))) return AB_EINVAL;
    if (!(flags & (AB_MM_PAIRED | AB_MM_PROCRUSTES | AB_MM_NN)) || (flags & ~(AB_MM_PAIRED | AB_MM_PROCRUSTES | AB_MM_NN))) return AB_EINVAL;
    if ((flags & (AB_MM_PAIRED | AB_MM_PROCRUSTES)) && N != M) return AB_EINVAL;
    if ((flags & AB_MM_PROCRUSTES) && N < 3) return AB_EINVAL;
    if (center_idx >= N) return AB_EINVAL;
    if (center_idx < 0) center_idx = -1;
    mm_thresholds thr;
    for (int t = 0; t < AB_MM_MAX_THRESHOLDS; ++t) thr.t[t] = t < T ? thresholds_host[t] : 0.f;
    const int cx = (N + MM_THREADS - 1) / MM_THREADS, cy = (M + MM_THREADS - 1) / MM_THREADS;
    const int passes = (flags & AB_MM_NN) ? ((flags & AB_MM_PROCRUSTES) ? 2 : 1) : 0;
    float* simws = (float*)workspace;
    float* part = simws + (size_t)B * MM_SIM;
    if (flags & (AB_MM_PAIRED | AB_MM_PROCRUSTES)) {
        mesh_metrics_align_kernel<<<(B + MM_WAVES - 1) / MM_WAVES, MM_WAVES * 64, 0, as_stream(stream)>>>(pred, targ, root, B, N, center_idx, flags,
                                                                                                         rows, simws);
        AB_LAUNCH_CHECK();
    }
    if (passes) {
        mesh_metrics_scan_kernel<<<dim3(passes * (cx + cy), B), MM_THREADS, 0, as_stream(stream)>>>(pred, targ, root, N, M, cx, cy, thr, T, simws, d_pg,
                                                                                                     d_gp, pa_d_pg, pa_d_gp, part);
        AB_LAUNCH_CHECK();
    }
    mesh_metrics_finalize_kernel<<<(B + 255) / 256, 256, 0, as_stream(stream)>>>(part, B, N, M, cx, cy, passes, T, flags, rows, counts);
    AB_LAUNCH_CHECK();
    return 0;
}
