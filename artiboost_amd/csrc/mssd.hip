// Maximum symmetry-aware surface distance of the evaluator:
//   anakin/metrics/bopAR.py:131-175 (MSSD.feed) and val_metric.py:272-320, the metric of AR and ValMetricAR2.  Per sample, with the
//   symmetry set S of the sample's object at its TRUE length (the BOP enumeration of a continuous symmetry does not contain the identity),
//     mssd[b] = min over k < count of max over v < V of || R_gt (S_k.R can_v + S_k.t) + t_gt - pred_v - c_b ||.
// The torch expression materialises four [B, K, V, 3] temporaries; here a lane owns one symmetry and composes its 3x4 residual map once
//   rigid  (pred_v = R_pred can_v + t_pred):  A = R_gt S_k.R - R_pred,  a = R_gt S_k.t + t_gt - t_pred - c_b
//   points (pred_v read from memory):         A = R_gt S_k.R,           a = R_gt S_k.t + t_gt - c_b,   residual = (A can_v + a) - pred_v
// and the sample's vertices go through LDS in SoA tiles: one wave-uniform (broadcast) ds_read_b128 serves four vertices for 64 symmetries.
// The four waves of a workgroup hold the SAME 64 symmetries and each takes a quarter of every tile, so a lane keeps a running maximum of
// the squared length with no cross-lane step in the loop; then a max across the waves through LDS, a wave min over the lanes with
// k < count, one partial per (sample, chunk of 64 symmetries) into the workspace and a second tiny launch for the min over the chunks and
// the one square root (sqrt is monotonic and correctly rounded: the bits equal the max of the roots).
// A vertex's residual is the same fused-multiply-add chain wherever the vertex sits, and max / min do not depend on the order: the result
// is bit-identical across calls, across positions in the batch and under repetition padding of the vertices.  No atomics.
#include "common.h"

#define MSSD_THREADS 256       // 4 waves, all on the same chunk of 64 symmetries; each scans a quarter of every staged tile
#define MSSD_TILE 1024         // vertices staged per round: 12 KiB SoA (24 KiB with the predicted points)

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

template <bool POINTS>
__global__ __launch_bounds__(MSSD_THREADS) void mssd_kernel(const float* __restrict__ can, const float* __restrict__ obj_transf,
                                                            const int64_t* __restrict__ obj_idx, const float* __restrict__ sym_R,
                                                            const float* __restrict__ sym_t, const int32_t* __restrict__ sym_count,
                                                            int n_obj, int Kmax, const float* __restrict__ pred_R,
                                                            const float* __restrict__ pred_t, const float* __restrict__ pred_pts,
                                                            const float* __restrict__ center, int V, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float vs[(POINTS ? 6 : 3) * MSSD_TILE];
    __shared__ float s_max[4][64];
    const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t id = obj_idx[b] - 1;                                           // 1-based; an id outside the table is clamped into it
    const int obj = id < 0 ? 0 : (id >= n_obj ? n_obj - 1 : (int)id);
    const int cnt = min(max(sym_count[obj], 0), Kmax);
    if (chunk * 64 >= cnt) return;                                              // block-uniform: nothing of this chunk is in the set
    const int k = min(chunk * 64 + lane, cnt - 1);                              // lanes past the count recompute the last member (masked below)
    const float* T = obj_transf + (size_t)b * 16;
    const float* SR = sym_R + ((size_t)obj * Kmax + k) * 9;
    const float* St = sym_t + ((size_t)obj * Kmax + k) * 3;
    float A[9], a[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float g0 = T[i * 4 + 0], g1 = T[i * 4 + 1], g2 = T[i * 4 + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float m = __builtin_fmaf(g2, SR[6 + j], __builtin_fmaf(g1, SR[3 + j], g0 * SR[j]));
            if (!POINTS) m -= pred_R[(size_t)b * 9 + i * 3 + j];
            A[i * 3 + j] = m;
        }
        float t = __builtin_fmaf(g2, St[2], __builtin_fmaf(g1, St[1], g0 * St[0])) + T[i * 4 + 3];
        if (!POINTS) t -= pred_t[(size_t)b * 3 + i];
        if (center) t -= center[(size_t)b * 3 + i];
        a[i] = t;
    }
    const float* cb = can + (size_t)b * V * 3;
    const float* pb = POINTS ? pred_pts + (size_t)b * V * 3 : nullptr;
    float best = 0.f;                                                           // squared lengths are >= 0
    for (int v0 = 0; v0 < V; v0 += MSSD_TILE) {
        const int n = min(MSSD_TILE, V - v0);
        const int npad = (n + 15) & ~15;                                        // four waves x groups of four; <= MSSD_TILE (a multiple of 16)
        __syncthreads();
        for (int j = threadIdx.x; j < npad; j += MSSD_THREADS) {
            const size_t src = (size_t)(v0 + (j < n ? j : 0)) * 3;              // the tail repeats the tile's first vertex: the max is unchanged
            vs[j] = cb[src]; vs[MSSD_TILE + j] = cb[src + 1]; vs[2 * MSSD_TILE + j] = cb[src + 2];
            if (POINTS) { vs[3 * MSSD_TILE + j] = pb[src]; vs[4 * MSSD_TILE + j] = pb[src + 1]; vs[5 * MSSD_TILE + j] = pb[src + 2]; }
        }
        __syncthreads();
        const int per = npad >> 2;                                              // this wave's quarter, a multiple of 4
        const int ja = wave * per, jb = ja + per;
        for (int j = ja; j < jb; j += 4) {
            const float4 x4 = *(const float4*)&vs[j], y4 = *(const float4*)&vs[MSSD_TILE + j], z4 = *(const float4*)&vs[2 * MSSD_TILE + j];
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
            float px[4] = {0.f, 0.f, 0.f, 0.f}, py[4] = {0.f, 0.f, 0.f, 0.f}, pz[4] = {0.f, 0.f, 0.f, 0.f};
            if (POINTS) {
                const float4 p = *(const float4*)&vs[3 * MSSD_TILE + j], q = *(const float4*)&vs[4 * MSSD_TILE + j], r = *(const float4*)&vs[5 * MSSD_TILE + j];
                px[0] = p.x; px[1] = p.y; px[2] = p.z; px[3] = p.w;
                py[0] = q.x; py[1] = q.y; py[2] = q.z; py[3] = q.w;
                pz[0] = r.x; pz[1] = r.y; pz[2] = r.z; pz[3] = r.w;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float rx = __builtin_fmaf(A[2], zs[u], __builtin_fmaf(A[1], ys[u], __builtin_fmaf(A[0], xs[u], a[0])));
                float ry = __builtin_fmaf(A[5], zs[u], __builtin_fmaf(A[4], ys[u], __builtin_fmaf(A[3], xs[u], a[1])));
                float rz = __builtin_fmaf(A[8], zs[u], __builtin_fmaf(A[7], ys[u], __builtin_fmaf(A[6], xs[u], a[2])));
                if (POINTS) { rx -= px[u]; ry -= py[u]; rz -= pz[u]; }
                best = fmaxf(best, __builtin_fmaf(rz, rz, __builtin_fmaf(ry, ry, rx * rx)));
            }
        }
    }
    s_max[wave][lane] = best;
    __syncthreads();
    if (wave == 0) {
        float m = fmaxf(fmaxf(s_max[0][lane], s_max[1][lane]), fmaxf(s_max[2][lane], s_max[3][lane]));
        if (chunk * 64 + lane >= cnt) m = __builtin_inff();
        m = wave_min(m);
        if (lane == 0) part[(size_t)b * nchunks + chunk] = m;
    }
}

__global__ __launch_bounds__(256) void mssd_finalize_kernel(const float* __restrict__ part, const int64_t* __restrict__ obj_idx,
                                                            const int32_t* __restrict__ sym_count, int n_obj, int Kmax, int nchunks, int B,
                                                            float* __restrict__ mssd) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int64_t id = obj_idx[b] - 1;
    const int obj = id < 0 ? 0 : (id >= n_obj ? n_obj - 1 : (int)id);
    const int cnt = min(max(sym_count[obj], 0), Kmax);
    const int used = (cnt + 63) >> 6;                                           // the chunks the first launch wrote; the rest is never read
    float m = __builtin_inff();                                                 // an empty set: +inf
    for (int c = 0; c < used; ++c) m = fminf(m, part[(size_t)b * nchunks + c]);
    mssd[b] = sqrtf(m);
}

extern "C" long ab_mssd_workspace(int B, int Kmax, int V) {
    (void)V;
    if (B < 1 || Kmax < 1) return 0;
    return (long)B * ((Kmax + 63) / 64) * (long)sizeof(float);
}

extern "C" int ab_mssd(const float* can, const float* obj_transf, const int64_t* obj_idx, const float* sym_R, const float* sym_t,
                       const int32_t* sym_count, int n_obj, int Kmax, const float* pred_R, const float* pred_t, const float* pred_pts,
                       const float* center, int B, int V, float* mssd, void* workspace, void* stream) {
    if (!can || !obj_transf || !obj_idx || !sym_R || !sym_t || !sym_count || !mssd || !workspace) return AB_EINVAL;
    if (B < 1 || B > 65535 || V < 1 || n_obj < 1 || Kmax < 1) return AB_EINVAL;
    if (pred_pts ? (pred_R || pred_t) : (!pred_R || !pred_t)) return AB_EINVAL;   // points mode XOR rigid mode
    const int nchunks = (Kmax + 63) / 64;
    if (nchunks > 65535) return AB_EINVAL;
    const dim3 grid(nchunks, B);
    float* part = (float*)workspace;
    if (pred_pts)
        mssd_kernel<true><<<grid, MSSD_THREADS, 0, as_stream(stream)>>>(can, obj_transf, obj_idx, sym_R, sym_t, sym_count, n_obj, Kmax, pred_R,
                                                                         pred_t, pred_pts, center, V, part);
    else
        mssd_kernel<false><<<grid, MSSD_THREADS, 0, as_stream(stream)>>>(can, obj_transf, obj_idx, sym_R, sym_t, sym_count, n_obj, Kmax, pred_R,
                                                                          pred_t, pred_pts, center, V, part);
    AB_LAUNCH_CHECK();
    mssd_finalize_kernel<<<(B + 255) / 256, 256, 0, as_stream(stream)>>>(part, obj_idx, sym_count, n_obj, Kmax, nchunks, B, mssd);
    AB_LAUNCH_CHECK();
    return 0;
}
