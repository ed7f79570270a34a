// The two symmetry-set pose errors of the evaluator (DESIGN.md sections 21 and 25), each for a whole batch:
//   ab_mssd  anakin/metrics/bopAR.py:131-175 (MSSD.feed) and val_metric.py:272-320, the metric of AR and ValMetricAR2.  Per sample, with the
//            symmetry set S of the sample's object at its TRUE length (the BOP enumeration of a continuous symmetry does not contain the
//            identity),  mssd[b] = min over k < count of max over v < V of || R_gt (S_k.R can_v + S_k.t) + t_gt - pred_v - c_b ||.
//   ab_mspd  bop_toolkit's pose_error.py: min over the same set of max over the model points of || proj(pred_v) - proj(sym_k(gt)_v) || in
//            pixels.  A point with camera-space Z <= 0 in either pose makes the sample's error +inf (a projection behind the camera is not
//            a pixel).
// The frame is the same for both.  The torch expression materialises four [B, K, V, 3] temporaries; here a lane owns one symmetry and
// composes its 3x4 map once
//   MSSD rigid  (pred_v = R_pred can_v + t_pred):  A = R_gt S_k.R - R_pred,  a = R_gt S_k.t + t_gt - t_pred - c_b
//   MSSD points (pred_v read from memory):         A = R_gt S_k.R,           a = R_gt S_k.t + t_gt - c_b,   residual = (A can_v + a) - pred_v
//   MSPD (fixed order, no FMA: the rasteriser's camera point):  A = R_gt S_k.R,  a = R_gt S_k.t + t_gt
// and the sample's vertices go through LDS in SoA tiles: one wave-uniform (broadcast) ds_read_b128 serves four vertices for 64 symmetries.
// For MSPD the thread that stages a point also projects the PREDICTED point (the same for every symmetry), so the scan reads x, y, z, pu, pv.
// The four waves of a workgroup hold the SAME 64 symmetries and each takes a quarter of every tile, so a lane keeps a running maximum of
// the squared length with no cross-lane step in the loop; then a max across the waves through LDS, a wave min over the lanes with
// k < count, one partial per (sample, chunk of 64 symmetries) into the workspace and a second tiny launch for the min over the chunks and
// the one square root (sqrt is monotonic and correctly rounded: the bits equal the max of the roots).
// A vertex's residual is the same chain of operations wherever the vertex sits, and max / min do not depend on the order: the result
// is bit-identical across calls, across positions in the batch and under repetition padding of the vertices.  No atomics.
#include "common.h"

#define SYM_THREADS 256        // 4 waves, all on the same chunk of 64 symmetries; each scans a quarter of every staged tile
#define SYM_TILE 1024          // vertices staged per round: 12 KiB SoA (MSSD; 24 KiB with the predicted points), x y z | pu pv, 20 KiB (MSPD)

// the sample's row of the symmetry table (ids are 1-based; one outside the table is clamped into it); returns the size of its set
__device__ __forceinline__ int sym_lookup(const int64_t* obj_idx, const int32_t* sym_count, int n_obj, int Kmax, int b, int& obj) {
    const int64_t id = obj_idx[b] - 1;
    obj = id < 0 ? 0 : (id >= n_obj ? n_obj - 1 : (int)id);
    return min(max(sym_count[obj], 0), Kmax);
}

// a lane's maximum over its wave's quarters -> the workgroup's partial: max over the four waves, min over the members of the set
__device__ __forceinline__ void sym_partial(float (*s_max)[64], float best, int cnt, float* __restrict__ part) {
    const int b = blockIdx.y, chunk = blockIdx.x, nchunks = gridDim.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s_max[wave][lane] = best;
    __syncthreads();
    if (wave == 0) {
        float m = fmaxf(fmaxf(s_max[0][lane], s_max[1][lane]), fmaxf(s_max[2][lane], s_max[3][lane]));
        if (chunk * 64 + lane >= cnt) m = __builtin_inff();
        m = wave_min(m);
        if (lane == 0) part[(size_t)b * nchunks + chunk] = m;
    }
}

template <bool POINTS>
__global__ __launch_bounds__(SYM_THREADS) void mssd_kernel(const float* __restrict__ can, const float* __restrict__ obj_transf,
                                                           const int64_t* __restrict__ obj_idx, const float* __restrict__ sym_R,
                                                           const float* __restrict__ sym_t, const int32_t* __restrict__ sym_count,
                                                           int n_obj, int Kmax, const float* __restrict__ pred_R,
                                                           const float* __restrict__ pred_t, const float* __restrict__ pred_pts,
                                                           const float* __restrict__ center, int V, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float vs[(POINTS ? 6 : 3) * SYM_TILE];
    __shared__ float s_max[4][64];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int obj;
    const int cnt = sym_lookup(obj_idx, sym_count, n_obj, Kmax, b, obj);
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
    for (int v0 = 0; v0 < V; v0 += SYM_TILE) {
        const int n = min(SYM_TILE, V - v0);
        const int npad = (n + 15) & ~15;                                        // four waves x groups of four; <= SYM_TILE (a multiple of 16)
        __syncthreads();
        for (int j = threadIdx.x; j < npad; j += SYM_THREADS) {
            const size_t src = (size_t)(v0 + (j < n ? j : 0)) * 3;              // the tail repeats the tile's first vertex: the max is unchanged
            vs[j] = cb[src]; vs[SYM_TILE + j] = cb[src + 1]; vs[2 * SYM_TILE + j] = cb[src + 2];
            if (POINTS) { vs[3 * SYM_TILE + j] = pb[src]; vs[4 * SYM_TILE + j] = pb[src + 1]; vs[5 * SYM_TILE + j] = pb[src + 2]; }
        }
        __syncthreads();
        const int per = npad >> 2;                                              // this wave's quarter, a multiple of 4
        const int ja = wave * per, jb = ja + per;
        for (int j = ja; j < jb; j += 4) {
            const float4 x4 = *(const float4*)&vs[j], y4 = *(const float4*)&vs[SYM_TILE + j], z4 = *(const float4*)&vs[2 * SYM_TILE + j];
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
            float px[4] = {0.f, 0.f, 0.f, 0.f}, py[4] = {0.f, 0.f, 0.f, 0.f}, pz[4] = {0.f, 0.f, 0.f, 0.f};
            if (POINTS) {
                const float4 p = *(const float4*)&vs[3 * SYM_TILE + j], q = *(const float4*)&vs[4 * SYM_TILE + j], r = *(const float4*)&vs[5 * SYM_TILE + j];
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
    sym_partial(s_max, best, cnt, part);
}

template <bool POINTS>
__global__ __launch_bounds__(SYM_THREADS) void mspd_kernel(const float* __restrict__ can, const float* __restrict__ obj_transf,
                                                           const int64_t* __restrict__ obj_idx, const float* __restrict__ sym_R,
                                                           const float* __restrict__ sym_t, const int32_t* __restrict__ sym_count,
                                                           int n_obj, int Kmax, const float* __restrict__ pred_R,
                                                           const float* __restrict__ pred_t, const float* __restrict__ pred_pts,
                                                           const float* __restrict__ cam_intr, int V, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float vs[5 * SYM_TILE];
    __shared__ float s_max[4][64];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int obj;
    const int cnt = sym_lookup(obj_idx, sym_count, n_obj, Kmax, b, obj);
    if (chunk * 64 >= cnt) return;                                              // block-uniform
    const int k = min(chunk * 64 + lane, cnt - 1);                              // lanes past the count recompute the last member (masked below)
    const float* T = obj_transf + (size_t)b * 16;
    const float* SR = sym_R + ((size_t)obj * Kmax + k) * 9;
    const float* St = sym_t + ((size_t)obj * Kmax + k) * 3;
    const float* Kc = cam_intr + (size_t)b * 9;
    const float fx = Kc[0], fy = Kc[4], cx = Kc[2], cy = Kc[5];
    const float inf = __builtin_inff();
    float A[9], a[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float g0 = T[i * 4 + 0], g1 = T[i * 4 + 1], g2 = T[i * 4 + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) A[i * 3 + j] = (g0 * SR[j] + g1 * SR[3 + j]) + g2 * SR[6 + j];
        a[i] = ((g0 * St[0] + g1 * St[1]) + g2 * St[2]) + T[i * 4 + 3];
    }
    float P[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
    if (!POINTS) {
#pragma unroll
        for (int i = 0; i < 9; ++i) P[i] = pred_R[(size_t)b * 9 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) p[i] = pred_t[(size_t)b * 3 + i];
    }
    const float* cb = can + (size_t)b * V * 3;
    const float* pb = POINTS ? pred_pts + (size_t)b * V * 3 : nullptr;
    float best = 0.f;                                                           // squared pixel distances are >= 0
    for (int v0 = 0; v0 < V; v0 += SYM_TILE) {
        const int n = min(SYM_TILE, V - v0);
        const int npad = (n + 15) & ~15;                                        // four waves x groups of four; <= SYM_TILE
        __syncthreads();
        for (int j = threadIdx.x; j < npad; j += SYM_THREADS) {
            const size_t src = (size_t)(v0 + (j < n ? j : 0)) * 3;              // the tail repeats the tile's first point: the max is unchanged
            const float x = cb[src], y = cb[src + 1], z = cb[src + 2];
            float qx, qy, qz;
            if (POINTS) { qx = pb[src]; qy = pb[src + 1]; qz = pb[src + 2]; }
            else {
                qx = ((P[0] * x + P[1] * y) + P[2] * z) + p[0];
                qy = ((P[3] * x + P[4] * y) + P[5] * z) + p[1];
                qz = ((P[6] * x + P[7] * y) + P[8] * z) + p[2];
            }
            const bool ok = qz > 0.f;
            vs[j] = x; vs[SYM_TILE + j] = y; vs[2 * SYM_TILE + j] = z;
            vs[3 * SYM_TILE + j] = ok ? fx * (qx / qz) + cx : inf;              // a predicted point at or behind the camera: the sample is +inf
            vs[4 * SYM_TILE + j] = ok ? fy * (qy / qz) + cy : 0.f;
        }
        __syncthreads();
        const int per = npad >> 2;                                              // this wave's quarter, a multiple of 4
        const int ja = wave * per, jb = ja + per;
        for (int j = ja; j < jb; j += 4) {
            const float4 x4 = *(const float4*)&vs[j], y4 = *(const float4*)&vs[SYM_TILE + j], z4 = *(const float4*)&vs[2 * SYM_TILE + j];
            const float4 u4 = *(const float4*)&vs[3 * SYM_TILE + j], w4 = *(const float4*)&vs[4 * SYM_TILE + j];
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
            const float us[4] = {u4.x, u4.y, u4.z, u4.w}, ws[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float X = ((A[0] * xs[u] + A[1] * ys[u]) + A[2] * zs[u]) + a[0];
                const float Y = ((A[3] * xs[u] + A[4] * ys[u]) + A[5] * zs[u]) + a[1];
                const float Z = ((A[6] * xs[u] + A[7] * ys[u]) + A[8] * zs[u]) + a[2];
                const float du = (fx * (X / Z) + cx) - us[u], dv = (fy * (Y / Z) + cy) - ws[u];
                float d2 = du * du + dv * dv;
                if (!(Z > 0.f) || d2 != d2) d2 = inf;                           // behind the camera in the ground truth, or inf - inf
                best = fmaxf(best, d2);
            }
        }
    }
    sym_partial(s_max, best, cnt, part);
}

// the min over a sample's chunks and the one square root, for either error
__global__ __launch_bounds__(256) void sym_finalize_kernel(const float* __restrict__ part, const int64_t* __restrict__ obj_idx,
                                                           const int32_t* __restrict__ sym_count, int n_obj, int Kmax, int nchunks, int B,
                                                           float* __restrict__ err) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int obj;
    const int cnt = sym_lookup(obj_idx, sym_count, n_obj, Kmax, b, obj);
    const int used = (cnt + 63) >> 6;                                           // the chunks the first launch wrote; the rest is never read
    float m = __builtin_inff();                                                 // an empty set: +inf
    for (int c = 0; c < used; ++c) m = fminf(m, part[(size_t)b * nchunks + c]);
    err[b] = sqrtf(m);
}

static long sym_workspace(int B, int Kmax) { return B < 1 || Kmax < 1 ? 0 : (long)B * ((Kmax + 63) / 64) * (long)sizeof(float); }
extern "C" long ab_mssd_workspace(int B, int Kmax, int V) { (void)V; return sym_workspace(B, Kmax); }
extern "C" long ab_mspd_workspace(int B, int Kmax, int V) { (void)V; return sym_workspace(B, Kmax); }

typedef void (*sym_kernel_t)(const float*, const float*, const int64_t*, const float*, const float*, const int32_t*, int, int, const float*,
                             const float*, const float*, const float*, int, float*);

// Both entry points: the argument checks, the error's kernel over (chunks of 64 symmetries, samples), the finalize.  `last` is the kernel's
// own operand (MSSD: center, optional; MSPD: cam_intr).
static int sym_run(sym_kernel_t rigid, sym_kernel_t points, const float* can, const float* obj_transf, const int64_t* obj_idx,
                   const float* sym_R, const float* sym_t, const int32_t* sym_count, int n_obj, int Kmax, const float* pred_R,
                   const float* pred_t, const float* pred_pts, const float* last, int B, int V, float* err, void* workspace, void* stream) {
    if (!can || !obj_transf || !obj_idx || !sym_R || !sym_t || !sym_count || !err || !workspace) return AB_EINVAL;
    if (B < 1 || B > 65535 || V < 1 || n_obj < 1 || Kmax < 1) return AB_EINVAL;
    if (pred_pts ? (pred_R || pred_t) : (!pred_R || !pred_t)) return AB_EINVAL;   // points mode XOR rigid mode
    const int nchunks = (Kmax + 63) / 64;
    if (nchunks > 65535) return AB_EINVAL;
    float* part = (float*)workspace;
    (pred_pts ? points : rigid)<<<dim3(nchunks, B), SYM_THREADS, 0, as_stream(stream)>>>(can, obj_transf, obj_idx, sym_R, sym_t, sym_count, n_obj, Kmax,
                                                                                       pred_R, pred_t, pred_pts, last, V, part);
    AB_LAUNCH_CHECK();
    sym_finalize_kernel<<<(B + 255) / 256, 256, 0, as_stream(stream)>>>(part, obj_idx, sym_count, n_obj, Kmax, nchunks, B, err);
    AB_LAUNCH_CHECK();
    return 0;
}

extern "C" int ab_mssd(const float* can, const float* obj_transf, const int64_t* obj_idx, const float* sym_R, const float* sym_t,
                       const int32_t* sym_count, int n_obj, int Kmax, const float* pred_R, const float* pred_t, const float* pred_pts,
                       const float* center, int B, int V, float* mssd, void* workspace, void* stream) {
    return sym_run(mssd_kernel<false>, mssd_kernel<true>, can, obj_transf, obj_idx, sym_R, sym_t, sym_count, n_obj, Kmax, pred_R, pred_t, pred_pts,
                   center, B, V, mssd, workspace, stream);
}

extern "C" int ab_mspd(const float* can, const float* obj_transf, const int64_t* obj_idx, const float* sym_R, const float* sym_t,
                       const int32_t* sym_count, int n_obj, int Kmax, const float* pred_R, const float* pred_t, const float* pred_pts,
                       const float* cam_intr, int B, int V, float* mspd, void* workspace, void* stream) {
    if (!cam_intr) return AB_EINVAL;
    return sym_run(mspd_kernel<false>, mspd_kernel<true>, can, obj_transf, obj_idx, sym_R, sym_t, sym_count, n_obj, Kmax, pred_R, pred_t, pred_pts,
                   cam_intr, B, V, mspd, workspace, stream);
}

