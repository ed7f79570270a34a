// VSD of bop_toolkit's pose_error.py for a whole batch (the other BOP error the evaluator lacked, MSPD, sits with MSSD
// in csrc/mssd.hip).
//
// ab_vsd: Visible Surface Discrepancy, fused so that no depth image reaches HBM unless asked for.  The stages are a contract (the header
//   has the full text; tests/bop_raster_ref.py restates it):
//   A  fp32, fixed order, no FMA: camera point ((r0 x + r1 y) + r2 z) + t, u = fx (X / Z) + cx, snap floorf(u 256 + 0.5); pixel (x, y) is
//      sampled AT (x, y) (BOP's depth_im_to_dist_im_fast), not at x + 1/2; a triangle is dropped when a vertex has Z <= VSD_NEAR or a snapped
//      coordinate outside +-VSD_RANGE; no back-face culling; zero-area triangles dropped.
//   B  int64 edge functions, top-left rule, as render.hip's cover().
//   C  float64: Z = 1 / ((l0 / Z0 + l1 / Z1) + l2 / Z2), l_i = (double)E_i / (double)A, rounded to fp32; visibility by an LDS atomicMin on
//      the bit pattern (positive floats order like unsigned integers): order-independent, so the image is the same on every call.
//   D  float64 per pixel in the order of depth_im_to_dist_im_fast, visibility._estimate_visib_mask (bop19) and vsd (cost_type "step"); only
//      integer counts leave a tile: per-tile partials in the workspace, a finalize launch, no global atomics.
// Launches: vsd_setup_kernel (project and snap the vertices of both poses and of the occluder into the workspace), vsd_tile_kernel (one
// workgroup per (sample, 32 x 32 tile): three LDS z-buffers, threads stride over the faces with a bounding-box reject, then stage D),
// vsd_finalize_kernel (one workgroup per sample).
#include "common.h"

#define VSD_TILE 32
#define VSD_THREADS 256
#define VSD_NEAR AB_VSD_NEAR            // metres: a triangle with a vertex at Z <= VSD_NEAR is dropped
#define VSD_RANGE AB_VSD_RANGE          // 1/256 px: a triangle with a snapped coordinate outside +-VSD_RANGE is dropped
#define VSD_EMPTY 0xffffffffu

struct VsdTaus { float v[AB_VSD_MAX_TAUS]; };

__device__ __forceinline__ int4 vsd_project(float X, float Y, float Z, float fx, float fy, float cx, float cy) {
    int4 r = make_int4(0, 0, __float_as_int(Z), 0);
    if (!(Z > VSD_NEAR)) return r;
    const float u = fx * (X / Z) + cx, v = fy * (Y / Z) + cy;
    const float su = floorf(u * 256.0f + 0.5f), sv = floorf(v * 256.0f + 0.5f);
    if (!(fabsf(su) <= (float)VSD_RANGE) || !(fabsf(sv) <= (float)VSD_RANGE)) return r;      // NaN and inf fail here too
    r.x = (int)su; r.y = (int)sv; r.w = 1;
    return r;
}

// rec: [B][2 Vmax + Nv] records (snapped x, snapped y, Z bits, valid): the object under the estimated pose, under the ground truth, the occluder
__global__ __launch_bounds__(256) void vsd_setup_kernel(const float* __restrict__ obj_verts, const int32_t* __restrict__ vert_off, int n_obj,
                                                        const int64_t* __restrict__ rows, const float* __restrict__ rot_est,
                                                        const float* __restrict__ tsl_est, const float* __restrict__ rot_gt,
                                                        const float* __restrict__ tsl_gt, const float* __restrict__ cam_intr,
                                                        const float* __restrict__ occ_verts, int Vmax, int Nv, int4* __restrict__ rec) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int per = 2 * Vmax + Nv;
    if (i >= per) return;
    const float* Kc = cam_intr + (size_t)b * 9;
    const float fx = Kc[0], fy = Kc[4], cx = Kc[2], cy = Kc[5];
    int4 r = make_int4(0, 0, 0, 0);
    if (i < 2 * Vmax) {
        const int64_t rr = rows[b];
        const int row = rr < 0 ? 0 : (rr >= n_obj ? n_obj - 1 : (int)rr);
        const int v = i < Vmax ? i : i - Vmax;
        const int nv = vert_off[row + 1] - vert_off[row];
        if (v < nv) {
            const float* R = (i < Vmax ? rot_est : rot_gt) + (size_t)b * 9;
            const float* t = (i < Vmax ? tsl_est : tsl_gt) + (size_t)b * 3;
            const float* q = obj_verts + ((size_t)vert_off[row] + v) * 3;
            const float x = q[0], y = q[1], z = q[2];
            const float X = ((R[0] * x + R[1] * y) + R[2] * z) + t[0];
            const float Y = ((R[3] * x + R[4] * y) + R[5] * z) + t[1];
            const float Z = ((R[6] * x + R[7] * y) + R[8] * z) + t[2];
            r = vsd_project(X, Y, Z, fx, fy, cx, cy);
        }
    } else {
        const float* q = occ_verts + ((size_t)b * Nv + (i - 2 * Vmax)) * 3;
        r = vsd_project(q[0], q[1], q[2], fx, fy, cx, cy);
    }
    rec[(size_t)b * per + i] = r;
}

__device__ __forceinline__ int64_t vsd_edge(int ax, int ay, int bx, int by, int px, int py) {
    return (int64_t)(bx - ax) * (py - ay) - (int64_t)(by - ay) * (px - ax);
}
__device__ __forceinline__ bool vsd_incl(int ax, int ay, int bx, int by) {
    const int dx = bx - ax, dy = by - ay;
    return (dy > 0) || (dy == 0 && dx < 0);
}

// One triangle into the tile's z-buffer(s).  tx0, ty0: the tile's origin; xe, ye: one past its last pixel inside the image.
__device__ __forceinline__ void vsd_raster(int4 a, int4 b, int4 c, int tx0, int ty0, int xe, int ye, unsigned* z0, unsigned* z1) {
    if (!(a.w & b.w & c.w)) return;
    int64_t area = (int64_t)(b.x - a.x) * (c.y - a.y) - (int64_t)(b.y - a.y) * (c.x - a.x);
    if (area == 0) return;
    if (area < 0) { const int4 t = b; b = c; c = t; area = -area; }
    const int minx = min(a.x, min(b.x, c.x)), maxx = max(a.x, max(b.x, c.x));
    const int miny = min(a.y, min(b.y, c.y)), maxy = max(a.y, max(b.y, c.y));
    const int x0 = max((minx + 255) >> 8, tx0), x1 = min(maxx >> 8, xe - 1);   // pixels whose sample x 256 lies inside [min, max]
    const int y0 = max((miny + 255) >> 8, ty0), y1 = min(maxy >> 8, ye - 1);
    if (x0 > x1 || y0 > y1) return;
    const bool i0 = vsd_incl(b.x, b.y, c.x, c.y), i1 = vsd_incl(c.x, c.y, a.x, a.y), i2 = vsd_incl(a.x, a.y, b.x, b.y);
    const double Za = (double)__int_as_float(a.z), Zb = (double)__int_as_float(b.z), Zc = (double)__int_as_float(c.z);
    const double Ad = (double)area;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            const int px = x * 256, py = y * 256;
            const int64_t e0 = vsd_edge(b.x, b.y, c.x, c.y, px, py), e1 = vsd_edge(c.x, c.y, a.x, a.y, px, py), e2 = vsd_edge(a.x, a.y, b.x, b.y, px, py);
            if (e0 < 0 || e1 < 0 || e2 < 0) continue;
            if ((e0 == 0 && !i0) || (e1 == 0 && !i1) || (e2 == 0 && !i2)) continue;
            const double l0 = (double)e0 / Ad, l1 = (double)e1 / Ad, l2 = (double)e2 / Ad;
            const double Z = 1.0 / ((l0 / Za + l1 / Zb) + l2 / Zc);
            const unsigned bits = __float_as_uint((float)Z);
            const int o = (y - ty0) * VSD_TILE + (x - tx0);
            atomicMin(&z0[o], bits);
            if (z1) atomicMin(&z1[o], bits);
        }
}

__device__ __forceinline__ double vsd_dist(float depth, double pX, double pY) {
    const double d = (double)depth;
    const double ax = pX * d, ay = pY * d;
    return sqrt((ax * ax + ay * ay) + d * d);
}

__global__ __launch_bounds__(VSD_THREADS) void vsd_tile_kernel(const int32_t* __restrict__ obj_faces, const int32_t* __restrict__ vert_off,
                                                               const int32_t* __restrict__ face_off, int n_obj,
                                                               const int64_t* __restrict__ rows, const float* __restrict__ cam_intr,
                                                               const float* __restrict__ depth_test, const int32_t* __restrict__ occ_faces,
                                                               int Vmax, int Nv, int Nf, int W, int H, float delta, VsdTaus taus, int T,
                                                               const float* __restrict__ diameter, int normalized,
                                                               const int4* __restrict__ rec, int32_t* __restrict__ part,
                                                               float* __restrict__ depth_out) {
    __shared__ unsigned zb[3][VSD_TILE * VSD_TILE];
    __shared__ int s_cnt[VSD_THREADS / 64][2 + AB_VSD_MAX_TAUS];
    const int b = blockIdx.y, tile = blockIdx.x, ntiles = gridDim.x;
    const int tiles_x = (W + VSD_TILE - 1) / VSD_TILE;
    const int tx0 = (tile % tiles_x) * VSD_TILE, ty0 = (tile / tiles_x) * VSD_TILE;
    const int xe = min(tx0 + VSD_TILE, W), ye = min(ty0 + VSD_TILE, H);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 3 * VSD_TILE * VSD_TILE; i += VSD_THREADS) (&zb[0][0])[i] = VSD_EMPTY;
    __syncthreads();
    const int64_t rr = rows[b];
    const int row = rr < 0 ? 0 : (rr >= n_obj ? n_obj - 1 : (int)rr);
    const int nv = min(vert_off[row + 1] - vert_off[row], Vmax);
    const int nf = max(face_off[row + 1] - face_off[row], 0);
    const int per = 2 * Vmax + Nv;
    const int4* rb = rec + (size_t)b * per;
    const bool occ = occ_faces != nullptr;
    const int items = 2 * nf + (occ ? Nf : 0);
    for (int it = threadIdx.x; it < items; it += VSD_THREADS) {
        if (it < 2 * nf) {
            const bool gt = it >= nf;
            const int32_t* f = obj_faces + ((size_t)face_off[row] + (gt ? it - nf : it)) * 3;
            const int a = f[0], bb = f[1], c = f[2];
            if ((unsigned)a >= (unsigned)nv || (unsigned)bb >= (unsigned)nv || (unsigned)c >= (unsigned)nv) continue;      // an index outside the mesh: dropped
            const int4* r = rb + (gt ? Vmax : 0);
            vsd_raster(r[a], r[bb], r[c], tx0, ty0, xe, ye, zb[gt ? 1 : 0], (gt && occ) ? zb[2] : nullptr);
        } else {
            const int32_t* f = occ_faces + (size_t)(it - 2 * nf) * 3;
            const int a = f[0], bb = f[1], c = f[2];
            if ((unsigned)a >= (unsigned)Nv || (unsigned)bb >= (unsigned)Nv || (unsigned)c >= (unsigned)Nv) continue;
            const int4* r = rb + 2 * Vmax;
            vsd_raster(r[a], r[bb], r[c], tx0, ty0, xe, ye, zb[2], nullptr);
        }
    }
    __syncthreads();
    // ---- stage D
    const float* Kc = cam_intr + (size_t)b * 9;
    const double fx = (double)Kc[0], fy = (double)Kc[4], cx = (double)Kc[2], cy = (double)Kc[5];
    const double diam = (double)diameter[row];
    int cnt[2 + AB_VSD_MAX_TAUS];
#pragma unroll
    for (int s = 0; s < 2 + AB_VSD_MAX_TAUS; ++s) cnt[s] = 0;
    for (int i = threadIdx.x; i < VSD_TILE * VSD_TILE; i += VSD_THREADS) {
        const int x = tx0 + (i & (VSD_TILE - 1)), y = ty0 + i / VSD_TILE;
        const bool in = x < W && y < H;
        bool uni = false, inter = false;
        double dd = 0.0;
        if (in) {
            const size_t pix = (size_t)y * W + x;
            const unsigned be = zb[0][i], bg = zb[1][i], bt = zb[2][i];
            const float de = be == VSD_EMPTY ? 0.f : __uint_as_float(be), dg = bg == VSD_EMPTY ? 0.f : __uint_as_float(bg);
            const float dm = depth_test ? depth_test[(size_t)b * W * H + pix] : 0.f;
            float dt = dm;
            if (occ) {                                                          // the scene a sensor would have seen: nearest of occluder, object, measurement
                dt = bt == VSD_EMPTY ? 0.f : __uint_as_float(bt);
                if (dm > 0.f && (dt == 0.f || dm < dt)) dt = dm;
            }
            if (depth_out) {
                float* o = depth_out + (size_t)b * 3 * W * H + pix;
                o[0] = de; o[(size_t)W * H] = dg; o[2 * (size_t)W * H] = dt;
            }
            const double pX = ((double)x - cx) / fx, pY = ((double)y - cy) / fy;
            const double Le = vsd_dist(de, pX, pY), Lg = vsd_dist(dg, pX, pY), Lt = vsd_dist(dt, pX, pY);
            const bool vg = (((float)Lg - (float)Lt <= delta) || Lt == 0.0) && Lg > 0.0;
            bool ve = (((float)Le - (float)Lt <= delta) || Lt == 0.0) && Le > 0.0;
            ve = ve || (vg && Le > 0.0);
            inter = vg && ve; uni = vg || ve;
            dd = fabs(Lg - Le);
            if (normalized) dd = dd / diam;
        }
        const unsigned long long mu = __ballot(uni), mc = __ballot(uni && !inter);
        cnt[0] += __popcll(mu); cnt[1] += __popcll(mc);
#pragma unroll
        for (int t = 0; t < AB_VSD_MAX_TAUS; ++t)
            if (t < T) cnt[2 + t] += __popcll(__ballot(inter && dd >= (double)taus.v[t]));      // t < T is uniform: every lane votes
    }
    if (lane == 0) {
#pragma unroll
        for (int s = 0; s < 2 + AB_VSD_MAX_TAUS; ++s) s_cnt[wave][s] = cnt[s];
    }
    __syncthreads();
    if (threadIdx.x < 2 + T) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < VSD_THREADS / 64; ++w) s += s_cnt[w][threadIdx.x];
        part[((size_t)b * ntiles + tile) * (2 + T) + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(64) void vsd_finalize_kernel(const int32_t* __restrict__ part, int ntiles, int T, int32_t* __restrict__ counts,
                                                          float* __restrict__ err) {
    __shared__ int s_tot[2 + AB_VSD_MAX_TAUS];
    const int b = blockIdx.x, s = threadIdx.x;
    if (s < 2 + T) {
        int tot = 0;
        for (int t = 0; t < ntiles; ++t) tot += part[((size_t)b * ntiles + t) * (2 + T) + s];
        s_tot[s] = tot;
        counts[(size_t)b * (2 + T) + s] = tot;
    }
    __syncthreads();
    if (s < T) {
        const int uni = s_tot[0], comp = s_tot[1];
        err[(size_t)b * T + s] = uni > 0 ? (float)((double)(s_tot[2 + s] + comp) / (double)uni) : 1.0f;
    }
}

static inline long vsd_rec_bytes(int B, int max_obj_verts, int Nv) { return (long)B * (2L * max_obj_verts + Nv) * 16L; }

extern "C" long ab_vsd_workspace(int B, int max_obj_verts, int Nv, int W, int H, int T) {
    if (B < 1 || max_obj_verts < 1 || Nv < 0 || W < 1 || H < 1 || T < 1) return 0;
    const long ntiles = (long)((W + VSD_TILE - 1) / VSD_TILE) * ((H + VSD_TILE - 1) / VSD_TILE);
    return vsd_rec_bytes(B, max_obj_verts, Nv) + (long)B * ntiles * (2 + T) * 4L;
}

extern "C" int ab_vsd(const float* obj_verts, const int32_t* obj_faces, const int32_t* vert_off, const int32_t* face_off, int n_obj,
                      int max_obj_verts, const int64_t* rows, const float* rot_est, const float* tsl_est, const float* rot_gt,
                      const float* tsl_gt, const float* cam_intr, int B, int W, int H, const float* depth_test, const float* occ_verts,
                      const int32_t* occ_faces, int Nv, int Nf, float delta, const float* taus_host, int T, const float* diameter,
                      int normalized_by_diameter, int32_t* counts, float* err, float* depth_out, void* workspace, void* stream) {
    if (!obj_verts || !obj_faces || !vert_off || !face_off || !rows || !rot_est || !tsl_est || !rot_gt || !tsl_gt || !cam_intr || !taus_host ||
        !diameter || !counts || !err || !workspace)
        return AB_EINVAL;
    if (B < 1 || B > 65535 || n_obj < 1 || max_obj_verts < 1 || W < 1 || H < 1 || W > 8192 || H > 8192 || T < 1 || T > AB_VSD_MAX_TAUS) return AB_EINVAL;
    if (!(delta >= 0.f)) return AB_EINVAL;
    if ((occ_verts != nullptr) != (occ_faces != nullptr)) return AB_EINVAL;
    if (occ_verts ? (Nv < 1 || Nf < 1) : (Nv != 0 || Nf != 0)) return AB_EINVAL;
    VsdTaus taus;
    for (int t = 0; t < AB_VSD_MAX_TAUS; ++t) taus.v[t] = t < T ? taus_host[t] : 0.f;
    const int ntiles = ((W + VSD_TILE - 1) / VSD_TILE) * ((H + VSD_TILE - 1) / VSD_TILE);
    int4* rec = (int4*)workspace;
    int32_t* part = (int32_t*)((char*)workspace + vsd_rec_bytes(B, max_obj_verts, Nv));
    const int per = 2 * max_obj_verts + Nv;
    vsd_setup_kernel<<<dim3((per + 255) / 256, B), 256, 0, as_stream(stream)>>>(obj_verts, vert_off, n_obj, rows, rot_est, tsl_est, rot_gt, tsl_gt,
                                                                                 cam_intr, occ_verts, max_obj_verts, Nv, rec);
    AB_LAUNCH_CHECK();
    vsd_tile_kernel<<<dim3(ntiles, B), VSD_THREADS, 0, as_stream(stream)>>>(obj_faces, vert_off, face_off, n_obj, rows, cam_intr, depth_test,
                                                                             occ_faces, max_obj_verts, Nv, Nf, W, H, delta, taus, T, diameter,
                                                                             normalized_by_diameter ? 1 : 0, rec, part, depth_out);
    AB_LAUNCH_CHECK();
    vsd_finalize_kernel<<<B, 64, 0, as_stream(stream)>>>(part, ntiles, T, counts, err);
    AB_LAUNCH_CHECK();
    return 0;
}
