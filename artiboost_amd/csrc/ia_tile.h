// The triangle primitive of ab_interaction (csrc/interact.hip) and ab_contact_loss (csrc/contact_loss.hip): one query per thread against a
// mesh whose triangles go through LDS in SoA tiles (nine coordinate arrays; one wave-uniform ds_read_b128 per array serves four triangles
// for 64 queries; a tile's tail repeats one vertex three times: solid angle 0, distance that of a point of the mesh).  Per triangle: the
// half solid angle atan2(num, den) into a compensated running sum, added in face order, and the closest point by the region form (vertex
// a, b, edge ab, vertex c, edge ac, edge bc, interior, the first that applies), every division guarded; cp - q = A + v (b - a) + w (c - a)
// is a sum of differences, squared lengths are compared under strict <: the first minimum in face order wins.  Both kernels call the same
// functions, so a distance has the same bits in both.  The definitions are those of the header of interact.hip.
#pragma once
#include "common.h"

#define IA_THREADS 256         // one query per thread
#define IA_TILE 512            // triangles staged per round: 9 x 512 floats = 18 KiB SoA
#define IA_TWO_PI 6.2831855f

__device__ __forceinline__ float ia_dot(float x0, float x1, float x2, float y0, float y1, float y2) {
    return __builtin_fmaf(x2, y2, __builtin_fmaf(x1, y1, x0 * y0));
}

// The half solid angle of one triangle (A, B, C relative to the query) into the compensated sum.
__device__ __forceinline__ void ia_half_angle(float Ax, float Ay, float Az, float Bx, float By, float Bz, float Cx, float Cy, float Cz, float& sum,
                                              float& comp) {
    const float la = sqrtf(ia_dot(Ax, Ay, Az, Ax, Ay, Az)), lb = sqrtf(ia_dot(Bx, By, Bz, Bx, By, Bz)), lc = sqrtf(ia_dot(Cx, Cy, Cz, Cx, Cy, Cz));
    const float num = ia_dot(Ax, Ay, Az, By * Cz - Bz * Cy, Bz * Cx - Bx * Cz, Bx * Cy - By * Cx);
    const float den = ((la * lb * lc + ia_dot(Ax, Ay, Az, Bx, By, Bz) * lc) + ia_dot(Bx, By, Bz, Cx, Cy, Cz) * la) + ia_dot(Cx, Cy, Cz, Ax, Ay, Az) * lb;
    const float half = (num == 0.f && den == 0.f) ? 0.f : atan2f(num, den);
    const float y = half - comp, t = sum + y;                                    // compensated: the sum of F terms rounds once
    comp = (t - sum) - y;
    sum = t;
}

// The closest point of one triangle by the region form: (rx, ry, rz) = cp - q, returns its squared length.
__device__ __forceinline__ float ia_closest(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz, float Ax, float Ay,
                                            float Az, float Bx, float By, float Bz, float Cx, float Cy, float Cz, float& rx, float& ry, float& rz) {
    const float e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
    const float d1 = -ia_dot(e1x, e1y, e1z, Ax, Ay, Az), d2 = -ia_dot(e2x, e2y, e2z, Ax, Ay, Az);
    const float d3 = -ia_dot(e1x, e1y, e1z, Bx, By, Bz), d4 = -ia_dot(e2x, e2y, e2z, Bx, By, Bz);
    const float d5 = -ia_dot(e1x, e1y, e1z, Cx, Cy, Cz), d6 = -ia_dot(e2x, e2y, e2z, Cx, Cy, Cz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    float nv = vb, nw = vc, dn = (va + vb) + vc;                                          // interior
    if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) { nv = e56; nw = e43; dn = e43 + e56; }   // edge bc
    if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { nv = 0.f; nw = d2; dn = d2 - d6; }        // edge ac
    if (d6 >= 0.f && d5 <= d6) { nv = 0.f; nw = 1.f; dn = 1.f; }                         // vertex c
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { nv = d1; nw = 0.f; dn = d1 - d3; }        // edge ab
    if (d3 >= 0.f && d4 <= d3) { nv = 1.f; nw = 0.f; dn = 1.f; }                         // vertex b
    if (d1 <= 0.f && d2 <= 0.f) { nv = 0.f; nw = 0.f; dn = 1.f; }                        // vertex a
    const bool ok = dn != 0.f;
    const float v = ok ? nv / dn : 0.f, w = ok ? nw / dn : 0.f;
    rx = __builtin_fmaf(w, e2x, __builtin_fmaf(v, e1x, Ax));
    ry = __builtin_fmaf(w, e2y, __builtin_fmaf(v, e1y, Ay));
    rz = __builtin_fmaf(w, e2z, __builtin_fmaf(v, e1z, Az));
    return ia_dot(rx, ry, rz, rx, ry, rz);
}

// One triangle against one query: the half solid angle into the compensated sum and, with DIST, the squared distance into the minimum.
template <bool DIST>
__device__ __forceinline__ void ia_tri(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz, float qx,
                                       float qy, float qz, float& sum, float& comp, float& best) {
    const float Ax = ax - qx, Ay = ay - qy, Az = az - qz;
    const float Bx = bx - qx, By = by - qy, Bz = bz - qz;
    const float Cx = cx - qx, Cy = cy - qy, Cz = cz - qz;
    ia_half_angle(Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz, sum, comp);
    if (DIST) {
        float rx, ry, rz;
        const float d = ia_closest(ax, ay, az, bx, by, bz, cx, cy, cz, Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz, rx, ry, rz);
        best = d < best ? d : best;
    }
}

// The running state of a query that keeps its closest point: the smallest squared distance with cp - q, and the compensated sum.
struct ia_hit { float best, rx, ry, rz, sum, comp; };

// One triangle against one query, the closest point kept with the minimum; with WIND also the half solid angle.
template <bool WIND>
__device__ __forceinline__ void ia_tri_cp(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz, float qx,
                                          float qy, float qz, ia_hit& h) {
    const float Ax = ax - qx, Ay = ay - qy, Az = az - qz;
    const float Bx = bx - qx, By = by - qy, Bz = bz - qz;
    const float Cx = cx - qx, Cy = cy - qy, Cz = cz - qz;
    if (WIND) ia_half_angle(Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz, h.sum, h.comp);
    float rx, ry, rz;
    const float d = ia_closest(ax, ay, az, bx, by, bz, cx, cy, cz, Ax, Ay, Az, Bx, By, Bz, Cx, Cy, Cz, rx, ry, rz);
    const bool lt = d < h.best;
    h.best = lt ? d : h.best; h.rx = lt ? rx : h.rx; h.ry = lt ? ry : h.ry; h.rz = lt ? rz : h.rz;
}

// Stages nf triangles (faces: indices local to verts, clamped into [0, nv)) tile by tile and calls tri(ax, ay, az, bx, ..., cz) for each in
// face order.  Every thread of the workgroup (IA_THREADS) calls it (barriers inside).  ts: 9 * IA_TILE floats of LDS, 16-byte aligned.
template <typename Tri>
__device__ __forceinline__ void ia_scan_tiles(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces, int nf, float* ts, Tri tri) {
    for (int f0 = 0; f0 < nf; f0 += IA_TILE) {
        const int n = min(IA_TILE, nf - f0);
        const int npad = (n + 3) & ~3;                                           // <= IA_TILE (a multiple of 4)
        __syncthreads();
        for (int j = threadIdx.x; j < npad; j += IA_THREADS) {
            const int32_t* fc = faces + (size_t)(f0 + (j < n ? j : 0)) * 3;
            const int i0 = min(max(fc[0], 0), nv - 1);
            const int i1 = j < n ? min(max(fc[1], 0), nv - 1) : i0, i2 = j < n ? min(max(fc[2], 0), nv - 1) : i0;   // the tail: one point three times
            const int idx[3] = {i0, i1, i2};
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int k = 0; k < 3; ++k) ts[(c * 3 + k) * IA_TILE + j] = verts[(size_t)idx[c] * 3 + k];
        }
        __syncthreads();
        for (int j = 0; j < npad; j += 4) {
            float t[9][4];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float4 x = *(const float4*)&ts[k * IA_TILE + j];
                t[k][0] = x.x; t[k][1] = x.y; t[k][2] = x.z; t[k][3] = x.w;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) tri(t[0][u], t[1][u], t[2][u], t[3][u], t[4][u], t[5][u], t[6][u], t[7][u], t[8][u]);
        }
    }
}

// Scans nf triangles for the calling workgroup's 256 queries: winding sum and, with DIST, the smallest squared distance.
template <bool DIST>
__device__ __forceinline__ void ia_scan(const float* __restrict__ verts, int nv, const int32_t* __restrict__ faces, int nf, float* ts, float qx,
                                        float qy, float qz, float& sum, float& comp, float& best) {
    ia_scan_tiles(verts, nv, faces, nf, ts, [&](float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
        ia_tri<DIST>(ax, ay, az, bx, by, bz, cx, cy, cz, qx, qy, qz, sum, comp, best);
    });
}

struct ia_object { const float* verts; const int32_t* faces; int nv, nf; float orient; float R[9], t[3]; };

__device__ __forceinline__ ia_object ia_load_object(const float* obj_verts, const int32_t* obj_faces, const int32_t* vert_off, const int32_t* face_off,
                                                    const float* obj_orient, int n_obj, const int64_t* obj_row, const float* rot, const float* tsl, int b) {
    ia_object o;
    const long r = (long)obj_row[b];
    const int row = (int)(r < 0 ? 0 : (r >= n_obj ? n_obj - 1 : r));             // clamped into the table
    const int v0 = vert_off[row], f0 = face_off[row];
    o.verts = obj_verts + (size_t)v0 * 3;
    o.faces = obj_faces + (size_t)f0 * 3;
    o.nv = max(vert_off[row + 1] - v0, 1);
    o.nf = max(face_off[row + 1] - f0, 0);
    o.orient = obj_orient[row];
#pragma unroll
    for (int k = 0; k < 9; ++k) o.R[k] = rot[(size_t)b * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.t[k] = tsl[(size_t)b * 3 + k];
    return o;
}

// q' = R^T (q - t)
__device__ __forceinline__ void ia_to_canonical(const ia_object& o, float qx, float qy, float qz, float& x, float& y, float& z) {
    const float d0 = qx - o.t[0], d1 = qy - o.t[1], d2 = qz - o.t[2];
    x = ia_dot(o.R[0], o.R[3], o.R[6], d0, d1, d2);
    y = ia_dot(o.R[1], o.R[4], o.R[7], d0, d1, d2);
    z = ia_dot(o.R[2], o.R[5], o.R[8], d0, d1, d2);
}
