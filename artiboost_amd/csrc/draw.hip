// Qualitative drawings of the submission pass (`--postprocess_draw`): for every sample of a batch, two views of "fitted hand mesh +
// posed object mesh" written into panels 2 and 3 of a uint8 contact sheet [B, H, 4W, 3].  Replaces, for the meshes, the reference's
//   anakin/viztools/opendr_renderer.py (OpenDR, three Lambertian point lights) and viztools/draw.py:236-276 (mayavi, off-screen X)
// which draw one sample at a time on the host.  The reference's pixels cannot be produced without those packages and a display; this
// file DEFINES the pixels of this build and tests/draw_oracle.py restates them in float64 / integers.
//
// Four launches per batch, no floating-point atomics (bit-identical from run to run):
//   draw_bbox_kernel    one workgroup per sample: bounding box of hand + posed object -> the orbit camera's position
//   draw_vertex_kernel  one thread per vertex: position, gathered area-weighted normal, three-light Lambert colour, and for BOTH views the
//                       screen position snapped to 1/256 px, the 24-bit inverse depth and the view depth -> a 48-byte record
//   draw_raster_kernel  one thread per (face, view): integer edge functions over the face's pixel box (the conventions of render.hip /
//                       oracle/render_oracle.c: pixel centres at +0.5, the same shared-edge rule), atomicMin of depth << 32 | face on a
//                       u64 key per pixel (integer, order-independent)
//   draw_resolve_kernel one thread per pixel: winning face -> perspective-correct colour, or the frame / white
// Bounds: the vertex stage is ~60 flops per vertex; the raster stage is bounded by the summed pixel boxes of the faces (a few pixels per face
// for a 10^4-face object in a 256^2 panel) and the key traffic, B * 2 * H * W * 8 bytes written once and read once.
#include "common.h"
#include <math.h>

#define DRAW_HAND_VERTS 778
#define DRAW_REC_WORDS 12           // int32 words per vertex record (DrawRec)
#define DRAW_NEAR 0.01f             // a face with a vertex at or behind z = DRAW_NEAR (view space) is dropped whole
#define DRAW_NEAR_INV 100.0f
#define DRAW_FAR_INV 0.01f
#define DRAW_ZMAX 16777215.0f
#define DRAW_XY_LIMIT 32768.0f      // |screen x|, |y| at or beyond this many pixels: the vertex is unusable, its faces are dropped
#define DRAW_AREA_LIMIT ((int64_t)1 << 39)   // doubled area in (1/256 px)^2; keeps sum(w_k z_k) < 2^63
#define DRAW_OBJ_BOX (-2)           // obj_id: the 12-triangle box over the sample's 8 corners; -1: no object

struct DrawRec {                    // 48 bytes; view 0 = the sample's camera, view 1 = the orbit camera
    int32_t sx0, sy0; uint32_t zq0; int32_t sx1, sy1; uint32_t zq1;
    float zv0, zv1, r, g, b; uint32_t flags;      // flags bit v: usable in view v
};
struct DrawCam { float pos[3]; float pad; };      // orbit camera position per sample

// Orbit camera (mayavi's view(azimuth=-50, elevation=50, distance=0.6), view angle 30 degrees), rows of the world -> view rotation.
// u = (sin el cos az, sin el sin az, cos el); position = centre + 0.6 u; forward f = -u; world up = +z;
// right r = normalize(f x up); down d = f x r.  Filled by the host entry point in double precision, rounded once to float.
struct DrawView { float r[3], d[3], f[3], off[3], focal; };

struct DrawArgs {
    const float* hand_verts; const int32_t* hand_faces; int nhf; const int32_t* adj_off; const int32_t* adj_face; int nadj;
    const float* obj_verts; const float* obj_normals; const int32_t* obj_faces; const int32_t* obj_vert_off; const int32_t* obj_face_off;
    int n_obj, nov, nof, max_obj_verts;
    const int32_t* obj_id; const float* obj_rot; const float* obj_tsl; const float* corners; const float* cam_intr; const float* image;
    int B, W, H, VP;
    DrawRec* rec; DrawCam* cam; unsigned long long* keys; uint8_t* out;
    DrawView view;
    float light[3][3];
};

// the box over 8 corners indexed 4 ix + 2 iy + iz, outward winding for a right-handed box
__constant__ int8_t c_box_faces[12][3] = {{0, 1, 3}, {0, 3, 2}, {4, 6, 7}, {4, 7, 5}, {0, 4, 5}, {0, 5, 1},
                                          {2, 3, 7}, {2, 7, 6}, {0, 2, 6}, {0, 6, 4}, {1, 5, 7}, {1, 7, 3}};

// number of object vertices / faces of sample b and where they start; obj < 0: none (box: 8 / 12)
__device__ __forceinline__ void draw_obj_range(const DrawArgs& a, int b, int& oid, int& v0, int& nv, int& f0, int& nf) {
    oid = a.obj_id ? a.obj_id[b] : -1;
    v0 = nv = f0 = nf = 0;
    if (oid == DRAW_OBJ_BOX && a.corners) { nv = 8; nf = 12; return; }
    if (oid < 0 || oid >= a.n_obj || !a.obj_verts || !a.obj_faces || !a.obj_normals) { oid = -1; return; }
    v0 = a.obj_vert_off[oid]; nv = a.obj_vert_off[oid + 1] - v0;
    f0 = a.obj_face_off[oid]; nf = a.obj_face_off[oid + 1] - f0;
    if (v0 < 0 || nv < 0 || v0 + nv > a.nov || f0 < 0 || nf < 0 || f0 + nf > a.nof) { oid = -1; v0 = nv = f0 = nf = 0; return; }
    if (nv > a.max_obj_verts) nv = a.max_obj_verts;        // the record pitch bounds what can be addressed; faces beyond it are dropped
}

__device__ __forceinline__ void draw_obj_point(const DrawArgs& a, int b, int oid, int v0, int i, float P[3]) {
    if (oid == DRAW_OBJ_BOX) {
        const float* c = a.corners + ((size_t)b * 8 + i) * 3;
        P[0] = c[0]; P[1] = c[1]; P[2] = c[2];
        return;
    }
    const float* p = a.obj_verts + (size_t)(v0 + i) * 3;
    const float* R = a.obj_rot + (size_t)b * 9;
    const float* t = a.obj_tsl + (size_t)b * 3;
    P[0] = (R[0] * p[0] + R[1] * p[1]) + (R[2] * p[2] + t[0]);
    P[1] = (R[3] * p[0] + R[4] * p[1]) + (R[5] * p[2] + t[1]);
    P[2] = (R[6] * p[0] + R[7] * p[1]) + (R[8] * p[2] + t[2]);
}

// ------------------------------------------------------------------ kernel 1: bounding box -> orbit camera position
__global__ __launch_bounds__(256) void draw_bbox_kernel(DrawArgs a) {
    const int b = blockIdx.x;
    int oid, v0, nv, f0, nf;
    draw_obj_range(a, b, oid, v0, nv, f0, nf);
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < DRAW_HAND_VERTS + nv; i += 256) {
        float P[3];
        if (i < DRAW_HAND_VERTS) {
            const float* p = a.hand_verts + ((size_t)b * DRAW_HAND_VERTS + i) * 3;
            P[0] = p[0]; P[1] = p[1]; P[2] = p[2];
        } else draw_obj_point(a, b, oid, v0, i - DRAW_HAND_VERTS, P);
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], P[k]); hi[k] = fmaxf(hi[k], P[k]); }
    }
    __shared__ float s_lo[4][3], s_hi[4][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], o, 64)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o, 64)); }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { s_lo[threadIdx.x >> 6][k] = lo[k]; s_hi[threadIdx.x >> 6][k] = hi[k]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        const float l = fminf(fminf(s_lo[0][k], s_lo[1][k]), fminf(s_lo[2][k], s_lo[3][k]));
        const float h = fmaxf(fmaxf(s_hi[0][k], s_hi[1][k]), fmaxf(s_hi[2][k], s_hi[3][k]));
        a.cam[b].pos[k] = (l + h) * 0.5f + a.view.off[k];
    }
    if (threadIdx.x == 3) a.cam[b].pad = 0.f;
}

// ------------------------------------------------------------------ kernel 2: vertex stage
__device__ __forceinline__ void draw_cross_acc(const float A[3], const float Bv[3], const float C[3], float n[3]) {
    const float e1[3] = {Bv[0] - A[0], Bv[1] - A[1], Bv[2] - A[2]}, e2[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    n[0] += e1[1] * e2[2] - e1[2] * e2[1];
    n[1] += e1[2] * e2[0] - e1[0] * e2[2];
    n[2] += e1[0] * e2[1] - e1[1] * e2[0];
}
__device__ __forceinline__ int32_t draw_snap(float x) { return (int32_t)floorf(x * 256.0f + 0.5f); }
__device__ __forceinline__ uint32_t draw_quant_z(float Z) {
    const float inv = 1.0f / Z;
    const float z01 = (inv - DRAW_NEAR_INV) / (DRAW_FAR_INV - DRAW_NEAR_INV);
    float q = floorf(z01 * DRAW_ZMAX + 0.5f);
    if (q < 0.f) q = 0.f;
    if (q > DRAW_ZMAX) q = DRAW_ZMAX;
    return (uint32_t)q;
}
__device__ __forceinline__ bool draw_project(float fx, float fy, float cx, float cy, float X, float Y, float Z, int32_t& sx, int32_t& sy,
                                             uint32_t& zq) {
    sx = sy = 0; zq = 0;
    if (!(Z > DRAW_NEAR)) return false;
    const float x = (fx * X) / Z + cx, y = (fy * Y) / Z + cy;
    if (!(fabsf(x) < DRAW_XY_LIMIT) || !(fabsf(y) < DRAW_XY_LIMIT)) return false;
    sx = draw_snap(x); sy = draw_snap(y); zq = draw_quant_z(Z);
    return true;
}

__global__ __launch_bounds__(256) void draw_vertex_kernel(DrawArgs a) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    int oid, v0, nv, f0, nf;
    draw_obj_range(a, b, oid, v0, nv, f0, nf);
    if (i >= DRAW_HAND_VERTS + nv) {                             // rows past this sample's vertices: zero, so the whole record plane is defined
        if (i < a.VP) { DrawRec z = {}; a.rec[(size_t)b * a.VP + i] = z; }
        return;
    }
    float P[3], n[3] = {0.f, 0.f, 0.f}, base[3];
    if (i < DRAW_HAND_VERTS) {
        const float* hv = a.hand_verts + (size_t)b * DRAW_HAND_VERTS * 3;
        P[0] = hv[i * 3]; P[1] = hv[i * 3 + 1]; P[2] = hv[i * 3 + 2];
        int j0 = a.adj_off[i], j1 = a.adj_off[i + 1];
        if (j0 < 0) j0 = 0;
        if (j1 > a.nadj) j1 = a.nadj;
        for (int j = j0; j < j1; ++j) {                           // gather: the faces around this vertex, in ascending face order
            const int f = a.adj_face[j];
            if (f < 0 || f >= a.nhf) continue;
            const int i0 = a.hand_faces[f * 3], i1 = a.hand_faces[f * 3 + 1], i2 = a.hand_faces[f * 3 + 2];
            if ((unsigned)i0 >= DRAW_HAND_VERTS || (unsigned)i1 >= DRAW_HAND_VERTS || (unsigned)i2 >= DRAW_HAND_VERTS) continue;
            draw_cross_acc(hv + i0 * 3, hv + i1 * 3, hv + i2 * 3, n);
        }
        base[0] = 102.0f / 255.0f; base[1] = 209.0f / 255.0f; base[2] = 243.0f / 255.0f;
    } else {
        const int ov = i - DRAW_HAND_VERTS;
        draw_obj_point(a, b, oid, v0, ov, P);
        if (oid == DRAW_OBJ_BOX) {
            const float* c = a.corners + (size_t)b * 24;
#pragma unroll
            for (int f = 0; f < 12; ++f) {
                const int i0 = c_box_faces[f][0], i1 = c_box_faces[f][1], i2 = c_box_faces[f][2];
                if (i0 == ov || i1 == ov || i2 == ov) draw_cross_acc(c + i0 * 3, c + i1 * 3, c + i2 * 3, n);
            }
        } else {
            const float* m = a.obj_normals + (size_t)(v0 + ov) * 3;
            const float* R = a.obj_rot + (size_t)b * 9;
            n[0] = (R[0] * m[0] + R[1] * m[1]) + R[2] * m[2];
            n[1] = (R[3] * m[0] + R[4] * m[1]) + R[5] * m[2];
            n[2] = (R[6] * m[0] + R[7] * m[1]) + R[8] * m[2];
        }
        base[0] = 255.0f / 255.0f; base[1] = 163.0f / 255.0f; base[2] = 172.0f / 255.0f;
    }
    const float nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    const float ninv = nn > 0.f ? 1.0f / sqrtf(nn) : 0.f;
    float shade[2] = {0.f, 0.f};                                 // the two white lights | the 0.7 light
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const float d[3] = {a.light[l][0] - P[0], a.light[l][1] - P[1], a.light[l][2] - P[2]};
        const float dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        const float dot = ((n[0] * d[0] + n[1] * d[1]) + n[2] * d[2]) * ninv / sqrtf(dd);
        if (dot > 0.f) shade[l == 2] += dot;
    }
    const float s = shade[0] + 0.7f * shade[1];
    DrawRec r;
    r.r = fminf(base[0] * s, 1.0f); r.g = fminf(base[1] * s, 1.0f); r.b = fminf(base[2] * s, 1.0f);
    const float* K = a.cam_intr + (size_t)b * 9;
    bool ok0 = draw_project(K[0], K[4], K[2], K[5], P[0], P[1], P[2], r.sx0, r.sy0, r.zq0);
    r.zv0 = P[2];
    const DrawView& V = a.view;
    const float q[3] = {P[0] - a.cam[b].pos[0], P[1] - a.cam[b].pos[1], P[2] - a.cam[b].pos[2]};
    const float xv = (V.r[0] * q[0] + V.r[1] * q[1]) + V.r[2] * q[2];
    const float yv = (V.d[0] * q[0] + V.d[1] * q[1]) + V.d[2] * q[2];
    const float zv = (V.f[0] * q[0] + V.f[1] * q[1]) + V.f[2] * q[2];
    bool ok1 = draw_project(V.focal, V.focal, 0.5f * (float)a.W, 0.5f * (float)a.H, xv, yv, zv, r.sx1, r.sy1, r.zq1);
    r.zv1 = zv;
    r.flags = (ok0 ? 1u : 0u) | (ok1 ? 2u : 0u);
    a.rec[(size_t)b * a.VP + i] = r;
}

// ------------------------------------------------------------------ kernel 3: raster (one thread per face and view)
struct DrawTri { int32_t x[3], y[3]; uint32_t z[3]; int vi[3]; };

// vertex records of face gid (hand faces first, then the object's) in view `view`, oriented to positive area; false: dropped
__device__ __forceinline__ bool draw_setup(const DrawArgs& a, int b, int view, int gid, int oid, int nv, int f0, int nf, DrawTri& t) {
    if (gid < a.nhf) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t.vi[k] = a.hand_faces[gid * 3 + k];
            if ((unsigned)t.vi[k] >= DRAW_HAND_VERTS) return false;
        }
    } else {
        const int f = gid - a.nhf;
        if (f >= nf) return false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int v = oid == DRAW_OBJ_BOX ? (int)c_box_faces[f][k] : a.obj_faces[(size_t)(f0 + f) * 3 + k];
            if ((unsigned)v >= (unsigned)nv) return false;
            t.vi[k] = DRAW_HAND_VERTS + v;
        }
    }
    const DrawRec* rec = a.rec + (size_t)b * a.VP;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const DrawRec& r = rec[t.vi[k]];
        if (!((r.flags >> view) & 1u)) return false;
        t.x[k] = view ? r.sx1 : r.sx0; t.y[k] = view ? r.sy1 : r.sy0; t.z[k] = view ? r.zq1 : r.zq0;
    }
    const int64_t area = (int64_t)(t.x[1] - t.x[0]) * (t.y[2] - t.y[0]) - (int64_t)(t.y[1] - t.y[0]) * (t.x[2] - t.x[0]);
    if (area == 0 || area >= DRAW_AREA_LIMIT || -area >= DRAW_AREA_LIMIT) return false;
    if (area < 0) {
        int32_t s = t.x[1]; t.x[1] = t.x[2]; t.x[2] = s;
        s = t.y[1]; t.y[1] = t.y[2]; t.y[2] = s;
        const uint32_t z = t.z[1]; t.z[1] = t.z[2]; t.z[2] = z;
        const int v = t.vi[1]; t.vi[1] = t.vi[2]; t.vi[2] = v;
    }
    return true;
}

__global__ __launch_bounds__(256) void draw_raster_kernel(DrawArgs a) {
    const int b = blockIdx.z, view = blockIdx.y, gid = blockIdx.x * 256 + threadIdx.x;
    if (view == 0 && gid >= a.nhf) return;                      // the overlay shows the hand alone
    int oid, v0, nv, f0, nf;
    draw_obj_range(a, b, oid, v0, nv, f0, nf);
    if (gid >= a.nhf + nf) return;
    DrawTri t;
    if (!draw_setup(a, b, view, gid, oid, nv, f0, nf, t)) return;
    const int32_t minx = min(t.x[0], min(t.x[1], t.x[2])), maxx = max(t.x[0], max(t.x[1], t.x[2]));
    const int32_t miny = min(t.y[0], min(t.y[1], t.y[2])), maxy = max(t.y[0], max(t.y[1], t.y[2]));
    const int x0 = max(0, (minx - 128 + 255) >> 8), x1 = min(a.W - 1, (maxx - 128) >> 8);
    const int y0 = max(0, (miny - 128 + 255) >> 8), y1 = min(a.H - 1, (maxy - 128) >> 8);
    if (x0 > x1 || y0 > y1) return;
    // the edge functions are affine in the pixel index: one 64-bit add per edge per pixel; the shared-edge rule is a bias of 1 on the
    // non-inclusive edges.  The doubled area is their sum.
    const int32_t ex[3] = {t.x[2] - t.x[1], t.x[0] - t.x[2], t.x[1] - t.x[0]};
    const int32_t ey[3] = {t.y[2] - t.y[1], t.y[0] - t.y[2], t.y[1] - t.y[0]};
    const int32_t axv[3] = {t.x[1], t.x[2], t.x[0]}, ayv[3] = {t.y[1], t.y[2], t.y[0]};
    const int32_t px0 = x0 * 256 + 128, py0 = y0 * 256 + 128;
    int64_t wrow[3], sx[3], sy[3], bias[3], sum = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        wrow[k] = (int64_t)ex[k] * (py0 - ayv[k]) - (int64_t)ey[k] * (px0 - axv[k]);
        sx[k] = -(int64_t)ey[k] * 256; sy[k] = (int64_t)ex[k] * 256;
        sum += wrow[k];
        bias[k] = ((ey[k] > 0) || (ey[k] == 0 && ex[k] < 0)) ? 0 : 1;
    }
    const double inv = 1.0 / (double)sum;
    unsigned long long* kb = a.keys + ((size_t)b * 2 + view) * a.W * a.H;
    for (int y = y0; y <= y1; ++y) {
        int64_t w0 = wrow[0], w1 = wrow[1], w2 = wrow[2];
        for (int x = x0; x <= x1; ++x) {
            if (((w0 - bias[0]) | (w1 - bias[1]) | (w2 - bias[2])) >= 0) {
                const int64_t num = w0 * (int64_t)t.z[0] + w1 * (int64_t)t.z[1] + w2 * (int64_t)t.z[2];
                int64_t q = (int64_t)((double)num * inv);        // exact floor(num / sum): double estimate (error < 1) + fix-up
                const int64_t r = num - q * sum;
                if (r < 0) --q; else if (r >= sum) ++q;
                atomicMin(&kb[(size_t)y * a.W + x], ((unsigned long long)q << 32) | (uint32_t)gid);
            }
            w0 += sx[0]; w1 += sx[1]; w2 += sx[2];
        }
        wrow[0] += sy[0]; wrow[1] += sy[1]; wrow[2] += sy[2];
    }
}

// ------------------------------------------------------------------ kernel 4: resolve
__device__ __forceinline__ uint8_t draw_q8(float c) {
    float q = floorf(255.0f * c + 0.5f);
    q = fminf(fmaxf(q, 0.f), 255.f);
    return (uint8_t)q;
}

__global__ __launch_bounds__(256) void draw_resolve_kernel(DrawArgs a) {
    const int b = blockIdx.z, view = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.W * a.H) return;
    const int x = i % a.W, y = i / a.W;
    const unsigned long long key = a.keys[((size_t)b * 2 + view) * a.W * a.H + i];
    uint8_t o[3];
    if (key == ~0ull) {
        if (view == 0) {
            // the frame: image + 0.5 (the batch's float CHW tensor), quantised as every drawing of this build does
            const float* im = a.image + (size_t)b * 3 * a.W * a.H;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = draw_q8(im[(size_t)c * a.W * a.H + i] + 0.5f);
        } else o[0] = o[1] = o[2] = 255;
    } else {
        int oid, v0, nv, f0, nf;
        draw_obj_range(a, b, oid, v0, nv, f0, nf);
        DrawTri t;
        o[0] = o[1] = o[2] = 0;
        if (draw_setup(a, b, view, (int)(uint32_t)key, oid, nv, f0, nf, t)) {
            const int32_t px = x * 256 + 128, py = y * 256 + 128;
            const int64_t w0 = (int64_t)(t.x[2] - t.x[1]) * (py - t.y[1]) - (int64_t)(t.y[2] - t.y[1]) * (px - t.x[1]);
            const int64_t w1 = (int64_t)(t.x[0] - t.x[2]) * (py - t.y[2]) - (int64_t)(t.y[0] - t.y[2]) * (px - t.x[2]);
            const int64_t w2 = (int64_t)(t.x[1] - t.x[0]) * (py - t.y[0]) - (int64_t)(t.y[1] - t.y[0]) * (px - t.x[0]);
            const float ws = (float)(w0 + w1 + w2);
            const float l0 = (float)w0 / ws, l1 = (float)w1 / ws, l2 = (float)w2 / ws;
            const DrawRec* rec = a.rec + (size_t)b * a.VP;
            const DrawRec &r0 = rec[t.vi[0]], &r1 = rec[t.vi[1]], &r2 = rec[t.vi[2]];
            const float i0 = 1.0f / (view ? r0.zv1 : r0.zv0), i1 = 1.0f / (view ? r1.zv1 : r1.zv0), i2 = 1.0f / (view ? r2.zv1 : r2.zv0);
            const float d = (l0 * i0 + l1 * i1) + l2 * i2;
            const float m0 = (l0 * i0) / d, m1 = (l1 * i1) / d, m2 = (l2 * i2) / d;
            o[0] = draw_q8((m0 * r0.r + m1 * r1.r) + m2 * r2.r);
            o[1] = draw_q8((m0 * r0.g + m1 * r1.g) + m2 * r2.g);
            o[2] = draw_q8((m0 * r0.b + m1 * r1.b) + m2 * r2.b);
        }
    }
    uint8_t* p = a.out + (((size_t)b * a.H + y) * 4 * a.W + (size_t)(1 + view) * a.W + x) * 3;
    p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
}

__global__ void draw_fill_keys_kernel(unsigned long long* __restrict__ k, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) k[i] = ~0ull;
}

// ------------------------------------------------------------------ host entry points
static inline long draw_al(long x) { return (x + 255) / 256 * 256; }
static inline long draw_rec_bytes(int B, int max_obj_verts) {
    return draw_al((long)B * (DRAW_HAND_VERTS + (max_obj_verts < 8 ? 8 : max_obj_verts)) * (long)sizeof(DrawRec));
}

extern "C" long ab_draw_workspace_bytes(int B, int W, int H, int max_obj_verts) {
    if (B <= 0 || W <= 0 || H <= 0 || max_obj_verts < 0) return 0;
    return draw_rec_bytes(B, max_obj_verts) + draw_al((long)B * (long)sizeof(DrawCam)) + draw_al((long)B * 2 * W * H * 8);
}
extern "C" long ab_draw_workspace_keys_offset(int B, int max_obj_verts) {
    if (B <= 0 || max_obj_verts < 0) return 0;
    return draw_rec_bytes(B, max_obj_verts) + draw_al((long)B * (long)sizeof(DrawCam));
}

extern "C" int ab_draw_meshes(const float* hand_verts, const int32_t* hand_faces, int nhf, const int32_t* adj_off, const int32_t* adj_face,
                              int nadj, const float* obj_verts, const float* obj_normals, const int32_t* obj_faces,
                              const int32_t* obj_vert_off, const int32_t* obj_face_off, int n_obj, int nov, int nof, int max_obj_verts,
                              int max_obj_faces, const int32_t* obj_id, const float* obj_rot, const float* obj_tsl, const float* corners,
                              const float* cam_intr, const float* image, int B, int W, int H, uint8_t* out, void* workspace, void* stream) {
    if (!hand_verts || !hand_faces || !adj_off || !adj_face || !cam_intr || !image || !out || !workspace) return AB_EINVAL;
    if (B <= 0 || W <= 0 || H <= 0 || W > 4096 || H > 4096 || nhf <= 0 || nadj < 0 || n_obj < 0 || nov < 0 || nof < 0 || max_obj_verts < 0 ||
        max_obj_faces < 0)
        return AB_ESHAPE;
    if (n_obj > 0 && (!obj_verts || !obj_normals || !obj_faces || !obj_vert_off || !obj_face_off || !obj_id || !obj_rot || !obj_tsl)) return AB_EINVAL;
    if (max_obj_verts < 8) max_obj_verts = 8;
    if (max_obj_faces < 12) max_obj_faces = 12;
    DrawArgs a;
    a.hand_verts = hand_verts; a.hand_faces = hand_faces; a.nhf = nhf; a.adj_off = adj_off; a.adj_face = adj_face; a.nadj = nadj;
    a.obj_verts = obj_verts; a.obj_normals = obj_normals; a.obj_faces = obj_faces; a.obj_vert_off = obj_vert_off; a.obj_face_off = obj_face_off;
    a.n_obj = n_obj; a.nov = nov; a.nof = nof; a.max_obj_verts = max_obj_verts;
    a.obj_id = obj_id; a.obj_rot = obj_rot; a.obj_tsl = obj_tsl; a.corners = corners; a.cam_intr = cam_intr; a.image = image;
    a.B = B; a.W = W; a.H = H; a.VP = DRAW_HAND_VERTS + max_obj_verts;
    char* ws = (char*)workspace;
    a.rec = (DrawRec*)ws;
    a.cam = (DrawCam*)(ws + draw_rec_bytes(B, max_obj_verts));
    a.keys = (unsigned long long*)(ws + ab_draw_workspace_keys_offset(B, max_obj_verts));
    a.out = out;
    // orbit camera and lights, formed in double and rounded once
    const double deg = 3.14159265358979323846 / 180.0, az = -50.0 * deg, el = 50.0 * deg, dist = 0.6;
    const double u[3] = {sin(el) * cos(az), sin(el) * sin(az), cos(el)};
    const double f[3] = {-u[0], -u[1], -u[2]};
    double r[3] = {f[1] * 1.0 - f[2] * 0.0, f[2] * 0.0 - f[0] * 1.0, 0.0};       // f x (0, 0, 1)
    const double rl = sqrt(r[0] * r[0] + r[1] * r[1]);
    r[0] /= rl; r[1] /= rl;
    const double d[3] = {f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]};
    for (int k = 0; k < 3; ++k) { a.view.r[k] = (float)r[k]; a.view.d[k] = (float)d[k]; a.view.f[k] = (float)f[k]; a.view.off[k] = (float)(dist * u[k]); }
    a.view.focal = (float)(0.5 * H / tan(15.0 * deg));
    const double lp[3][3] = {{-200, -100, -100}, {800, 10, 300}, {-500, 500, 1000}}, ry = 120.0 * deg;
    for (int l = 0; l < 3; ++l) {                                               // row vector times R_y(120 degrees)
        a.light[l][0] = (float)(lp[l][0] * cos(ry) - lp[l][2] * sin(ry));
        a.light[l][1] = (float)lp[l][1];
        a.light[l][2] = (float)(lp[l][0] * sin(ry) + lp[l][2] * cos(ry));
    }
    hipStream_t st = as_stream(stream);
    const long nkeys = (long)B * 2 * W * H;
    draw_fill_keys_kernel<<<(unsigned)((nkeys + 255) / 256), 256, 0, st>>>(a.keys, nkeys);
    draw_bbox_kernel<<<B, 256, 0, st>>>(a);
    draw_vertex_kernel<<<dim3((unsigned)((a.VP + 255) / 256), B), 256, 0, st>>>(a);
    draw_raster_kernel<<<dim3((unsigned)((nhf + max_obj_faces + 255) / 256), 2, B), 256, 0, st>>>(a);
    draw_resolve_kernel<<<dim3((unsigned)((W * H + 255) / 256), 2, B), 256, 0, st>>>(a);
    AB_LAUNCH_CHECK();
    return 0;
}
