// Hand-object interaction measures of the evaluator on the device, eager only:
//   ab_interaction   per sample: the hand vertices against the posed object mesh (signed distance, generalised winding number, maximum
//                    and mean penetration depth, smallest distance, contact) and the intersection volume of the two meshes on a lattice.
//
// Definitions (the header, metrics.interaction_values_torch and the tests use the same ones).  A mesh is vertices and triangles (a, b, c);
// for a query q, with A = a - q, B = b - q, C = c - q:
//   solid angle      num = A . (B x C),  den = |A||B||C| + (A.B)|C| + (B.C)|A| + (C.A)|B|,  Omega = 2 atan2(num, den), 0 when both are 0
//   winding number   w(q) = sum_f Omega_f / (4 pi);  q is INSIDE when o w(q) > 0.5, o = +-1 the sign of the mesh's signed volume, computed
//                    by the host per mesh in float64 (nothing here assumes a sign; the meshes need not be watertight)
//   distance         d(q) = min_f |q - cp_f(q)|, cp_f the closest point of triangle f by the region form (vertex a, b, edge ab, vertex c,
//                    edge ac, edge bc, interior, the first that applies), every division guarded: a zero denominator gives parameter 0.
//                    cp - q = A + v (b - a) + w (c - a) is a sum of differences; squared lengths are compared, one square root per query.
// The object of sample b is R_b can + t_b.  Winding number and distance are invariant under rigid maps, so a query is taken into the
// object's canonical frame once, q' = R_b^T (q - t_b), and the canonical triangles are scanned straight from the packed table: no posed
// face list is written, coordinates stay within the object's extent, and samples that hold the same object read the same table lines.
//
// Launches.  (1) AB_IA_VERTS, one workgroup of 256 threads per (sample, chunk of 256 hand vertices): the object's triangles go through LDS
// in SoA tiles of 512 (nine coordinate arrays, one wave-uniform ds_read_b128 per array serves four triangles for 64 queries; a tile's tail
// repeats one vertex three times: solid angle 0, distance that of a point of the mesh); per lane one running minimum and one compensated
// running sum of half-angles atan2(num, den), added in face order; a chunk leaves n_inside, the sum and maximum of the inside depths and
// the smallest distance in the workspace (wave butterflies, the four waves in turn).  (2) AB_IA_VOLUME, one workgroup per sample: the boxes
// of the hand vertices and of the posed object vertices, their intersection, the lattice index ranges and n_lattice (or the capped mark).
// (3) AB_IA_VOLUME, a FIXED grid of ceil(max_voxels / 256) chunks per sample; a workgroup past n_lattice or of a capped sample leaves at
// once, so the host reads nothing back between the launches.  A lattice point p = h (i + 1/2, j + 1/2, k + 1/2) of the camera frame is
// tested against the object (canonical frame) and, when any point of the chunk is inside it, against the hand mesh (camera frame); the
// count of points inside both does not depend on that shortcut.  (4) one thread per sample adds its chunks in turn and writes the row.
// No atomics of any kind; two calls give the same bits, and a sample's row, counts, sdf and wind do not depend on the batch around it.
// Like the three mesh entry points before it this one is never captured in a hipGraph (DESIGN.md sections 19, 23, 24).
// The triangle primitive (ia_tri, ia_scan, the object row and the canonical frame) is csrc/ia_tile.h, shared with csrc/contact_loss.hip.
#include "ia_tile.h"

#define IA_PART 4              // words per (sample, vertex chunk): n_inside (int32) | sum of inside depths | largest inside depth | smallest distance
#define IA_HEAD 8              // int32 words per sample: first lattice index [3] | lattice points per axis [3] | n_lattice | capped

// ---- launch 1: the hand vertices against the object ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IA_THREADS) void interaction_verts_kernel(const float* __restrict__ hand_verts, int Nh, const float* __restrict__ obj_verts,
                                                                        const int32_t* __restrict__ obj_faces, const int32_t* __restrict__ vert_off,
                                                                        const int32_t* __restrict__ face_off, const float* __restrict__ obj_orient,
                                                                        int n_obj, const int64_t* __restrict__ obj_row, const float* __restrict__ rot,
                                                                        const float* __restrict__ tsl, float* __restrict__ sdf, float* __restrict__ wind,
                                                                        float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float ts[9 * IA_TILE];
    __shared__ float s_part[4][IA_PART];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * IA_THREADS + (int)threadIdx.x;
    const bool live = q < Nh;
    const int qc = live ? q : Nh - 1;                                            // lanes past the end recompute the last vertex (masked below)
    const ia_object o = ia_load_object(obj_verts, obj_faces, vert_off, face_off, obj_orient, n_obj, obj_row, rot, tsl, b);
    const float* hv = hand_verts + ((size_t)b * Nh + qc) * 3;
    float qx, qy, qz;
    ia_to_canonical(o, hv[0], hv[1], hv[2], qx, qy, qz);
    float sum = 0.f, comp = 0.f, best = __builtin_inff();
    ia_scan<true>(o.verts, o.nv, o.faces, o.nf, ts, qx, qy, qz, sum, comp, best);
    const float w = o.orient * (sum / IA_TWO_PI);                                // sum of half-angles / (2 pi) = sum of Omega / (4 pi)
    const float d = sqrtf(best);
    const bool in = live && w > 0.5f;
    if (live && sdf) sdf[(size_t)b * Nh + q] = in ? -d : d;
    if (live && wind) wind[(size_t)b * Nh + q] = w;
    const int cnt = (int)__popcll(__ballot(in));
    const float ps = wave_sum(in ? d : 0.f), pm = wave_max(in ? d : 0.f), mn = -wave_max(live ? -d : -__builtin_inff());
    if (lane == 0) { s_part[wave][0] = __int_as_float(cnt); s_part[wave][1] = ps; s_part[wave][2] = pm; s_part[wave][3] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* p = part + ((size_t)b * gridDim.x + blockIdx.x) * IA_PART;
        p[0] = __int_as_float(((__float_as_int(s_part[0][0]) + __float_as_int(s_part[1][0])) + __float_as_int(s_part[2][0])) + __float_as_int(s_part[3][0]));
        p[1] = ((s_part[0][1] + s_part[1][1]) + s_part[2][1]) + s_part[3][1];
        p[2] = fmaxf(fmaxf(s_part[0][2], s_part[1][2]), fmaxf(s_part[2][2], s_part[3][2]));
        p[3] = fminf(fminf(s_part[0][3], s_part[1][3]), fminf(s_part[2][3], s_part[3][3]));
    }
}

// ---- launch 2: the two boxes, the lattice index ranges and n_lattice, one workgroup per sample ----------------------------------------------------
__global__ __launch_bounds__(IA_THREADS) void interaction_boxes_kernel(const float* __restrict__ hand_verts, int Nh, const float* __restrict__ obj_verts,
                                                                        const int32_t* __restrict__ obj_faces, const int32_t* __restrict__ vert_off,
                                                                        const int32_t* __restrict__ face_off, const float* __restrict__ obj_orient,
                                                                        int n_obj, const int64_t* __restrict__ obj_row, const float* __restrict__ rot,
                                                                        const float* __restrict__ tsl, float voxel, int max_voxels, int32_t* __restrict__ head) {
    __shared__ float s_box[4][12];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ia_object o = ia_load_object(obj_verts, obj_faces, vert_off, face_off, obj_orient, n_obj, obj_row, rot, tsl, b);
    const float inf = __builtin_inff();
    float box[12] = {inf, inf, inf, -inf, -inf, -inf, inf, inf, inf, -inf, -inf, -inf};      // hand lo | hand hi | object lo | object hi
    for (int i = threadIdx.x; i < Nh; i += IA_THREADS)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = hand_verts[((size_t)b * Nh + i) * 3 + k];
            box[k] = fminf(box[k], x); box[3 + k] = fmaxf(box[3 + k], x);
        }
    for (int i = threadIdx.x; i < o.nv; i += IA_THREADS) {
        const float* v = o.verts + (size_t)i * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = ia_dot(o.R[k * 3], o.R[k * 3 + 1], o.R[k * 3 + 2], v[0], v[1], v[2]) + o.t[k];     // R can + t
            box[6 + k] = fminf(box[6 + k], x); box[9 + k] = fmaxf(box[9 + k], x);
        }
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const bool lo = (k / 3) % 2 == 0;
        const float v = lo ? -wave_max(-box[k]) : wave_max(box[k]);
        if (lane == 0) s_box[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int first[3], cnt[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float hl = inf, hh = -inf, ol = inf, oh = -inf;
            for (int w = 0; w < 4; ++w) { hl = fminf(hl, s_box[w][k]); hh = fmaxf(hh, s_box[w][3 + k]); ol = fminf(ol, s_box[w][6 + k]); oh = fmaxf(oh, s_box[w][9 + k]); }
            const float lo = fmaxf(hl, ol), hi = fminf(hh, oh);
            // h (i + 1/2) in [lo, hi]  <=>  i in [lo / h - 1/2, hi / h - 1/2]
            const float fl = fminf(fmaxf(ceilf(lo / voxel - 0.5f), -1.0e9f), 1.0e9f), fh = fminf(fmaxf(floorf(hi / voxel - 0.5f), -1.0e9f), 1.0e9f);
            first[k] = (int)fl;
            cnt[k] = fh >= fl ? (int)fh - (int)fl + 1 : 0;
        }
        const long long nxy = (long long)cnt[0] * cnt[1];
        const bool capped = nxy > max_voxels || nxy * cnt[2] > max_voxels;
        const long long nl = capped ? (nxy > 0x7fffffffLL / max(cnt[2], 1) ? 0x7fffffffLL : nxy * cnt[2]) : nxy * cnt[2];
        int32_t* h = head + (size_t)b * IA_HEAD;
        h[0] = first[0]; h[1] = first[1]; h[2] = first[2]; h[3] = cnt[0]; h[4] = cnt[1]; h[5] = cnt[2]; h[6] = (int)nl; h[7] = capped ? 1 : 0;
    }
}

// ---- launch 3: the lattice points against both meshes, a fixed grid ------------------------------------------------------------------------------
__global__ __launch_bounds__(IA_THREADS) void interaction_volume_kernel(const float* __restrict__ hand_verts, const int32_t* __restrict__ hand_faces, int Nh,
                                                                         int Fh, float hand_orient, const float* __restrict__ obj_verts,
                                                                         const int32_t* __restrict__ obj_faces, const int32_t* __restrict__ vert_off,
                                                                         const int32_t* __restrict__ face_off, const float* __restrict__ obj_orient,
                                                                         int n_obj, const int64_t* __restrict__ obj_row, const float* __restrict__ rot,
                                                                         const float* __restrict__ tsl, float voxel, const int32_t* __restrict__ head,
                                                                         int32_t* __restrict__ vpart) {
    __shared__ __attribute__((aligned(16))) float ts[9 * IA_TILE];
    __shared__ int s_cnt[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* h = head + (size_t)b * IA_HEAD;
    const int nl = h[6];
    if (h[7] || (long long)blockIdx.x * IA_THREADS >= nl) return;                // block-uniform: capped, or past the lattice
    const int idx = blockIdx.x * IA_THREADS + (int)threadIdx.x;
    const bool live = idx < nl;
    const int ic = live ? idx : nl - 1;
    const int nx = h[3], ny = h[4];
    const int i = ic % nx, j = (ic / nx) % ny, k = ic / (nx * ny);
    const float px = voxel * ((float)(h[0] + i) + 0.5f), py = voxel * ((float)(h[1] + j) + 0.5f), pz = voxel * ((float)(h[2] + k) + 0.5f);
    const ia_object o = ia_load_object(obj_verts, obj_faces, vert_off, face_off, obj_orient, n_obj, obj_row, rot, tsl, b);
    float qx, qy, qz;
    ia_to_canonical(o, px, py, pz, qx, qy, qz);
    float sum = 0.f, comp = 0.f, best = 0.f;
    ia_scan<false>(o.verts, o.nv, o.faces, o.nf, ts, qx, qy, qz, sum, comp, best);
    const bool in_obj = live && o.orient * (sum / IA_TWO_PI) > 0.5f;
    const int wave_any = __ballot(in_obj) != 0ull;                               // every lane votes: not under the lane-0 branch
    if (lane == 0) s_cnt[wave] = wave_any;
    __syncthreads();
    const bool any = (s_cnt[0] | s_cnt[1] | s_cnt[2] | s_cnt[3]) != 0;           // block-uniform
    __syncthreads();
    bool both = false;
    if (any) {                                                                   // a chunk with no point inside the object holds no point inside both
        sum = 0.f; comp = 0.f;
        ia_scan<false>(hand_verts + (size_t)b * Nh * 3, Nh, hand_faces, Fh, ts, px, py, pz, sum, comp, best);
        both = in_obj && hand_orient * (sum / IA_TWO_PI) > 0.5f;
    }
    const int cnt = (int)__popcll(__ballot(both));
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) vpart[(size_t)b * gridDim.x + blockIdx.x] = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
}

// ---- launch 4: one thread per sample adds its chunks in turn ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void interaction_finalize_kernel(const float* __restrict__ part, const int32_t* __restrict__ head,
                                                                   const int32_t* __restrict__ vpart, int B, int Nh, int cv, int cl, float contact_thr,
                                                                   float voxel, int flags, float* __restrict__ rows, int32_t* __restrict__ counts) {
    const int b = blockIdx.x * 256 + (int)threadIdx.x;
    if (b >= B) return;
    float* row = rows + (size_t)b * AB_IA_ROW;
    int32_t* cn = counts + (size_t)b * 4;
#pragma unroll
    for (int k = 0; k < AB_IA_ROW; ++k) row[k] = ab_nan();
    cn[0] = cn[1] = cn[2] = cn[3] = 0;
    if (flags & AB_IA_VERTS) {
        int n_in = 0;
        float ps = 0.f, pm = 0.f, mn = __builtin_inff();
        for (int c = 0; c < cv; ++c) {
            const float* p = part + ((size_t)b * cv + c) * IA_PART;
            n_in += __float_as_int(p[0]); ps += p[1]; pm = fmaxf(pm, p[2]); mn = fminf(mn, p[3]);
        }
        row[AB_IA_PEN_MAX] = pm;
        row[AB_IA_PEN_MEAN] = n_in > 0 ? ps / (float)n_in : 0.f;
        row[AB_IA_MIN_DIST] = mn;
        row[AB_IA_INSIDE_FRAC] = (float)n_in / (float)Nh;
        row[AB_IA_CONTACT] = (n_in > 0 || mn <= contact_thr) ? 1.f : 0.f;
        cn[0] = n_in;
    }
    if (flags & AB_IA_VOLUME) {
        const int32_t* h = head + (size_t)b * IA_HEAD;
        cn[1] = h[6]; cn[3] = h[7];
        if (!h[7]) {
            const int nc = (int)(((long long)h[6] + IA_THREADS - 1) / IA_THREADS);       // <= cl: n_lattice <= max_voxels
            int n_both = 0;
            for (int c = 0; c < nc; ++c) n_both += vpart[(size_t)b * cl + c];
            cn[2] = n_both;
            row[AB_IA_VOL] = (float)n_both * (voxel * voxel * voxel);
        }
    }
}

static inline long ia_vchunks(int Nh) { return ((long)Nh + IA_THREADS - 1) / IA_THREADS; }
static inline long ia_lchunks(int max_voxels) { return ((long)max_voxels + IA_THREADS - 1) / IA_THREADS; }

extern "C" long ab_interaction_workspace(int B, int Nh, int max_voxels) {
    if (B < 1 || Nh < 1 || max_voxels < 1) return 0;
    return (long)B * (IA_HEAD + ia_vchunks(Nh) * IA_PART + ia_lchunks(max_voxels)) * (long)sizeof(float);
}

extern "C" int ab_interaction(const float* hand_verts, const int32_t* hand_faces, int Nh, int Fh, float hand_orient, const float* obj_verts,
                              const int32_t* obj_faces, const int32_t* vert_off, const int32_t* face_off, const float* obj_orient, int n_obj,
                              const int64_t* obj_row, const float* rot, const float* tsl, int B, float contact_thr, float voxel, int max_voxels,
                              int flags, float* rows, int32_t* counts, float* sdf, float* wind, void* workspace, void* stream) {
    if (!hand_verts || !obj_verts || !obj_faces || !vert_off || !face_off || !obj_orient || !obj_row || !rot || !tsl) return AB_EINVAL;
    if (!rows || !counts || !workspace) return AB_EINVAL;
    if (B < 1 || B > 65535 || Nh < 1 || Nh > (1 << 24) || Fh < 1 || Fh > (1 << 24) || n_obj < 1) return AB_EINVAL;
    if (!(flags & (AB_IA_VERTS | AB_IA_VOLUME)) || (flags & ~(AB_IA_VERTS | AB_IA_VOLUME))) return AB_EINVAL;
    if ((flags & AB_IA_VOLUME) && (!hand_faces || !(hand_orient == 1.f || hand_orient == -1.f))) return AB_EINVAL;
    if (!(contact_thr >= 0.f) || !(voxel > 0.f) || !(voxel < __builtin_inff()) || max_voxels < 1 || max_voxels > (1 << 24)) return AB_EINVAL;
    const int cv = (int)ia_vchunks(Nh), cl = (int)ia_lchunks(max_voxels);
    int32_t* head = (int32_t*)workspace;
    float* part = (float*)workspace + (size_t)B * IA_HEAD;
    int32_t* vpart = (int32_t*)(part + (size_t)B * cv * IA_PART);
    if (flags & AB_IA_VERTS) {
        interaction_verts_kernel<<<dim3(cv, B), IA_THREADS, 0, as_stream(stream)>>>(hand_verts, Nh, obj_verts, obj_faces, vert_off, face_off, obj_orient,
                                                                                    n_obj, obj_row, rot, tsl, sdf, wind, part);
        AB_LAUNCH_CHECK();
    }
    if (flags & AB_IA_VOLUME) {
        interaction_boxes_kernel<<<B, IA_THREADS, 0, as_stream(stream)>>>(hand_verts, Nh, obj_verts, obj_faces, vert_off, face_off, obj_orient, n_obj,
                                                                          obj_row, rot, tsl, voxel, max_voxels, head);
        AB_LAUNCH_CHECK();
        interaction_volume_kernel<<<dim3(cl, B), IA_THREADS, 0, as_stream(stream)>>>(hand_verts, hand_faces, Nh, Fh, hand_orient, obj_verts, obj_faces,
                                                                                     vert_off, face_off, obj_orient, n_obj, obj_row, rot, tsl, voxel,
                                                                                     head, vpart);
        AB_LAUNCH_CHECK();
    }
    interaction_finalize_kernel<<<(B + 255) / 256, 256, 0, as_stream(stream)>>>(part, head, vpart, B, Nh, cv, cl, contact_thr, voxel, flags, rows, counts);
    AB_LAUNCH_CHECK();
    return 0;
}
