// The reverse direction of ab_interaction, eager only:
//   ab_interaction_sym   per sample: the vertices of the object against the posed hand mesh (signed distance, generalised winding number,
//                        maximum and mean penetration depth, smallest distance, contact).
//
// Definitions: solid angle, winding number, orientation, "inside <=> o w > 0.5", the closest point by the region form and the first
// minimum in face order are those of the header of interact.hip, computed by the same functions (csrc/ia_tile.h), so a distance has the
// same bits here as there.  Here the TRIANGLES are posed per sample (the hand) and the QUERIES come from the packed table (the object):
// each hand vertex is taken into the object's canonical frame once, v' = R_b^T (v - t_b), with the arithmetic of ia_to_canonical, and the
// canonical object vertices are the queries as they stand in the table.  No posed object vertex is formed; coordinates stay within the
// object's extent.  No query is culled by the hand's box: on a mesh that is not watertight a point outside the box can still have
// o w > 0.5, and the definition does not depend on a shortcut.
//
// Launches.  (1) one thread per (sample, hand vertex) writes hand_can [B,Nh,3] into the workspace.  (2) a FIXED grid of
// ceil(No_max / 256) chunks x B samples, 256 threads, one object vertex per thread: a workgroup whose chunk starts at or past No_r fills
// its slots of sdf_obj / wind_obj with NaN and leaves, block-uniformly and before any barrier (the host reads nothing back); lanes past
// No_r of the last live chunk recompute the last vertex and are masked out of every reduction; the hand's triangles go through LDS in SoA
// tiles of 512 (ia_scan, unchanged); a chunk leaves n_inside, the sum and maximum of the inside depths and the smallest distance in the
// workspace (ballot + popcount, wave butterflies, the four waves in turn).  (3) one thread per sample adds its live chunks in turn and
// writes the row and the counts.  Every output word has one writer and every sum a fixed order: two calls give the same bits, and a
// sample's row, counts, sdf_obj and wind_obj do not depend on the batch around it.
// Like ab_interaction this entry point is never captured in a hipGraph (DESIGN.md sections 19, 24, 27).
#include "ia_tile.h"

#define IAS_PART 4             // words per (sample, object vertex chunk): n_inside (int32) | sum of inside depths | largest inside depth | smallest distance

// The object row of sample b clamped into the table, its first vertex and its vertex count (at least 1, at most No_max).
__device__ __forceinline__ void ias_object(const int32_t* vert_off, int n_obj, const int64_t* obj_row, int b, int No_max, int& v0, int& nv) {
    const long r = (long)obj_row[b];
    const int row = (int)(r < 0 ? 0 : (r >= n_obj ? n_obj - 1 : r));
    v0 = vert_off[row];
    nv = min(max(vert_off[row + 1] - v0, 1), No_max);
}

// ---- launch 1: the hand vertices into the object's canonical frame --------------------------------------------------------------------------------
__global__ __launch_bounds__(IA_THREADS) void interaction_sym_canon_kernel(const float* __restrict__ hand_verts, int Nh, const float* __restrict__ rot,
                                                                            const float* __restrict__ tsl, float* __restrict__ hand_can) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * IA_THREADS + (int)threadIdx.x;
    if (i >= Nh) return;
    ia_object o;
#pragma unroll
    for (int k = 0; k < 9; ++k) o.R[k] = rot[(size_t)b * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.t[k] = tsl[(size_t)b * 3 + k];
    const float* hv = hand_verts + ((size_t)b * Nh + i) * 3;
    float x, y, z;
    ia_to_canonical(o, hv[0], hv[1], hv[2], x, y, z);
    float* hc = hand_can + ((size_t)b * Nh + i) * 3;
    hc[0] = x; hc[1] = y; hc[2] = z;
}

// ---- launch 2: the object vertices against the canonical hand, a fixed grid ----------------------------------------------------------------------
__global__ __launch_bounds__(IA_THREADS) void interaction_sym_verts_kernel(const float* __restrict__ hand_can, const int32_t* __restrict__ hand_faces, int Nh,
                                                                            int Fh, float hand_orient, const float* __restrict__ obj_verts,
                                                                            const int32_t* __restrict__ vert_off, int n_obj,
                                                                            const int64_t* __restrict__ obj_row, int No_max, float* __restrict__ sdf_obj,
                                                                            float* __restrict__ wind_obj, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float ts[9 * IA_TILE];
    __shared__ float s_part[4][IAS_PART];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * IA_THREADS + (int)threadIdx.x;
    int v0, nv;
    ias_object(vert_off, n_obj, obj_row, b, No_max, v0, nv);
    if ((int)blockIdx.x * IA_THREADS >= nv) {                                         // block-uniform: past the object's vertices
        if (q < No_max) {
            if (sdf_obj) sdf_obj[(size_t)b * No_max + q] = ab_nan();
            if (wind_obj) wind_obj[(size_t)b * No_max + q] = ab_nan();
        }
        return;
    }
    const bool live = q < nv;
    const int qc = live ? q : nv - 1;                                            // lanes past the end recompute the last vertex (masked below)
    const float* c = obj_verts + ((size_t)v0 + qc) * 3;
    const float qx = c[0], qy = c[1], qz = c[2];
    float sum = 0.f, comp = 0.f, best = __builtin_inff();
    ia_scan<true>(hand_can + (size_t)b * Nh * 3, Nh, hand_faces, Fh, ts, qx, qy, qz, sum, comp, best);
    const float w = hand_orient * (sum / IA_TWO_PI);                             // sum of half-angles / (2 pi) = sum of Omega / (4 pi)
    const float d = sqrtf(best);
    const bool in = live && w > 0.5f;
    if (q < No_max) {
        if (sdf_obj) sdf_obj[(size_t)b * No_max + q] = live ? (in ? -d : d) : ab_nan();
        if (wind_obj) wind_obj[(size_t)b * No_max + q] = live ? w : ab_nan();
    }
    const int cnt = (int)__popcll(__ballot(in));
    const float ps = wave_sum(in ? d : 0.f), pm = wave_max(in ? d : 0.f), mn = -wave_max(live ? -d : -__builtin_inff());
    if (lane == 0) { s_part[wave][0] = __int_as_float(cnt); s_part[wave][1] = ps; s_part[wave][2] = pm; s_part[wave][3] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* p = part + ((size_t)b * gridDim.x + blockIdx.x) * IAS_PART;
        p[0] = __int_as_float(((__float_as_int(s_part[0][0]) + __float_as_int(s_part[1][0])) + __float_as_int(s_part[2][0])) + __float_as_int(s_part[3][0]));
        p[1] = ((s_part[0][1] + s_part[1][1]) + s_part[2][1]) + s_part[3][1];
        p[2] = fmaxf(fmaxf(s_part[0][2], s_part[1][2]), fmaxf(s_part[2][2], s_part[3][2]));
        p[3] = fminf(fminf(s_part[0][3], s_part[1][3]), fminf(s_part[2][3], s_part[3][3]));
    }
}

// ---- launch 3: one thread per sample adds its live chunks in turn ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void interaction_sym_finalize_kernel(const float* __restrict__ part, const int32_t* __restrict__ vert_off, int n_obj,
                                                                       const int64_t* __restrict__ obj_row, int B, int No_max, int co, float contact_thr,
                                                                       float* __restrict__ rows, int32_t* __restrict__ counts) {
    const int b = blockIdx.x * 256 + (int)threadIdx.x;
    if (b >= B) return;
    int v0, nv;
    ias_object(vert_off, n_obj, obj_row, b, No_max, v0, nv);
    const int nc = (nv + IA_THREADS - 1) / IA_THREADS;                           // <= co: nv <= No_max; the chunks past it wrote nothing
    int n_in = 0;
    float ps = 0.f, pm = 0.f, mn = __builtin_inff();
    for (int c = 0; c < nc; ++c) {
        const float* p = part + ((size_t)b * co + c) * IAS_PART;
        n_in += __float_as_int(p[0]); ps += p[1]; pm = fmaxf(pm, p[2]); mn = fminf(mn, p[3]);
    }
    float* row = rows + (size_t)b * AB_IAS_ROW;
#pragma unroll
    for (int k = 0; k < AB_IAS_ROW; ++k) row[k] = ab_nan();
    row[AB_IAS_OBJ_PEN_MAX] = pm;
    row[AB_IAS_OBJ_PEN_MEAN] = n_in > 0 ? ps / (float)n_in : 0.f;
    row[AB_IAS_OBJ_MIN_DIST] = mn;
    row[AB_IAS_OBJ_INSIDE_FRAC] = (float)n_in / (float)nv;
    row[AB_IAS_OBJ_CONTACT] = (n_in > 0 || mn <= contact_thr) ? 1.f : 0.f;
    counts[(size_t)b * 2] = n_in;
    counts[(size_t)b * 2 + 1] = nv;
}

static inline long ias_chunks(int n) { return ((long)n + IA_THREADS - 1) / IA_THREADS; }

extern "C" long ab_interaction_sym_workspace(int B, int Nh, int No_max) {
    if (B < 1 || Nh < 1 || No_max < 1) return 0;
    return (long)B * ((long)Nh * 3 + ias_chunks(No_max) * IAS_PART) * (long)sizeof(float);
}

extern "C" int ab_interaction_sym(const float* hand_verts, const int32_t* hand_faces, int Nh, int Fh, float hand_orient, const float* obj_verts,
                                  const int32_t* vert_off, int n_obj, const int64_t* obj_row, const float* rot, const float* tsl, int B, int No_max,
                                  float contact_thr, float* rows, int32_t* counts, float* sdf_obj, float* wind_obj, void* workspace, void* stream) {
    if (!hand_verts || !hand_faces || !obj_verts || !vert_off || !obj_row || !rot || !tsl) return AB_EINVAL;
    if (!rows || !counts || !workspace) return AB_EINVAL;
    if (B < 1 || B > 65535 || Nh < 1 || Nh > (1 << 24) || Fh < 1 || Fh > (1 << 24) || No_max < 1 || No_max > (1 << 24) || n_obj < 1) return AB_EINVAL;
    if (!(contact_thr >= 0.f) || !(hand_orient == 1.f || hand_orient == -1.f)) return AB_EINVAL;
    const int ch = (int)ias_chunks(Nh), co = (int)ias_chunks(No_max);
    float* hand_can = (float*)workspace;
    float* part = hand_can + (size_t)B * Nh * 3;
    interaction_sym_canon_kernel<<<dim3(ch, B), IA_THREADS, 0, as_stream(stream)>>>(hand_verts, Nh, rot, tsl, hand_can);
    AB_LAUNCH_CHECK();
    interaction_sym_verts_kernel<<<dim3(co, B), IA_THREADS, 0, as_stream(stream)>>>(hand_can, hand_faces, Nh, Fh, hand_orient, obj_verts, vert_off, n_obj,
                                                                                   obj_row, No_max, sdf_obj, wind_obj, part);
    AB_LAUNCH_CHECK();
    interaction_sym_finalize_kernel<<<(B + 255) / 256, 256, 0, as_stream(stream)>>>(part, vert_off, n_obj, obj_row, B, No_max, co, contact_thr, rows, counts);
    AB_LAUNCH_CHECK();
    return 0;
}
