// The contact loss of Hasson et al. (CVPR 2019) on the device, eager only:
//   ab_contact_loss   per sample: repulsion of the hand vertices inside the posed object, attraction of the contact zones that do not touch
//                     it, and the analytic gradient for the hand vertices and the object pose, in one call.
//
// Definitions (the header, criterions.contact_loss_torch and the tests use the same ones).  The object of sample b is R_b can + t_b from
// the packed table of ab_interaction; a hand vertex q is taken into the canonical frame once, q' = R_b^T (q - t_b).
//   distance      d(q) and the closest point cp'(q) by the triangle region form of csrc/ia_tile.h, the first minimum in face order winning;
//                 the residual r' = q' - cp' is the sum of differences that form leaves (negated), d = |r'|.
//   box           box_b = the closed axis-aligned box of the object's canonical vertices (obj_box [n_obj,6]: lo xyz | hi xyz, exact in fp32,
//                 formed once per object by the host).
//   inside(q)     q' in box_b AND o w(q) > 0.5, w the generalised winding number and o the table's orientation (csrc/interact.hip).  A vertex
//                 outside the box is outside by definition and its winding number is not computed: the mesh lies in a half-space seen
//                 from there, so a closed mesh has w = 0 and an open one a small |w|.
//   candidates    the vertices that can contribute: q' in box_b, or zone_id >= 0.  Only they are scanned.
//   repulsion     rep_b = (1 / Nh) sum over inside vertices of rho tanh(d / rho).
//   attraction    zone_id int32 [Nh]: -1 (or any value outside 0 .. Z-1) = no zone.  For zone z, among its vertices that are NOT inside, d_z is
//                 the smallest d, the lowest vertex index winning ties; a zone without such a vertex contributes 0.  The box does not limit
//                 attraction.  att_b = (1 / max(Z, 1)) sum_z alpha tanh(d_z / alpha).
//   loss          (lambda_r sum_b m_b rep_b + lambda_a sum_b m_b att_b) / B, m_b = 0 for a sample whose obj_row is outside the table or
//                 whose mask is 0 (it still counts in B; nothing of it is scanned: rep_b = att_b = 0, counts 0, sdf NaN, gradients 0).
//   gradient      cp' minimises the distance, so it is held fixed: d = |q - (R_b cp' + t_b)|.  With n = R_b r' / d and s = sech^2(d / scale), a
//                 contributing vertex gets g_q = weight s n (0 when d == 0): weight lambda_r m_b / (B Nh), scale rho for an inside vertex,
//                 weight lambda_a m_b / (B max(Z, 1)), scale alpha for a zone's winner; the two sets are disjoint and every other vertex gets
//                 exactly 0.  g_tsl[b] = -sum g_q, g_rot[b] = -sum g_q cp'^T (the nine entries free, the convention of ab_chamfer_rigid).
//
// Launches (chunk = 256 candidates, tile = 512 triangles = 18 KiB of LDS).  (1) classify, one workgroup per sample: every vertex into the
// canonical frame, the candidates written as an ascending index list by ballots and prefix counts (fixed order), their state cleared, sdf
// NaN-filled.  (2) scan, a FIXED grid of ceil(Nh / 256) workgroups per sample; one past the list's length leaves at once, so the host reads
// nothing back.  Each lane keeps the minimum with its residual; a chunk that holds an in-box candidate also keeps the compensated half-angle
// sums.  A candidate leaves (r', d) and its state (exterior / inside) in per-VERTEX slots of the workspace, so nothing below depends on
// how the list was cut into chunks.  (3) finalize, one workgroup per sample: each zone's winner by a lexicographic (d, index) minimum, then one
// pass over the vertices in a fixed thread-strided order: repulsion terms, gradients, the 12 pose sums (wave butterflies, the four waves in
// turn).  (4) one workgroup sums the batch.  No atomics of any kind; two calls give the same bits; a sample's rep, att, sdf, counts and B x its
// gradients do not depend on the batch around it when B is a power of two.  AB_CL_SCAN_ALL lists every vertex of an unmasked sample
// instead of the candidates; whatever it scans beyond them is dropped, so every output has the same bits with and without it (sdf stays NaN
// and n_candidates stays the candidates' count).  Like the mesh losses before it this entry point is never captured in a hipGraph.
#include "ia_tile.h"

#define CL_HEAD 2              // int32 words per sample: listed vertices | candidates
#define CL_REC 4               // floats per vertex: r' [3] | d
#define CL_MAX_ZONES 16

struct cl_vertex { float qx, qy, qz; bool inbox; int zone; };

__device__ __forceinline__ int cl_table_row(const int64_t* obj_row, int n_obj, int b) {
    const long r = (long)obj_row[b];
    return (int)(r < 0 ? 0 : (r >= n_obj ? n_obj - 1 : r));
}

__device__ __forceinline__ bool cl_sample_live(const int64_t* obj_row, int n_obj, const float* mask, int b) {
    const long r = (long)obj_row[b];
    return r >= 0 && r < n_obj && (!mask || mask[b] != 0.f);
}

// Vertex i of sample b in the canonical frame, its box test (closed) and its zone (-1 for any id outside 0 .. Z-1).
__device__ __forceinline__ cl_vertex cl_load_vertex(const ia_object& o, const float* box, const float* hand_verts, const int32_t* zone_id, int Nh, int Z,
                                                    int b, int i) {
    cl_vertex v;
    const float* hv = hand_verts + ((size_t)b * Nh + i) * 3;
    ia_to_canonical(o, hv[0], hv[1], hv[2], v.qx, v.qy, v.qz);
    v.inbox = v.qx >= box[0] && v.qx <= box[3] && v.qy >= box[1] && v.qy <= box[4] && v.qz >= box[2] && v.qz <= box[5];
    const int z = Z > 0 ? zone_id[i] : -1;
    v.zone = (z >= 0 && z < Z) ? z : -1;
    return v;
}

// ---- launch 1: classify and compact, one workgroup per sample ---------------------------------------------------------------------------------
__global__ __launch_bounds__(IA_THREADS) void contact_classify_kernel(const float* __restrict__ hand_verts, const int32_t* __restrict__ zone_id, int Nh, int Z,
                                                                       const float* __restrict__ obj_verts, const int32_t* __restrict__ obj_faces,
                                                                       const int32_t* __restrict__ vert_off, const int32_t* __restrict__ face_off,
                                                                       const float* __restrict__ obj_orient, const float* __restrict__ obj_box, int n_obj,
                                                                       const int64_t* __restrict__ obj_row, const float* __restrict__ rot,
                                                                       const float* __restrict__ tsl, const float* __restrict__ mask, int flags,
                                                                       int32_t* __restrict__ head, int32_t* __restrict__ list, int32_t* __restrict__ st,
                                                                       float* __restrict__ sdf) {
    __shared__ int s_cnt[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool sample = cl_sample_live(obj_row, n_obj, mask, b);
    const ia_object o = ia_load_object(obj_verts, obj_faces, vert_off, face_off, obj_orient, n_obj, obj_row, rot, tsl, b);
    const float* box = obj_box + (size_t)cl_table_row(obj_row, n_obj, b) * 6;
    int n_list = 0, n_cand = 0;                                                  // the same in every thread
    for (int i0 = 0; i0 < Nh; i0 += IA_THREADS) {
        const int i = i0 + (int)threadIdx.x;
        bool cand = false, listed = false;
        if (i < Nh) {
            const cl_vertex v = cl_load_vertex(o, box, hand_verts, zone_id, Nh, Z, b, i);
            cand = sample && (v.inbox || v.zone >= 0);
            listed = sample && (cand || (flags & AB_CL_SCAN_ALL));
            st[(size_t)b * Nh + i] = 0;
            if (sdf) sdf[(size_t)b * Nh + i] = ab_nan();
        }
        const unsigned long long bl = __ballot(listed), bc = __ballot(cand);     // every lane votes
        if (lane == 0) s_cnt[wave] = (int)__popcll(bl) | ((int)__popcll(bc) << 8);
        __syncthreads();
        int before = 0, tot_l = 0, tot_c = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = s_cnt[w];
            before += w < wave ? (c & 255) : 0;
            tot_l += c & 255; tot_c += c >> 8;
        }
        if (listed) list[(size_t)b * Nh + n_list + before + (int)__popcll(bl & ((1ull << lane) - 1ull))] = i;      // ascending: round, wave, lane
        n_list += tot_l; n_cand += tot_c;
        __syncthreads();
    }
    if (threadIdx.x == 0) { head[(size_t)b * CL_HEAD] = n_list; head[(size_t)b * CL_HEAD + 1] = n_cand; }
}

// ---- launch 2: the listed vertices against the object, a fixed grid ------------------------------------------------------------------------------
__global__ __launch_bounds__(IA_THREADS) void contact_scan_kernel(const float* __restrict__ hand_verts, const int32_t* __restrict__ zone_id, int Nh, int Z,
                                                                   const float* __restrict__ obj_verts, const int32_t* __restrict__ obj_faces,
                                                                   const int32_t* __restrict__ vert_off, const int32_t* __restrict__ face_off,
                                                                   const float* __restrict__ obj_orient, const float* __restrict__ obj_box, int n_obj,
                                                                   const int64_t* __restrict__ obj_row, const float* __restrict__ rot,
                                                                   const float* __restrict__ tsl, const int32_t* __restrict__ head,
                                                                   const int32_t* __restrict__ list, int32_t* __restrict__ st, float* __restrict__ rec,
                                                                   float* __restrict__ sdf) {
    __shared__ __attribute__((aligned(16))) float ts[9 * IA_TILE];
    __shared__ int s_any[4];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = head[(size_t)b * CL_HEAD];                                     // <= Nh
    if ((long long)blockIdx.x * IA_THREADS >= n) return;                         // block-uniform: past the list
    const int k = blockIdx.x * IA_THREADS + (int)threadIdx.x;
    const bool live = k < n;
    const int i = min(max(list[(size_t)b * Nh + (live ? k : n - 1)], 0), Nh - 1);      // lanes past the end recompute the last entry (masked below)
    const ia_object o = ia_load_object(obj_verts, obj_faces, vert_off, face_off, obj_orient, n_obj, obj_row, rot, tsl, b);
    const float* box = obj_box + (size_t)cl_table_row(obj_row, n_obj, b) * 6;
    const cl_vertex v = cl_load_vertex(o, box, hand_verts, zone_id, Nh, Z, b, i);
    const int wave_any = __ballot(live && v.inbox) != 0ull;                      // every lane votes
    if (lane == 0) s_any[wave] = wave_any;
    __syncthreads();
    const bool any = (s_any[0] | s_any[1] | s_any[2] | s_any[3]) != 0;           // block-uniform: a chunk without an in-box vertex needs no winding number
    ia_hit h = {__builtin_inff(), 0.f, 0.f, 0.f, 0.f, 0.f};
    const float qx = v.qx, qy = v.qy, qz = v.qz;
    if (any)
        ia_scan_tiles(o.verts, o.nv, o.faces, o.nf, ts, [&](float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
            ia_tri_cp<true>(ax, ay, az, bx, by, bz, cx, cy, cz, qx, qy, qz, h);
        });
    else
        ia_scan_tiles(o.verts, o.nv, o.faces, o.nf, ts, [&](float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
            ia_tri_cp<false>(ax, ay, az, bx, by, bz, cx, cy, cz, qx, qy, qz, h);
        });
    if (live && (v.inbox || v.zone >= 0)) {                                      // what AB_CL_SCAN_ALL scans beyond the candidates is dropped here
        const bool inside = v.inbox && o.orient * (h.sum / IA_TWO_PI) > 0.5f;
        const float d = sqrtf(h.best);
        float* r = rec + ((size_t)b * Nh + i) * CL_REC;
        r[0] = -h.rx; r[1] = -h.ry; r[2] = -h.rz; r[3] = d;                      // r' = q' - cp'
        st[(size_t)b * Nh + i] = inside ? 2 : 1;
        if (sdf) sdf[(size_t)b * Nh + i] = inside ? -d : d;
    }
}

// ---- launch 3: the zones' winners, the sample's terms and its gradients, one workgroup per sample --------------------------------------------------
__global__ __launch_bounds__(IA_THREADS) void contact_finalize_kernel(const float* __restrict__ hand_verts, const int32_t* __restrict__ zone_id, int Nh, int Z,
                                                                       const float* __restrict__ obj_verts, const int32_t* __restrict__ obj_faces,
                                                                       const int32_t* __restrict__ vert_off, const int32_t* __restrict__ face_off,
                                                                       const float* __restrict__ obj_orient, const float* __restrict__ obj_box, int n_obj,
                                                                       const int64_t* __restrict__ obj_row, const float* __restrict__ rot,
                                                                       const float* __restrict__ tsl, const int32_t* __restrict__ head,
                                                                       const int32_t* __restrict__ st, const float* __restrict__ rec, float rho, float alpha,
                                                                       float w_rep, float w_att, float* __restrict__ rep, float* __restrict__ att,
                                                                       int32_t* __restrict__ counts, float* __restrict__ g_hand, float* __restrict__ g_rot,
                                                                       float* __restrict__ g_tsl) {
    __shared__ float s_d[4];
    __shared__ int s_i[4];
    __shared__ float win_d[CL_MAX_ZONES];
    __shared__ int win_i[CL_MAX_ZONES];
    __shared__ float s_red[4][14];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ia_object o = ia_load_object(obj_verts, obj_faces, vert_off, face_off, obj_orient, n_obj, obj_row, rot, tsl, b);
    const float* box = obj_box + (size_t)cl_table_row(obj_row, n_obj, b) * 6;
    const int32_t* sb = st + (size_t)b * Nh;
    const float* rb = rec + (size_t)b * Nh * CL_REC;
    // each zone's exterior vertex of smallest d, the lowest index among equals: a lexicographic minimum, whatever the order it is taken in
    for (int z = 0; z < Z; ++z) {
        float bd = __builtin_inff();
        int bi = 0x7fffffff;
        for (int i = threadIdx.x; i < Nh; i += IA_THREADS) {
            const int zi = zone_id[i];
            if (zi == z && sb[i] == 1) {
                const float d = rb[(size_t)i * CL_REC + 3];
                if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const float od = __shfl_xor(bd, s, 64);
            const int oi = __shfl_xor(bi, s, 64);
            if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
        }
        if (lane == 0) { s_d[wave] = bd; s_i[wave] = bi; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float d = s_d[0];
            int i = s_i[0];
            for (int w = 1; w < 4; ++w)
                if (s_d[w] < d || (s_d[w] == d && s_i[w] < i)) { d = s_d[w]; i = s_i[w]; }
            win_d[z] = d; win_i[z] = i == 0x7fffffff ? -1 : i;
        }
        __syncthreads();
    }
    // one pass over the vertices, thread-strided: repulsion terms, gradients, pose sums
    float acc[14];                                                               // g_rot [9] | g_tsl [3] | repulsion | n_inside (int bits)
#pragma unroll
    for (int k = 0; k < 14; ++k) acc[k] = 0.f;
    int n_in = 0;
    for (int i = threadIdx.x; i < Nh; i += IA_THREADS) {
        const int s = sb[i];
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (s != 0) {
            const cl_vertex v = cl_load_vertex(o, box, hand_verts, zone_id, Nh, Z, b, i);
            const float* r = rb + (size_t)i * CL_REC;
            const float rx = r[0], ry = r[1], rz = r[2], d = r[3];
            float wgt = 0.f, scale = 1.f;
            bool on = false;
            if (s == 2) {
                on = true; wgt = w_rep; scale = rho;
                acc[12] += rho * tanhf(d / rho);
                ++n_in;
            } else if (v.zone >= 0 && win_i[v.zone] == i) {
                on = true; wgt = w_att; scale = alpha;
            }
            if (on && d > 0.f && g_hand) {
                const float e = expf(-2.f * (d / scale)), ope = 1.f + e;
                const float c = (wgt * ((4.f * e) / (ope * ope))) / d;            // weight sech^2(d / scale) / d
                gx = c * ia_dot(o.R[0], o.R[1], o.R[2], rx, ry, rz);             // n = R r' / d
                gy = c * ia_dot(o.R[3], o.R[4], o.R[5], rx, ry, rz);
                gz = c * ia_dot(o.R[6], o.R[7], o.R[8], rx, ry, rz);
                const float cx = v.qx - rx, cy = v.qy - ry, cz = v.qz - rz;       // cp' = q' - r'
                acc[0] -= gx * cx; acc[1] -= gx * cy; acc[2] -= gx * cz;
                acc[3] -= gy * cx; acc[4] -= gy * cy; acc[5] -= gy * cz;
                acc[6] -= gz * cx; acc[7] -= gz * cy; acc[8] -= gz * cz;
                acc[9] -= gx; acc[10] -= gy; acc[11] -= gz;
            }
        }
        if (g_hand) {
            float* g = g_hand + ((size_t)b * Nh + i) * 3;
            g[0] = gx; g[1] = gy; g[2] = gz;
        }
    }
#pragma unroll
    for (int k = 0; k < 13; ++k) {
        const float t = wave_sum(acc[k]);
        if (lane == 0) s_red[wave][k] = t;
    }
    int cnt = n_in;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
    if (lane == 0) s_red[wave][13] = __int_as_float(cnt);
    __syncthreads();
    if (threadIdx.x == 0) {
        float tot[13];
        for (int k = 0; k < 13; ++k) tot[k] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
        const int n_inside = ((__float_as_int(s_red[0][13]) + __float_as_int(s_red[1][13])) + __float_as_int(s_red[2][13])) + __float_as_int(s_red[3][13]);
        float a = 0.f;
        for (int z = 0; z < Z; ++z)
            if (win_i[z] >= 0) a += alpha * tanhf(win_d[z] / alpha);
        rep[b] = tot[12] / (float)Nh;
        att[b] = a / (float)max(Z, 1);
        counts[(size_t)b * 2] = n_inside;
        counts[(size_t)b * 2 + 1] = head[(size_t)b * CL_HEAD + 1];
        if (g_hand) {
            for (int k = 0; k < 9; ++k) g_rot[(size_t)b * 9 + k] = tot[k];
            for (int k = 0; k < 3; ++k) g_tsl[(size_t)b * 3 + k] = tot[9 + k];
        }
    }
}

// ---- launch 4: the batch ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IA_THREADS) void contact_batch_kernel(const float* __restrict__ rep, const float* __restrict__ att, int B, float lambda_r,
                                                                    float lambda_a, float* __restrict__ loss) {
    __shared__ float s_sum[4][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float r = 0.f, a = 0.f;
    for (int b = threadIdx.x; b < B; b += IA_THREADS) { r += rep[b]; a += att[b]; }
    r = wave_sum(r); a = wave_sum(a);
    if (lane == 0) { s_sum[wave][0] = r; s_sum[wave][1] = a; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float sr = ((s_sum[0][0] + s_sum[1][0]) + s_sum[2][0]) + s_sum[3][0], sa = ((s_sum[0][1] + s_sum[1][1]) + s_sum[2][1]) + s_sum[3][1];
        loss[0] = (lambda_r * sr + lambda_a * sa) / (float)B;
    }
}

static inline long cl_chunks(int Nh) { return ((long)Nh + IA_THREADS - 1) / IA_THREADS; }

extern "C" long ab_contact_loss_workspace(int B, int Nh) {
    if (B < 1 || Nh < 1) return 0;
    return (long)B * (CL_HEAD + (long)Nh * (2 + CL_REC)) * (long)sizeof(float);
}

extern "C" int ab_contact_loss(const float* hand_verts, const int32_t* zone_id, int Nh, int Z, const float* obj_verts, const int32_t* obj_faces,
                               const int32_t* vert_off, const int32_t* face_off, const float* obj_orient, const float* obj_box, int n_obj,
                               const int64_t* obj_row, const float* rot, const float* tsl, const float* mask, int B, float rho, float alpha,
                               float lambda_r, float lambda_a, int flags, float* loss, float* rep, float* att, int32_t* counts, float* sdf,
                               float* g_hand, float* g_rot, float* g_tsl, void* workspace, void* stream) {
    if (!hand_verts || !obj_verts || !obj_faces || !vert_off || !face_off || !obj_orient || !obj_box || !obj_row || !rot || !tsl) return AB_EINVAL;
    if (!loss || !rep || !att || !counts || !workspace) return AB_EINVAL;
    if (B < 1 || B > 65535 || Nh < 1 || Nh > (1 << 24) || Z < 0 || Z > CL_MAX_ZONES || n_obj < 1) return AB_EINVAL;
    if (Z > 0 && !zone_id) return AB_EINVAL;
    if (!(rho > 0.f) || !(rho < __builtin_inff()) || !(alpha > 0.f) || !(alpha < __builtin_inff())) return AB_EINVAL;
    if (!(lambda_r == lambda_r) || !(lambda_a == lambda_a) || (flags & ~AB_CL_SCAN_ALL)) return AB_EINVAL;
    if ((g_hand != nullptr) != (g_rot != nullptr) || (g_hand != nullptr) != (g_tsl != nullptr)) return AB_EINVAL;      // all three or none
    int32_t* head = (int32_t*)workspace;
    int32_t* list = head + (size_t)B * CL_HEAD;
    int32_t* st = list + (size_t)B * Nh;
    float* rec = (float*)(st + (size_t)B * Nh);
    const float w_rep = lambda_r / ((float)B * (float)Nh), w_att = lambda_a / ((float)B * (float)(Z > 1 ? Z : 1));
    hipStream_t s = as_stream(stream);
    contact_classify_kernel<<<B, IA_THREADS, 0, s>>>(hand_verts, zone_id, Nh, Z, obj_verts, obj_faces, vert_off, face_off, obj_orient, obj_box, n_obj, obj_row,
                                                    rot, tsl, mask, flags, head, list, st, sdf);
    AB_LAUNCH_CHECK();
    contact_scan_kernel<<<dim3((unsigned)cl_chunks(Nh), B), IA_THREADS, 0, s>>>(hand_verts, zone_id, Nh, Z, obj_verts, obj_faces, vert_off, face_off, obj_orient,
                                                                                obj_box, n_obj, obj_row, rot, tsl, head, list, st, rec, sdf);
    AB_LAUNCH_CHECK();
    contact_finalize_kernel<<<B, IA_THREADS, 0, s>>>(hand_verts, zone_id, Nh, Z, obj_verts, obj_faces, vert_off, face_off, obj_orient, obj_box, n_obj, obj_row,
                                                    rot, tsl, head, st, rec, rho, alpha, w_rep, w_att, rep, att, counts, g_hand, g_rot, g_tsl);
    AB_LAUNCH_CHECK();
    contact_batch_kernel<<<1, IA_THREADS, 0, s>>>(rep, att, B, lambda_r, lambda_a, loss);
    AB_LAUNCH_CHECK();
    return 0;
}
