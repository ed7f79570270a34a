// The LDS-tiled brute-force nearest-neighbour scan of ab_chamfer_rigid (csrc/mesh_align.hip) and ab_mesh_metrics (csrc/mesh_metrics.hip):
// one query point per thread, the scanned cloud staged in SoA tiles so that one wave-uniform (broadcast) ds_read_b128 per coordinate serves
// four scanned points for 64 queries.  A lane keeps a running minimum of the sum of squared differences (never |x|^2 + |y|^2 - 2 x.y) and,
// with INDEX, its index; strict <: the first minimum wins, as argmin does.
#pragma once
#include "common.h"

struct nn_hit { float d2; int idx; };                                             // idx stays 0 without INDEX

// vs: 3 * TILE floats of LDS, 16-byte aligned.  stage(src, a0, a1, a2) forms the scanned point whose first coordinate sits at float
// offset src of its cloud; it is called by every thread of the workgroup, which must reach this call together (two barriers per tile).
template <int TILE, int THREADS, bool INDEX, typename Stage>
__device__ __forceinline__ nn_hit nn_tile_scan(float* vs, int ns, float px, float py, float pz, Stage stage) {
    nn_hit hit = {__builtin_inff(), 0};
    for (int v0 = 0; v0 < ns; v0 += TILE) {
        const int n = min(TILE, ns - v0);
        const int npad = (n + 3) & ~3;                                           // <= TILE (a multiple of 4)
        __syncthreads();
        for (int j = threadIdx.x; j < npad; j += THREADS) {
            float a0, a1, a2;
            stage((size_t)(v0 + (j < n ? j : 0)) * 3, a0, a1, a2);               // the tail repeats the tile's first point: under strict < it never wins
            vs[j] = a0; vs[TILE + j] = a1; vs[2 * TILE + j] = a2;
        }
        __syncthreads();
        for (int j = 0; j < npad; j += 4) {
            const float4 x4 = *(const float4*)&vs[j], y4 = *(const float4*)&vs[TILE + j], z4 = *(const float4*)&vs[2 * TILE + j];
            const float xs[4] = {x4.x, x4.y, x4.z, x4.w}, ys[4] = {y4.x, y4.y, y4.z, y4.w}, zs[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float dx = px - xs[u], dy = py - ys[u], dz = pz - zs[u];
                const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                if (d < hit.d2) { hit.d2 = d; if (INDEX) hit.idx = v0 + j + u; }
            }
        }
    }
    return hit;
}
