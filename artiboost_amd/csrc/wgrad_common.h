// Device pieces shared by the weight-gradient kernels (wgrad3x3.hip, wgrad_gemm2.hip, conv_wgrad.hip): the transpose-read
// fragment pair, the swizzled LDS image both DMA kernels use, the MFMA step and the 32x32 accumulator store.
#pragma once
#include "conv_common.h"

typedef short short4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) short4_t lds_short4;

// One 16 x 32 bf16 MFMA operand through ds_read_b64_tr_b16: k rows 0..3 (+8 for the upper lane groups) at addr_lo, rows 4..7 at addr_hi.
__device__ __forceinline__ uint4 tr_pair(unsigned addr_lo, unsigned addr_hi) {
    short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4*)(size_t)addr_lo);
    short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4*)(size_t)addr_hi);
    uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
    return make_uint4(l2.x, l2.y, h2.x, h2.y);
}

// LDS image of a tile of PITCH-byte rows filled by lane-linear DMA (no padding): the 16-byte chunk c of row r sits in slot
// c ^ (f(r) << 2), f(r) = (r >> 1) & 1 for 128-byte rows and r & 3 for longer ones, which puts the four consecutive rows x 64 bytes
// a transpose read touches on four distinct 64-byte bank groups.  The fill side fetches the chunk that belongs in its slot with the
// same function (the XOR is its own inverse).
template <int PITCH> __device__ __forceinline__ int swz_chunk(int row, int chunk) {
    return chunk ^ ((PITCH == 128 ? (row >> 1) & 1 : row & 3) << 2);
}
// byte offset of element (row, col) in that image
template <int PITCH> __device__ __forceinline__ unsigned frag_addr(int row, int col) {
    return row * PITCH + (swz_chunk<PITCH>(row, col >> 3) << 4) + (col & 7) * 2;
}

__device__ __forceinline__ void mfma16(f32x16& acc, uint4 a, uint4 b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

// a wave's 32x32 accumulator to out[row0 + ..][col0 + ..] (row length ld); GUARD: only rows below `rows`; SCALE: times `scale`
template <bool GUARD = false, bool SCALE = false>
__device__ __forceinline__ void store_acc_tile(float* out, int ld, int row0, int col0, const f32x16& acc, int rows = 0, float scale = 1.f) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), col = col0 + (lane & 31);
        if (!GUARD || row < rows) out[(long)row * ld + col] = SCALE ? acc[r] * scale : acc[r];
    }
}
