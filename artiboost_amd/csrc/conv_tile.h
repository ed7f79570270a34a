// Device pieces shared by the forward / data-gradient convolution kernels (conv3x3.hip, conv3x3r.hip, conv2x2.hip, convp.hip and, for its
// fp32 row bodies, conv_gemm2.hip): the swizzled LDS image of the resident-patch kernels, the split-bf16 MFMA step, the fp32 epilogue
// (staging store, 4-channel row bodies, partial-row reduction), the LDS budget of a tile and the launch helper.
// What is NOT here differs from kernel to kernel: the K-loop schedules (issue order, counted vmcnt waits, barriers, ring depths).
// conv3x3.hip's kernel keeps the image and the fp32 epilogue spelled out in its own body (measured: see the top of that file); it follows
// the format documented here and calls split_planes / reduce_partial_rows<8> only.
#pragma once
#include "conv_common.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;

// ---- LDS image.  Both operands are lane-linear global_load_lds fills (a 1-KiB wave instruction = 8 rows x 8 slots of 16 bytes, lane & 7 the
// slot), so the bank-conflict swizzle sits on the SOURCE address: slot s of a 128-byte row holds the row's logical chunk s ^ key(row), and a
// fragment read applies the same XOR (it is its own inverse).
//   patch : pixel pp = py * PW + px at byte pp * 128, key (px >> 1) & 7
//           (8-wide tiles, where a ds_read_b128 lane group spans four patch rows: ((px >> 1) & 3) | ((py & 1) << 2), on an odd row pitch, so
//           that consecutive patch rows alternate the 128-byte half -- with the px-only key every fragment read of that tile was a 2-way bank
//           conflict: SQ_LDS_BANK_CONFLICT 0.33 of the LDS cycles)
//   weight: row r (output channel) at byte r * 128, key (r >> 1) & 7
// Both are conflict-free for the 16-lane groups of ds_read_b128 (for 16-wide tiles two half-rows complement each other).
// A bf16 row carries 64 channels as chunks 0..7; a split-bf16 row carries 32 channels as [hi: chunks 0..3][lo: chunks 4..7].
template <int TW> __device__ __forceinline__ int patch_key(int py, int px) { return TW == 8 ? (((px >> 1) & 3) | ((py & 1) << 2)) : ((px >> 1) & 7); }
__device__ __forceinline__ int wrow_key(int r) { return (r >> 1) & 7; }
// 8-wide tiles: a tap one patch row down flips the (py & 1) bit of the key, i.e. bit 6 of the fragment address (row bases are 128-byte aligned)
template <int TW> __device__ __forceinline__ unsigned tap_row_flip(int dh) { return (TW == 8 && (dh & 1)) ? 64u : 0u; }
// fill side: the logical chunk this lane's slot holds; of a split-bf16 row: its plane and its element offset inside the 32-channel chunk
__device__ __forceinline__ int fill_chunk(int lane, int key) { return (lane & 7) ^ key; }
__device__ __forceinline__ int chunk_lo(int c) { return c & 4; }      // non-zero: the lo plane
__device__ __forceinline__ int chunk_elem(int c) { return (c & 3) * 8; }
// fragment side: byte offset of logical chunk `slot` of row `row` (bf16 / split-bf16 32x32x16 operands: slot = 2 * k-slice + (lane >> 5))
__device__ __forceinline__ unsigned frag_off(int row, int slot, int key) { return row * 128 + ((slot ^ key) << 4); }

// ---- accumulators
template <int TM, int TN> __device__ __forceinline__ void zero_acc(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// ---- the split-bf16 step of the resident-patch kernels, two calls (a knock-out build skips each on its own).  Slots 0, 1 of a row are the hi
// k-slices (16 channels each), slots 2, 3 the lo planes of the same channels.  a_rel / b_rel: per-lane LDS addresses of (tile, slot); a tap
// shifts the patch address by `aoff` (and `aflip`, see tap_row_flip), `boff` selects the ring stage.
template <int TM, int TN>
__device__ __forceinline__ void x3_read_frags(u32x4 (&fa)[4][TM], u32x4 (&fb)[4][TN], const unsigned (&a_rel)[TM][4], unsigned aflip, unsigned aoff,
                                              const unsigned (&b_rel)[TN][4], unsigned boff) {
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[k2 + 2 * h][i] = *(const lds_u32x4*)((a_rel[i][k2 + 2 * h] ^ aflip) + aoff);
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[k2 + 2 * h][j] = *(const lds_u32x4*)(b_rel[j][k2 + 2 * h] + boff);
        }
    }
}
// hi*hi on `acc`; the two cross products on a second chain (more independent MFMA chains per SIMD, and the small terms are summed among
// themselves before they meet the large one).  Weights as the first operand: the accumulator is the TRANSPOSED tile (a lane owns one pixel).
template <int TM, int TN>
__device__ __forceinline__ void x3_mfma_step(f32x16 (&acc)[TM][TN], f32x16 (&accx)[TM][TN], const u32x4 (&fa)[4][TM], const u32x4 (&fb)[4][TN]) {
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const bf16x8 bh = __builtin_bit_cast(bf16x8, fb[k2][j]), bl = __builtin_bit_cast(bf16x8, fb[k2 + 2][j]);
                const bf16x8 ah = __builtin_bit_cast(bf16x8, fa[k2][i]), al = __builtin_bit_cast(bf16x8, fa[k2 + 2][i]);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, ah, acc[i][j], 0, 0, 0);
                accx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bh, al, accx[i][j], 0, 0, 0);
                accx[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bl, ah, accx[i][j], 0, 0, 0);
            }
    }
}

// ---- fp32 epilogue of the split-bf16 launches.  The MFMAs computed the transposed tile (weights x pixels), so in the C/D layout a lane owns
// ONE pixel (lane & 31) and per register quad four consecutive channels: one 16-byte LDS store of acc + accx into the pixel-major staging
// tile (row pitch BN * 4 + 16 bytes: + 16 spreads the rows over the banks), from which the rows leave as 16-byte vectors.
template <int BN> constexpr int stage_pitch_f32() { return BN * 4 + 16; }
template <int BN, int TM, int TN>
__device__ __forceinline__ void stage_store_f32(unsigned char* smem, const f32x16 (&acc)[TM][TN], const f32x16 (&accx)[TM][TN], int wave_m, int wave_n, int lane) {
    const int l32 = lane & 31, fhalf = lane >> 5;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row = (wave_m * TM + i) * 32 + l32;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const int cl = (wave_n * TN + j) * 32 + 8 * q4 + 4 * fhalf;
                float4 w;
                w.x = acc[i][j][q4 * 4] + accx[i][j][q4 * 4]; w.y = acc[i][j][q4 * 4 + 1] + accx[i][j][q4 * 4 + 1];
                w.z = acc[i][j][q4 * 4 + 2] + accx[i][j][q4 * 4 + 2]; w.w = acc[i][j][q4 * 4 + 3] + accx[i][j][q4 * 4 + 3];
                *(float4*)(smem + row * stage_pitch_f32<BN>() + cl * 4) = w;
            }
        }
    }
}

// Row bodies: what a thread does with one group of consecutive channels of one staged row.  A thread keeps the same channel group over all
// its rows, so its per-channel sums (s, q) stay in registers until reduce_partial_rows.
// BatchNorm partials of the values as stored: (sum, sum of squares)
__device__ __forceinline__ void stat4(float (&s)[4], float (&q)[4], const float4 v) {
    s[0] += v.x; q[0] += v.x * v.x; s[1] += v.y; q[1] += v.y * v.y;
    s[2] += v.z; q[2] += v.z * v.z; s[3] += v.w; q[3] += v.w * v.w;
}
// eval-mode fold of the BatchNorm (+ ReLU) that follows: bn_apply_x3_kernel's own expression (norm_pool.hip), bit-identical to conv + apply pass
__device__ __forceinline__ void affine_relu4(float4& v, const float* scale, const float* shift, int relu) {
    const float4 sc = *(const float4*)scale, sh = *(const float4*)shift;
    v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
    if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
}
// W fp32 values as the operand planes the next convolution reads: hi = bf16(v), lo = bf16(v - hi), two channels per word
template <int W> __device__ __forceinline__ void split_planes(const float (&v)[W], uint32_t (&h)[W / 2], uint32_t (&l)[W / 2]) {
#pragma unroll
    for (int k = 0; k < W / 2; ++k) {
        h[k] = pack_bf16x2(v[2 * k], v[2 * k + 1]);
        l[k] = pack_bf16x2(v[2 * k] - __uint_as_float(h[k] << 16), v[2 * k + 1] - __uint_as_float(h[k] & 0xffff0000u));
    }
}
__device__ __forceinline__ void store_planes4(void* out_hi, void* out_lo, long o, const float4 v) {
    const float f[4] = {v.x, v.y, v.z, v.w};
    uint32_t h[2], l[2];
    split_planes<4>(f, h, l);
    *(uint2*)((bf16_t*)out_hi + o) = make_uint2(h[0], h[1]); *(uint2*)((bf16_t*)out_lo + o) = make_uint2(l[0], l[1]);
}

// Fused BatchNorm-backward: the tile is the gradient arriving at relu(bn(y) [+ residual]).  Four channels' [scale | shift | mean | invstd]
// of the BatchNorm record bnp (4 x Cn floats); a channel group past Cn (ok = false) reads nothing.
struct BnBwdCh4 {
    float sc[4], sh[4], mean[4], istd[4];
    __device__ __forceinline__ void load(const float* bnp, int Cn, int col, bool ok = true) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sc[k] = ok ? bnp[col + k] : 0.f; sh[k] = ok ? bnp[Cn + col + k] : 0.f;
            mean[k] = ok ? bnp[2 * Cn + col + k] : 0.f; istd[k] = ok ? bnp[3 * Cn + col + k] : 0.f;
        }
    }
};
// dz = the staged gradient v4 where the activation was alive -- by the stored activation's hi plane (has_mask: m2 = two packed words of it),
// or by bn_apply's own expression on y4 = bn_y (no residual was added) -- else 0; (s, q) gain (dz, dz * xhat), xhat = (y - mean) * invstd
__device__ __forceinline__ float4 bn_bwd_mask4(const float4 v4, const float4 y4, const uint2 m2, bool has_mask, const BnBwdCh4& p, float (&s)[4], float (&q)[4]) {
    float v[4] = {v4.x, v4.y, v4.z, v4.w};
    const float y[4] = {y4.x, y4.y, y4.z, y4.w};
    const float m[4] = {__uint_as_float(m2.x << 16), __uint_as_float(m2.x & 0xffff0000u), __uint_as_float(m2.y << 16), __uint_as_float(m2.y & 0xffff0000u)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool dead = has_mask ? !(m[k] > 0.f) : !(y[k] * p.sc[k] + p.sh[k] > 0.f);
        v[k] = dead ? 0.f : v[k];
        s[k] += v[k]; q[k] += v[k] * ((y[k] - p.mean[k]) * p.istd[k]);
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}

// Partial-row reduction: NT threads, each with the sums (s, q) of one group of G channels over its rows -- thread tid owns group tid % (BN / G)
// -- meet in sp [NT / (BN / G)][BN][2]; one thread per channel then adds the row groups in ascending order and writes row `row` of
// part_out [rows][Cn][2].  Ends in no barrier; the caller has synchronised before sp is overwritten.
template <int G, int BN, int NT>
__device__ __forceinline__ void reduce_partial_rows(float* sp, const float (&s)[G], const float (&q)[G], float* part_out, long row, int Cn, int n0) {
    constexpr int CPR = BN / G;
    static_assert(NT % CPR == 0, "a thread keeps one channel group over all its rows");
    const int tid = threadIdx.x, rg = tid / CPR, cb = (tid % CPR) * G;
#pragma unroll
    for (int k = 0; k < G; ++k) { sp[(rg * BN + cb + k) * 2] = s[k]; sp[(rg * BN + cb + k) * 2 + 1] = q[k]; }
    __syncthreads();
    for (int c = tid; c < BN; c += NT) {
        const int col = n0 + c;
        if (col < Cn) {
            float s2 = 0.f, q2 = 0.f;
            for (int r = 0; r < NT / CPR; ++r) { s2 += sp[(r * BN + c) * 2]; q2 += sp[(r * BN + c) * 2 + 1]; }
            part_out[(row * Cn + col) * 2] = s2;
            part_out[(row * Cn + col) * 2 + 1] = q2;
        }
    }
}

// ---- LDS budget of a resident-patch tile, read by the kernel and by its launcher: NPIX patch pixels of 128 bytes filled by NW waves, BN weight
// rows per ring stage, BM x BN outputs through the fp32 staging tile, whose space the partial rows reuse.
template <int NPIX_, int NW, int BM, int BN> struct PatchTileLds {
    static constexpr int NT = 64 * NW;
    static constexpr int NPIX = NPIX_;
    static constexpr int PI = (NPIX + 7) / 8;                 // 1-KiB fill instructions per patch
    static constexpr int LP = (PI + NW - 1) / NW;             // ... per wave
    static constexpr int PATCH_BYTES = LP * NW * 1024;        // every wave issues exactly LP fills; the tail past NPIX is slack
    static constexpr int BBYTES = BN * 128;                   // one ring stage of weights
    static constexpr int STAGE_F32 = BM * stage_pitch_f32<BN>();
    static constexpr int PART_F32 = (NT / (BN / 4)) * BN * 8;
    // a split-bf16 kernel with NRING weight stages and NPATCH patch buffers: the K loop's image, then the epilogue's over it
    static constexpr int x3_lds(int nring, int npatch) {
        const int ring = nring * BBYTES + npatch * PATCH_BYTES;
        return ring > STAGE_F32 ? (ring > PART_F32 ? ring : PART_F32) : (STAGE_F32 > PART_F32 ? STAGE_F32 : PART_F32);
    }
};

// ---- launch with dynamic LDS: raise the kernel's limit once per instantiation (to lds_max), launch, return the error
template <auto KERNEL, typename Args>
static int launch_dyn_lds(const Args& g, int blocks, int threads, size_t lds, size_t lds_max, hipStream_t st) {
    static bool attr_done = false;
    if (!attr_done) {
        hipError_t e = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
        if (e != hipSuccess) return (int)e;
        attr_done = true;
    }
    KERNEL<<<blocks, threads, lds, st>>>(g);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
