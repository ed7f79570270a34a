// Shared device helpers for the artiboost_hip kernels (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/artiboost_hip.h"

#define AB_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)

typedef uint16_t bf16_t;

__device__ __forceinline__ float bf16_to_f32(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
// round-to-nearest-even, NaN preserved (same as torch's float->bfloat16)
// round-to-nearest-even; on gfx950 the conversion is one v_cvt_pk_bf16_f32 (the bit-twiddled form is 7 VALU ops, which made
// the fused BN + ReLU + max-pool kernel VALU-bound)
__device__ __forceinline__ bf16_t f32_to_bf16(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
// two floats -> packed bf16 pair (lo in bits 0..15): one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}
template <typename T> __device__ __forceinline__ float ld_f32(const T* p);
template <> __device__ __forceinline__ float ld_f32<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ld_f32<bf16_t>(const bf16_t* p) { return bf16_to_f32(*p); }
template <typename T> __device__ __forceinline__ void st_f32(T* p, float v);
template <> __device__ __forceinline__ void st_f32<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void st_f32<bf16_t>(bf16_t* p, float v) { *p = f32_to_bf16(v); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// The fixed-order sum of a 256-thread block behind every "no atomics, two calls give the same bits" kernel: each column of acc by wave
// butterfly, lane 0 of each wave into red, waves 0..3 in turn.  Returns column tid's total to the threads tid < K (0 to the others).
// Holds a barrier: every thread of the block calls it.
template <int K>
__device__ __forceinline__ float block_sum4(float (&acc)[K], float (*red)[K]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave][k] = acc[k];
    }
    __syncthreads();
    return tid < K ? ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid] : 0.f;
}
// a sample's n workspace rows of K floats, added in row (chunk) order
template <int K>
__device__ __forceinline__ void sum_rows(const float* __restrict__ rows, int n, float (&s)[K]) {
    for (int k = 0; k < K; ++k) s[k] = 0.f;
    for (int r = 0; r < n; ++r)
        for (int k = 0; k < K; ++k) s[k] += rows[(size_t)r * K + k];
}
// point i of a packed [n][3] array
__device__ __forceinline__ void ld3(const float* p, size_t i, float v[3]) { v[0] = p[i * 3]; v[1] = p[i * 3 + 1]; v[2] = p[i * 3 + 2]; }
__device__ __forceinline__ void st3(float* p, size_t i, float a, float b, float c) { p[i * 3] = a; p[i * 3 + 1] = b; p[i * 3 + 2] = c; }
__device__ __forceinline__ void st3(float* p, size_t i, const float v[3]) { st3(p, i, v[0], v[1], v[2]); }
// plain multiplies and subtractions (the library is built with -ffp-contract=off)
__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float ab_nan() { return __builtin_nanf(""); }        // "not computed" in the evaluator's result rows
static inline hipStream_t as_stream(void* s) { return (hipStream_t)s; }
