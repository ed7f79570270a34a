// Host side of the weight-gradient family: what wgrad3x3.hip, wgrad_gemm2.hip and conv_wgrad.hip define for each other and for
// conv_x3.hip, declared once, and the problem fill the two generic kernels' argument structs share.
#pragma once
#include "common.h"

// ---- wgrad3x3.hip: 3x3 / stride 1 / pad 1, all nine taps per workgroup.  *_slices: slabs the launch writes (0: shape not handled)
int wgrad3x3_slices(int N, int H, int W, int Cin, int Cout);
int wgrad3x3_run(const void* x, const void* dy, float* slabs, int N, int H, int W, int Cin, int Cout, hipStream_t st);
// split-bf16 planes, G <= 8 same-shape problems in one grid (G = 1: the single launch); slices PER PROBLEM, slabs[p]: problem p's
// [ns][Cout][9][Cin] partials
int wgrad3x3_x3_group_slices(int G, int N, int H, int W, int Cin, int Cout);
int wgrad3x3_x3_group_run(int G, const void* const* x_hi, const void* const* x_lo, const void* const* dy_hi, const void* const* dy_lo,
                          float* const* slabs, int N, int H, int W, int Cin, int Cout, hipStream_t st);

// ---- wgrad_gemm2.hip: any tap set / stride; the stem on the zero-bordered NHWC4 image (slab rows [8][8][4])
int wgrad_gemm2_slices(int M, int Cout, int Cin, int ntaps);
int wgrad_gemm2_max_slices(int M, int Cout, int jtot);           // upper bound whatever the tap split (workspace sizing)
int wgrad_gemm2_run(const void* x, const void* dy, float* slabs, int N, int H, int W, int Cin, int Cout, int kh, int kw,
                    int stride, int pad, hipStream_t st);
int wgrad_gemm2_stem_slices(int N, int H, int W, int Cout);
int wgrad_gemm2_stem_run(const void* xpad, const void* dy, float* slabs, int N, int H, int W, int Cout, hipStream_t st);
int wgrad_gemm2_x3_slices(int M, int Cout, int Cin, int ntaps);
int wgrad_gemm2_x3_run(const void* x_hi, const void* x_lo, const void* dy_hi, const void* dy_lo, float* slabs, int N, int H, int W,
                       int Cin, int Cout, int kh, int kw, int stride, int pad, hipStream_t st);
// xpad_lo == NULL: xpad_hi is the integer image plane (AB_DT_U8N)
int wgrad_gemm2_x3_stem_run(const void* xpad_hi, const void* xpad_lo, const void* dy_hi, const void* dy_lo, float* slabs, int N,
                            int H, int W, int Cout, hipStream_t st);

// ---- conv_wgrad.hip: the fixed-order slab reduction all of them end in (recorded instead of launched inside a *_deferred call)
int wgrad_launch_reduce(const float* slabs, int ns, long slab_elems, int src_j, int dst_j, float* dst, int accumulate,
                        int stem_mask, hipStream_t st);
// A launch that runs as two half-batches (conv_x3.hip, X3_WGRAD_MAX_M) must not record its reductions: both halves write the same
// slab workspace and one descriptor holds one reduction.  It calls this first; each half then reduces at once, in stream order,
// and the *_deferred caller's descriptor keeps nslices == 0 (nothing pending).
void wgrad_reduce_now();

// run a slab kernel, then sum its ns slabs of [Cout][src_j] into dw [Cout][dst_j]
template <class Run>
static inline int wgrad_then_reduce(Run&& run, float* slabs, int ns, int Cout, int src_j, int dst_j, float* dw, int accumulate,
                                    int stem_mask, hipStream_t st) {
    if (int rc = run()) return rc;
    return wgrad_launch_reduce(slabs, ns, (long)Cout * src_j, src_j, dst_j, dw, accumulate, stem_mask, st);
}

// rows of a pixel slice when M rows go to n slices in whole steps
static inline int wgrad_rows_per_slice(int M, int n, int step) { return ((M + n - 1) / n + step - 1) / step * step; }

// ---- the problem, for Wg2Args (wgrad_gemm2.hip) and WgradArgs (conv_wgrad.hip) alike
template <class Args>
static inline void wgrad_fill_conv(Args& g, const void* x, const void* dy, float* slabs, int N, int H, int W, int Cin, int Cout, int kh,
                                   int kw, int stride, int pad) {
    g.X = x; g.DY = dy; g.slabs = slabs;
    g.N = N; g.Ha = H; g.Wa = W; g.Ca = Cin;
    g.P = (H + 2 * pad - kh) / stride + 1; g.Q = (W + 2 * pad - kw) / stride + 1; g.Cout = Cout;
    g.stride = stride; g.ntaps = kh * kw; g.Cin = Cin; g.jtot = kh * kw * Cin; g.M = N * g.P * g.Q;
    for (int i = 0; i < kh; ++i) for (int j = 0; j < kw; ++j) { g.dh[i * kw + j] = (int8_t)(i - pad); g.dw[i * kw + j] = (int8_t)(j - pad); }
}
// Stem (see ab_conv2d_stem_fwd): x is the zero-bordered NHWC4 image and a dW row is [8 kernel rows (7 + 1 pad)][8 px][4 ch]: eight
// taps of 32 columns, tap t at image row 2p + t (tap 7 is an in-bounds row of padding, dropped by the reduction's stem mask).
// wgrad_gemm2_kernel<.., STEM> covers the 256 columns with one tile and reads none of ntaps / Cin / dh / dw.
template <class Args>
static inline void wgrad_fill_stem(Args& g, const void* xpad, const void* dy, float* slabs, int N, int H, int W, int Cout) {
    g.X = xpad; g.DY = dy; g.slabs = slabs;
    g.N = N; g.Ha = H + 6; g.Wa = W + 8; g.Ca = 4;
    g.P = H / 2; g.Q = W / 2; g.Cout = Cout;
    g.stride = 2; g.ntaps = 8; g.Cin = 32; g.jtot = 256; g.M = N * g.P * g.Q;
    for (int i = 0; i < 8; ++i) { g.dh[i] = (int8_t)i; g.dw[i] = 0; }
}
