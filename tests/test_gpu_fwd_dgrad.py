"""Every bf16x3 forward and data-gradient tile form against torch-CPU float64, one case per kernel instantiation, reached by shape alone.

conv3x3.hip (eight c3_config geometries x forward + BatchNorm partials, plain data gradient, data gradient + addend, data gradient with the
fused BatchNorm-backward epilogue), conv3x3r.hip (the persistent 64 -> 64 kernel), convp.hip (3x3 / s2), conv2x2.hip (4x4 / s2), the generic
conv_gemm2_kernel<..., X3 = 1, ALT> (four tiles, two- and three-stage ring, N-major order, four-parity-class grid, 1x1 fused BatchNorm) and
gemm_rw.hip.  No test here sets an environment switch.  A case is (N, H, W, Cin, Cout, k, stride, pad) of the FORWARD convolution; a
data-gradient mode of the same case runs dy [N, Ho, Wo, Cout] -> dx [N, H, W, Cin], i.e. the kernel sees C = Cout, Cn = Cin.

Exact class (tolerance 0).  Operands for which fp32 accumulation is exact in ANY order, so the kernel must be bit-equal to float64:
  'split': a + b * 2^-8, a in {-3, -2, 2, 3}, b in {-1, 0, 1}, q = 2^-8, for which split() is asserted to return the planes (a, b * 2^-8);
  'int':   integers from {-3..3}, q = 1 (lo planes zero) -- taken where the split class would exceed the condition below (more than ~1800
           products per output);
  every kernel here keeps hi*hi + hi*lo + lo*hi with the ACTIVATION as the first factor (read from the MFMA triples of conv3x3.hip,
  conv3x3r.hip, convp.hip, conv2x2.hip, conv_gemm2.hip, gemm_rw.hip), so the float64 reference is  op(a, w_hi) + op(a_hi, w_lo).
  Condition, asserted per case before the launch: sum |a||w| (+ |addend| + |bias|) <= 2^22 q for every output element.
  A dropped or doubled product shows as a difference of 4 q or more.
  'sparse': entries from {-1, 0, 1} at a density fixed on the CPU (_density) so that every PARTIAL SUM a launch returns stays exact as well:
  per channel sum |y| and sum y^2 over the whole launch <= 2^22 (forward / transposed-forward BatchNorm partial rows), sum |dz| <= 2^22 and
  sum |dz * xhat| <= 2^21 (fused BatchNorm-backward rows; xhat is a multiple of 1/2).  On that draw the outputs AND the row sums of the
  partial rows are bit-equal to float64.
Fused BatchNorm-backward epilogue, exact form: bnp = (scale, shift, mean, invstd) built by hand -- integer bn_y in {-3..3}, integer mean,
  invstd in {1/2, 1, 2}, scale in {-2, -1, 1, 2}, shift an odd multiple of 1/2, integer residual -- so that the pre-activation
  bn_y * scale + shift [+ residual] is an odd multiple of 1/2 (never 0: asserted) and xhat = (bn_y - mean) * invstd is exact.  All four
  epilogues (conv3x3.hip, conv3x3r.hip, convp.hip, conv_gemm2.hip) form xhat as (y - mean) * invstd and the mask as y * scale + shift > 0 or
  hi plane > 0, which are exact for such inputs: nothing had to move to the random class.
Random class.  randn operands at close(..., X3_TOL); statistics / partial rows and bn_bwd_x3(part=..., premasked=True) against its own
  reduction pass at the tolerances tests/test_gpu_conv_x3.py uses.  err / bound is printed per case.

Per case, on the same operands: the route (the row counts ab_conv2d_x3_stat_rows / ab_conv2d_dgrad_x3_stat_rows / ab_conv2d_dgrad_x3_bn_rows
/ ab_conv2d_dgrad_x3_pair_bn_rows report and the shapes of the returned stats / part tensors, against the tables below, which restate
c3_config, conv3x3r_rows, cp_rows, conv2x2_*_rows / _ok, pick_tile2x and gemm_rw_ok), and a second call bit-equal to the first.
What a row count does NOT show, and the table's form column therefore states from the predicate alone: the plain 3x3 / s1 data gradient
writes no rows (its form is that of a forward with the channel roles swapped, which the same predicate decides); an addend sends a
conv3x3r.hip shape to conv3x3_kernel geometry 4; geometries 1 / 7 / 2 and 3 / 4 share pixel tiles and differ in Cn <= 64 or the tile count;
the ring depth (nsteps <= 16 or the 128 x 128 tile: two stages), the N-major order (weights > 3 MiB, activations <= 8 MiB, more than one
channel tile), the ALT pair form and gemm_rw against the generic kernel leave the row count unchanged.

Section 1: 3x3 / s1 / p1 on conv3x3_kernel, geometries 1-8 x five modes; partial tiles in H and W, ragged last channel tile where the
           geometry admits one, Cin % 64 == 32, a stacked pair (geometry 8) whose images differ 1e4 in scale.
Section 2: conv3x3r.hip at exactly 64 tiles, one tile under (falls back to conv3x3_kernel), and 280 / 576 tiles on 256 workgroups.
Section 3: the stride-2 families: convp forward / data gradient / pair / pair + BatchNorm on both base grids, conv2x2 forward and transposed
           forward, the generic four-parity-class grid with and without ALT and with statistics.
Section 4: conv_gemm2_kernel tiles 64x64, 64x128, 128x64, 128x128, both ring depths, N-major, bias / ReLU / statistics, 1x1 fused BatchNorm,
           and gemm_rw with K in {64, 128, 192, 256}.
Section 5: outputs written into a slice of a larger buffer leave a guarded 4 KiB tail of 0xA5 unchanged, once per kernel family.

Not reachable by shape: conv_gemm2_kernel<128, 128, 4, 2, 3, false, 1, ALT> (both ALT values) -- conv_gemm2_x3_run gives the 128 x 128 tile
the two-stage ring whatever the step count, so only AB_G2X_NBUF2=0 launches the three-stage form; cp_launch<128, 64, false, 1, 2> is
AB_CP_HALF=1 only.  Neither is in the tables.

Observed on an MI355X.
  Exact class: all 160 (case, mode) pairs of sections 1-4 are bit-equal to float64 (158 on the split class, the two 2048-term N-major
  cases on the integer class); the 92 of them that return partial rows are also bit-equal, outputs and row sums, on the sparse draw; the
  fused-epilogue pairs on every (mask source, addend) combination their entry point takes.  The four logits tensors of section 4 and the
  fourteen guarded launches of section 5 are bit-equal too.  Every row count agrees with the tables.  Nothing was found, and nothing in a
  kernel or dispatcher was changed.
  Largest err / bound of the random class (bound = X3_TOL * max|ref|):
    section 1  0.184  dgrad        c3<5,FLIP=1,X3=1>    (3, 7, 7, 128, 64, 3, 1, 1)
    section 2  0.171  fwd_stats    c3r<0>               (5, 64, 112, 64, 64, 3, 1, 1)
    section 3  0.202  dgrad        cp<128,64,true,1>    (2, 16, 16, 64, 64, 3, 2, 1)
    section 4  0.254  fwd_stats    g2x<128,64,2>        (1, 257, 255, 32, 40, 1, 1, 0)
  Moved from the exact to the random class: nothing (xhat and both mask forms are exact for the hand-built BatchNorm records).
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_x3 import X3_TOL, close, nchw, nhwc
from test_gpu_wgrad import _device_operands, _seed, cdiv

pytestmark = pytest.mark.gpu

X3 = "x3"
LIM = 2.0 ** 22
C3_TILE = {1: (4, 32), 2: (8, 32), 3: (8, 16), 4: (8, 16), 5: (8, 8), 6: (16, 16), 7: (8, 32)}     # geometry -> (rows, columns) of its pixel tile


# ---------------------------------------------------------------- the pickers, restated (the library's row functions are the authority)
def c3_config(N, H, W, C, Cn, plain):
    """c3_config(N, H, W, ceil64(C), Cn, x3plain = plain, x3 = true) of conv3x3.hip with every switch at its default."""
    if C % 32 or Cn % 8:
        return 0
    if W >= 24:
        if plain and Cn <= 64 and W % 16 == 0 and H % 8 == 0:
            return 4
        if Cn <= 64 and N * cdiv(H, 8) * cdiv(W, 32) >= 512:
            return 7
        return 1 if Cn <= 64 else 2
    if W >= 12:
        if W <= 16 and H % 16 == 0 and Cn % 64 == 0:
            return 6
        return 4 if Cn <= 64 else 3
    if 5 <= W <= 8 and H <= 8 and Cn > 64:
        return 8 if (H == 8 and W == 8 and N % 2 == 0 and Cn % 64 == 0) else 5
    return 0


def c3_route(N, H, W, C, Cn, plain, addend=False):
    """(form, rows) of a 3x3 / s1 / p1 bf16x3 launch C -> Cn: 'r' conv3x3r.hip, 1-8 a conv3x3_kernel geometry, 0 the generic kernel."""
    if (C, Cn) == (64, 64) and H % 8 == 0 and W % 16 == 0 and N * (H // 8) * (W // 16) >= 64 and not (plain and addend):
        return "r", min(N * (H // 8) * (W // 16), 256)
    cfg = c3_config(N, H, W, C, Cn, plain)
    if cfg == 0:
        return 0, 0
    if cfg == 8:
        return 8, N // 2
    th, tw = C3_TILE[cfg]
    return cfg, N * cdiv(H, th) * cdiv(W, tw)


def g2x_tile(M, Cn, nsteps, nclass=0):
    """pick_tile2x + the ring depth of conv_gemm2_x3_run: (bm, bn, stages)."""
    bn = 128 if Cn > 64 else 64
    bm = 128 if cdiv(M, 128) * cdiv(Cn, bn) * max(nclass, 1) >= 512 else 64
    return bm, bn, 2 if (nsteps <= 16 or (bm, bn) == (128, 128)) else 3


def cp_rows(N, P, Q):
    if P % 16 == 0 and Q % 16 == 0:
        return N * (P // 16) * (Q // 16)
    return N // 2 if (P == 8 and Q == 8 and N % 2 == 0) else 0


def _geom(case):
    N, H, W, Cin, Cout, k, s, p = case
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def route(case, mode):
    """(form, rows) of a launch as the dispatchers of conv_x3.hip decide it.  rows: what the mode's row function reports (forward:
    ab_conv2d_x3_stat_rows; dgrad_stats: ab_conv2d_dgrad_x3_stat_rows; bn_*: ab_conv2d_dgrad_x3_bn_rows; pair_bn_*:
    ab_conv2d_dgrad_x3_pair_bn_rows), or for the modes without rows of their own (dgrad, dgrad_add, pair, pair_add) the row count of the
    predicate that decides them."""
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = _geom(case)
    ksp = (k, s, p)
    if mode.startswith("fwd"):
        plainlaunch = mode in ("fwd", "fwd_stats")
        if ksp == (3, 1, 1) and plainlaunch:
            form, rows = c3_route(N, H, W, Cin, Cout, True)
            if form:
                return ("c3r<0>" if form == "r" else f"c3<{form},FLIP=0,X3=1>"), rows
        M = N * Ho * Wo
        bm, bn, st = g2x_tile(M, Cout, k * k * (Cin // 32))
        generic = f"g2x<{bm},{bn},{st}>", cdiv(M, bm)
        if ksp == (1, 1, 0) and mode in ("fwd", "fwd_bias") and M % 64 == 0 and Cout % 32 == 0 and 32 <= Cout <= 8192 and Cin in (64, 128, 192, 256):
            return f"gemm_rw<{Cin // 64}>", generic[1]
        if ksp == (4, 2, 1) and plainlaunch and Cin % 32 == 0 and Cout % 64 == 0:
            if (H, W) == (32, 32):
                return "c22<256,64,4,false>", N
            if (H, W) == (16, 16) and N % 2 == 0:
                return "c22<128,64,4,true>", N // 2
        if ksp == (3, 2, 1) and plainlaunch and Cin >= 128 and Cin % 32 == 0 and Cout % 64 == 0 and H % 2 == 0 and W % 2 == 0:
            r = cp_rows(N, H // 2, W // 2)
            if r:
                return ("cp<128,64,true,0>" if H // 2 == 8 else "cp<256,64,false,0>"), r
        return generic
    # ---- data-gradient modes: the kernel sees C = Cout, Cn = Cin
    bn_mode, pair = mode.startswith("bn_") or mode.startswith("pair_bn_"), mode.startswith("pair")
    addend = mode.endswith("_add")
    if ksp == (3, 1, 1):
        if bn_mode:
            form, rows = c3_route(N, H, W, Cout, Cin, False)
            assert form, "the fused epilogue needs a conv3x3 shape"
            if form == "r":
                return "c3r<1,1,addend,mask>", rows
            return f"c3<{form},FLIP=1,X3=2>", rows
        form, rows = c3_route(N, H, W, Cout, Cin, True, addend)
        if form:
            return ("c3r<1>" if form == "r" else f"c3<{form},FLIP=1,X3=1>"), rows
    if s == 1:
        M = N * H * W
        bm, bn, st = g2x_tile(M, Cin, k * k * (Cout // 32))
        if bn_mode:
            assert ksp == (1, 1, 0) and Cin % 64 == 0 and (Cin <= 64 or Cin % 128 == 0)
            return f"g2x<{bm},{bn},{st}>+bn", cdiv(M, bm)
        return f"g2x<{bm},{bn},{st}>", cdiv(M, bm)
    assert s == 2 and H % 2 == 0 and W % 2 == 0
    if ksp == (4, 2, 1) and not addend and not pair and Cout % 32 == 0:
        if (H, W) == (32, 32) and Cin % 64 == 0:
            return f"c22<256,{128 if Cin % 128 == 0 else 64},1,false>", N * 4
        if (H, W) == (16, 16) and N % 4 == 0 and Cin % 64 == 0:
            return "c22<256,64,1,true>", N
    cp = cp_rows(N, H // 2, W // 2) if (ksp == (3, 2, 1) and Cout % 32 == 0 and Cout >= 64 and Cin % 64 == 0) else 0
    if mode.startswith("pair_bn_"):
        assert cp, "the paired fused epilogue exists on convp.hip only"
        return ("cp<128,64,true,1>+bn" if H // 2 == 8 else "cp<256,64,false,1>+bn"), 4 * cp
    if cp and mode in ("dgrad", "pair"):
        return ("cp<128,64,true,1>" if H // 2 == 8 else "cp<256,64,false,1>"), 4 * cp
    maxt = max(sum(1 for i in range(k) for j in range(k) if (a + p - i) % 2 == 0 and (b + p - j) % 2 == 0) for a in (0, 1) for b in (0, 1))
    M = N * (H // 2) * (W // 2)
    bm, bn, st = g2x_tile(M, Cin, maxt * (Cout // 32), 4)
    return f"g2x<{bm},{bn},{st},nclass=4{',ALT' if pair else ''}>", 4 * cdiv(M, bm)


def library_rows(cd, case, mode):
    """The library's own host-side row function for the mode (cd: the ctypes library; runs without a GPU)."""
    N, H, W, Cin, Cout, k, s, p = case
    if mode.startswith("fwd"):
        return cd.ab_conv2d_x3_stat_rows(N, H, W, Cin, Cout, k, k, s, p)
    if mode.startswith("pair_bn_"):
        return cd.ab_conv2d_dgrad_x3_pair_bn_rows(N, H, W, Cin, Cout, k, k, p)
    if mode.startswith("bn_"):
        return cd.ab_conv2d_dgrad_x3_bn_rows(N, H, W, Cin, Cout, k, k, s, p)
    if s == 1 and (k, p) == (3, 1):          # no rows of its own: the forward predicate with the channel roles swapped decides the same c3_config
        r = cd.ab_conv2d_x3_stat_rows(N, H, W, Cout, Cin, 3, 3, 1, 1)
        if mode == "dgrad_add" and route(case, "dgrad")[0] == "c3r<1>":       # the addend keeps the launch off conv3x3r.hip: geometry 4's tiles
            return N * cdiv(H, 8) * cdiv(W, 16)
        return r
    if s == 1:
        # 1x1: conv_gemm2_x3_mtiles of the swapped forward; other stride-1 kernels (3x3 / p0): the library has no row function that sees them
        return cd.ab_conv2d_x3_stat_rows(N, H, W, Cout, Cin, k, k, 1, p) if k == 1 else route(case, mode)[1]
    r = cd.ab_conv2d_dgrad_x3_pair_bn_rows(N, H, W, Cin, Cout, k, k, p) if mode in ("dgrad", "pair") and (k, p) == (3, 1) else 0
    return r if r else cd.ab_conv2d_dgrad_x3_stat_rows(N, H, W, Cin, Cout, k, k, s, p)


# ---------------------------------------------------------------- case tables.  Every form and row count below is LITERAL; route() and the
# library's row functions are asserted against them per case (here before the launch, and in tests/test_fwd_dgrad_host.py without a GPU)
C3_MODES = ("fwd_stats", "dgrad", "dgrad_add", "bn_recompute", "bn_hi")


def _c3(shape, plain, bnr, note, modes=C3_MODES, seam=False):
    """shape (N, H, W, C, Cn) in the KERNEL's view; plain / bnr: (form, rows) of the plain and of the fused-epilogue launch."""
    return types.SimpleNamespace(shape=shape, plain=plain, bnr=bnr, note=note, modes=modes, seam=seam)


S1 = [
    _c3((2, 12, 20, 64, 40), (4, 8), (4, 8), "geometry 4: partial tiles in H and W, ragged 40-channel tile"),
    _c3((1, 8, 32, 64, 64), (4, 2), (1, 2), "W >= 24 shortcut to geometry 4; the fused epilogue lands on geometry 1 (4 x 32 tiles, same count)"),
    _c3((1, 10, 24, 96, 64), (1, 3), (1, 3), "geometry 1: C % 64 == 32 (an odd number of 32-channel chunks), partial tiles both ways"),
    _c3((2, 6, 40, 64, 24), (1, 8), (1, 8), "geometry 1: ragged 24-channel tile, two tiles in W"),
    _c3((1, 9, 28, 64, 136), (2, 2), (2, 2), "geometry 2: second channel tile holds 8 channels, partial H and W"),
    _c3((1, 14, 14, 64, 72), (3, 2), (3, 2), "geometry 3: ragged channel tile, partial H and W"),
    _c3((1, 8, 20, 64, 128), (3, 2), (3, 2), "geometry 3: two tiles in W, the second partial"),
    _c3((1, 16, 16, 64, 128), (6, 1), (6, 1), "geometry 6: whole-image tile, two channel tiles"),
    _c3((2, 32, 12, 64, 64), (6, 4), (6, 4), "geometry 6: W < tile width, two tiles per image in H"),
    _c3((3, 7, 7, 64, 128), (5, 3), (5, 3), "geometry 5: odd N at <= 8 x 8 must not stack; partial H and W"),
    _c3((1, 8, 8, 64, 72), (5, 1), (5, 1), "geometry 5: ragged channel tile"),
    _c3((2, 8, 8, 64, 128), (8, 1), (8, 1), "geometry 8: a stacked pair, image 0 at 1e4 scale in the random class", seam=True),
    _c3((4, 8, 8, 128, 192), (8, 2), (8, 2), "geometry 8: two pairs, three channel tiles, two 64-channel K chunks"),
    _c3((128, 9, 33, 64, 40), (7, 512), (7, 512), "geometry 7 (>= 512 tiles of 8 x 32): partial H and W, ragged channel tile"),
    _c3((37, 56, 56, 64, 64), (7, 518), (7, 518), "geometry 7 at layer 1's evaluation size", modes=("fwd_stats", "bn_recompute")),
    _c3((1, 56, 144, 64, 64), (4, 63), (1, 70), "63 tiles of 8 x 16: one under conv3x3r.hip's limit, falls back to conv3x3_kernel"),
]
S2 = [
    _c3((1, 64, 128, 64, 64), ("r", 64), ("r", 64), "conv3x3r.hip at exactly 64 tiles (one per workgroup)"),
    _c3((5, 64, 112, 64, 64), ("r", 256), ("r", 256), "280 tiles on 256 persistent workgroups: 24 loop twice, 232 once"),
    _c3((9, 64, 128, 64, 64), ("r", 256), ("r", 256), "576 tiles: 64 workgroups loop three times, 192 twice", modes=("fwd_stats", "dgrad", "bn_hi")),
]


def _c3_case(c, mode):
    """The forward-view case of a kernel-view shape: data-gradient modes swap the channel roles."""
    N, H, W, C, Cn = c.shape
    return (N, H, W, C, Cn, 3, 1, 1) if mode.startswith("fwd") else (N, H, W, Cn, C, 3, 1, 1)


def _c3_expect(c, mode):
    if mode.startswith("bn_"):
        form, rows = c.bnr
        return ("c3r<1,1,addend,mask>" if form == "r" else f"c3<{form},FLIP=1,X3=2>"), rows
    form, rows = c.plain
    if form == "r" and mode == "dgrad_add":
        N, H, W, C, Cn = c.shape
        return "c3<4,FLIP=1,X3=1>", N * cdiv(H, 8) * cdiv(W, 16)
    fl = 0 if mode.startswith("fwd") else 1
    return (f"c3r<{fl}>" if form == "r" else f"c3<{form},FLIP={fl},X3=1>"), rows


# (case, mode, form, rows, note)
S3 = [
    # convp forward (3x3 / s2 / p1, Cin >= 128, Cout % 64 == 0)
    ((1, 32, 32, 128, 64, 3, 2, 1), "fwd_stats", "cp<256,64,false,0>", 1, "16 x 16 base grid, one tile"),
    ((2, 32, 64, 128, 128, 3, 2, 1), "fwd_stats", "cp<256,64,false,0>", 4, "several tiles, two channel tiles"),
    ((2, 16, 16, 128, 64, 3, 2, 1), "fwd_stats", "cp<128,64,true,0>", 1, "paired 8 x 8 form"),
    ((1, 32, 32, 160, 64, 3, 2, 1), "fwd_stats", "cp<256,64,false,0>", 1, "an odd number of 32-channel chunks"),
    ((3, 16, 16, 128, 64, 3, 2, 1), "fwd_stats", "g2x<64,64,3>", 3, "odd N at 8 x 8: the generic kernel"),
    ((2, 32, 32, 64, 64, 3, 2, 1), "fwd_stats", "g2x<64,64,3>", 8, "Cin = 64: convp declines"),
    # convp data gradient: plain, paired with the 1x1 / s2 branch, paired with the BatchNorm epilogue; both base forms
    ((1, 32, 32, 64, 64, 3, 2, 1), "dgrad", "cp<256,64,false,1>", 4, ""),
    ((1, 32, 32, 64, 64, 3, 2, 1), "pair", "cp<256,64,false,1>", 4, ""),
    ((1, 32, 32, 64, 64, 3, 2, 1), "pair_bn_recompute", "cp<256,64,false,1>+bn", 4, ""),
    ((1, 32, 32, 64, 64, 3, 2, 1), "pair_bn_hi", "cp<256,64,false,1>+bn", 4, ""),
    ((2, 32, 64, 128, 96, 3, 2, 1), "dgrad", "cp<256,64,false,1>", 16, "two channel tiles, K = 96 (three chunks)"),
    ((2, 32, 64, 128, 96, 3, 2, 1), "pair", "cp<256,64,false,1>", 16, ""),
    ((2, 32, 64, 128, 96, 3, 2, 1), "pair_bn_recompute", "cp<256,64,false,1>+bn", 16, ""),
    ((2, 32, 64, 128, 96, 3, 2, 1), "pair_bn_hi", "cp<256,64,false,1>+bn", 16, ""),
    ((2, 16, 16, 64, 64, 3, 2, 1), "dgrad", "cp<128,64,true,1>", 4, "paired 8 x 8 form"),
    ((2, 16, 16, 64, 64, 3, 2, 1), "pair", "cp<128,64,true,1>", 4, ""),
    ((2, 16, 16, 64, 64, 3, 2, 1), "pair_bn_recompute", "cp<128,64,true,1>+bn", 4, ""),
    ((2, 16, 16, 64, 64, 3, 2, 1), "pair_bn_hi", "cp<128,64,true,1>+bn", 4, ""),
    # conv2x2 forward (4x4 / s2 / p1) and transposed forward (its data gradient form)
    ((1, 32, 32, 32, 64, 4, 2, 1), "fwd_stats", "c22<256,64,4,false>", 1, "32 x 32"),
    ((2, 16, 16, 64, 64, 4, 2, 1), "fwd_stats", "c22<128,64,4,true>", 1, "two 16 x 16 images per tile"),
    ((1, 32, 32, 96, 128, 4, 2, 1), "fwd_stats", "c22<256,64,4,false>", 1, "three K chunks, two channel tiles"),
    ((3, 16, 16, 64, 64, 4, 2, 1), "fwd_stats", "g2x<64,64,3>", 3, "odd N misses the grouping"),
    ((1, 32, 32, 128, 32, 4, 2, 1), "dgrad_stats", "c22<256,128,1,false>", 4, "Cn % 128 == 0"),
    ((1, 32, 32, 64, 64, 4, 2, 1), "dgrad_stats", "c22<256,64,1,false>", 4, "Cn % 64 == 0 only"),
    ((4, 16, 16, 64, 32, 4, 2, 1), "dgrad_stats", "c22<256,64,1,true>", 4, "four 16 x 16 images per tile"),
    ((2, 32, 32, 192, 96, 4, 2, 1), "dgrad_stats", "c22<256,64,1,false>", 8, "192 = 3 x 64 channels, three K chunks"),
    ((3, 16, 16, 64, 64, 4, 2, 1), "dgrad_stats", "g2x<64,64,2,nclass=4>", 12, "N % 4 != 0 misses the grouping"),
    # the generic four-parity-class grid
    ((2, 14, 14, 64, 32, 4, 2, 1), "dgrad_stats", "g2x<64,64,2,nclass=4>", 8, "4x4 / s2 at a size conv2x2 declines"),
    ((3, 14, 10, 64, 128, 3, 2, 1), "dgrad_stats", "g2x<64,64,2,nclass=4>", 8, "3x3 / s2 on a 7 x 5 base map"),
    ((3, 14, 10, 64, 128, 3, 2, 1), "dgrad", "g2x<64,64,2,nclass=4>", 8, ""),
    ((3, 14, 10, 64, 128, 3, 2, 1), "pair", "g2x<64,64,2,nclass=4,ALT>", 8, "ALT, two-stage ring"),
    ((3, 14, 10, 64, 160, 3, 2, 1), "pair_add", "g2x<64,64,3,nclass=4,ALT>", 8, "ALT, three-stage ring (20 steps), addend"),
    ((3, 14, 10, 128, 64, 3, 2, 1), "pair", "g2x<64,128,2,nclass=4,ALT>", 8, "ALT on the 128-channel tile"),
    ((3, 14, 10, 128, 160, 3, 2, 1), "pair", "g2x<64,128,3,nclass=4,ALT>", 8, "... on the three-stage ring"),
    ((3, 14, 10, 128, 160, 3, 2, 1), "dgrad_stats", "g2x<64,128,3,nclass=4>", 8, ""),
    # 128-row tiles of the four-class grid: 4 x ceil(M / 128) >= 512 needs M = 16 384 base pixels (an addend keeps convp.hip out)
    ((4, 128, 128, 64, 64, 3, 2, 1), "dgrad_add", "g2x<128,64,2,nclass=4>", 512, ""),
    ((4, 128, 128, 64, 64, 3, 2, 1), "pair_add", "g2x<128,64,2,nclass=4,ALT>", 512, ""),
    ((4, 128, 128, 64, 160, 3, 2, 1), "pair_add", "g2x<128,64,3,nclass=4,ALT>", 512, ""),
    ((4, 128, 128, 128, 64, 3, 2, 1), "pair_add", "g2x<128,128,2,nclass=4,ALT>", 512, ""),
    ((4, 128, 128, 128, 64, 3, 2, 1), "dgrad_add", "g2x<128,128,2,nclass=4>", 512, ""),
    ((2, 32, 32, 64, 64, 3, 2, 1), "pair_add", "g2x<64,64,2,nclass=4,ALT>", 32, "an addend keeps a convp shape on the generic kernel"),
    ((3, 16, 16, 64, 64, 3, 2, 1), "dgrad", "g2x<64,64,2,nclass=4>", 12, "odd N at 8 x 8: convp declines"),
    ((2, 14, 14, 64, 128, 1, 2, 0), "dgrad_stats", "g2x<64,64,2,nclass=4>", 8, "1x1 / s2: three of the four classes have no tap"),
    ((2, 14, 14, 64, 128, 1, 2, 0), "dgrad_add", "g2x<64,64,2,nclass=4>", 8, ""),
]
S4 = [
    # conv_gemm2_kernel tiles; M and Cn ragged against every tile
    ((2, 9, 5, 64, 40, 1, 1, 0), "fwd_stats", "g2x<64,64,2>", 2, "64 x 64, M = 90, Cn = 40"),
    ((2, 9, 5, 64, 40, 1, 1, 0), "fwd_bias", "g2x<64,64,2>", 2, ""),
    ((2, 9, 5, 64, 40, 1, 1, 0), "fwd_relu", "g2x<64,64,2>", 2, ""),
    ((2, 9, 5, 64, 40, 1, 1, 0), "fwd_bias_relu", "g2x<64,64,2>", 2, ""),
    ((2, 9, 5, 64, 40, 1, 1, 0), "fwd_bias_stats", "g2x<64,64,2>", 2, ""),
    ((2, 9, 5, 256, 616, 1, 1, 0), "fwd_stats", "g2x<64,128,2>", 2, "64 x 128, Cn = 616 = 4 x 128 + 104"),
    ((2, 9, 5, 256, 616, 1, 1, 0), "fwd_bias_relu", "g2x<64,128,2>", 2, "the final layer's form"),
    ((2, 9, 5, 616, 256, 1, 1, 0), "dgrad", "g2x<64,128,2>", 2, "a 1x1 data gradient onto 616 = 4 x 128 + 104 channels"),
    ((1, 257, 255, 32, 40, 1, 1, 0), "fwd_stats", "g2x<128,64,2>", 512, "128 x 64: M = 65 535 = 511 x 128 + 127"),
    ((2, 65, 63, 32, 1000, 1, 1, 0), "fwd_stats", "g2x<128,128,2>", 64, "128 x 128: M = 8190, Cn = 1000 = 7 x 128 + 104"),
    ((1, 9, 7, 64, 40, 3, 1, 0), "fwd_stats", "g2x<64,64,3>", 1, "3x3 / s1 / p0: 18 steps, three-stage ring"),
    ((2, 9, 5, 576, 136, 1, 1, 0), "fwd_stats", "g2x<64,128,3>", 2, "1x1 with Cin = 576: 18 steps"),
    ((1, 259, 257, 64, 8, 3, 1, 0), "fwd_stats", "g2x<128,64,3>", 512, "128 x 64 on the three-stage ring"),
    ((2, 9, 5, 2048, 400, 1, 1, 0), "fwd_stats", "g2x<64,128,3>", 2, "N-major order: 3.1 MiB of weights, two M tiles x four channel tiles"),
    ((2, 9, 5, 400, 2048, 1, 1, 0), "dgrad_add", "g2x<64,128,3>", 2, "N-major data gradient + addend"),
    ((1, 7, 9, 64, 96, 3, 1, 0), "dgrad", "g2x<64,64,3>", 1, "3x3 / s1 / p0 data gradient (27 steps)"),
    # the 1x1 fused-BatchNorm data gradient on 64- and 128-channel tiles
    ((3, 16, 16, 64, 96, 1, 1, 0), "bn_recompute", "g2x<64,64,2>+bn", 12, ""),
    ((2, 9, 5, 128, 64, 1, 1, 0), "bn_recompute", "g2x<64,128,2>+bn", 2, "ragged M"),
    ((2, 9, 5, 256, 704, 1, 1, 0), "bn_recompute", "g2x<64,128,3>+bn", 2, "two channel tiles, 22 steps"),
    # gemm_rw (1x1 / s1 / p0, no statistics, no ReLU): K in {64, 128, 192, 256}
    ((1, 8, 8, 64, 32, 1, 1, 0), "fwd", "gemm_rw<1>", 1, "M = 64, N = 32"),
    ((3, 80, 80, 64, 32, 1, 1, 0), "fwd_bias", "gemm_rw<1>", 300, "300 tiles on one group of <= 256 workgroups"),
    ((6, 40, 40, 128, 288, 1, 1, 0), "fwd", "gemm_rw<2>", 150, "N = 288: a second group of one wave; 150 tiles on 128 workgroups per group"),
    ((1, 8, 16, 192, 96, 1, 1, 0), "fwd_bias", "gemm_rw<3>", 2, ""),
    ((2, 8, 8, 256, 704, 1, 1, 0), "fwd_bias", "gemm_rw<4>", 2, "three groups (8 + 8 + 6 waves)"),
    ((1, 9, 7, 64, 32, 1, 1, 0), "fwd_bias", "g2x<64,64,2>", 1, "M % 64 != 0: gemm_rw declines"),
    ((1, 8, 8, 320, 32, 1, 1, 0), "fwd_bias", "g2x<64,64,2>", 1, "K = 320: gemm_rw declines"),
]
SAM = [((1, 8, 8, 64, 32, 1, 1, 0), 1, 32), ((6, 40, 40, 128, 288, 1, 1, 0), 9, 17), ((1, 8, 16, 192, 96, 1, 1, 0), 3, 32),
       ((2, 8, 8, 256, 704, 1, 1, 0), 22, 28)]                                                  # (case, C classes, D depth bins): gemm_rw<K / 64, SAM>


def all_cases():
    """Every (section, case, mode, form, rows, seam) of this file."""
    out = []
    for sec, tab in ((1, S1), (2, S2)):
        for c in tab:
            for mode in c.modes:
                form, rows = _c3_expect(c, mode)
                out.append((sec, _c3_case(c, mode), mode, form, rows, c.seam))
    for sec, tab in ((3, S3), (4, S4)):
        for case, mode, form, rows, _ in tab:
            out.append((sec, case, mode, form, rows, False))
    return out


def _params(section):
    return [pytest.param(case, mode, form, rows, seam, id=f"{mode}-{form}-" + "x".join(map(str, case)))
            for sec, case, mode, form, rows, seam in all_cases() if sec == section]


# ---------------------------------------------------------------- operands and float64 references (computed once, shared, never written to)
def _is_fwd(mode):
    return mode.startswith("fwd")


def _terms(case, mode):
    """Products per output element (an upper bound): what decides the operand class."""
    N, H, W, Cin, Cout, k, s, p = case
    if _is_fwd(mode):
        return k * k * Cin
    t = (cdiv(k, s) ** 2) * Cout
    return t + Cout if mode.startswith("pair") else t


def exact_class(case, mode):
    """'split' where (3 + 2^-8)^2 * terms * 2^8 stays under 2^22, else 'int'."""
    return "split" if (3 + 2.0 ** -8) ** 2 * _terms(case, mode) * 256 + 4 * 256 <= LIM else "int"


def _density(case, mode):
    """Densities (operands, addend) of the sparse draw, fixed here on the CPU: with entries of +-1 at density d the expected per-channel
    total of |products| -- and of y^2 -- over the launch is outputs * terms * d^2.  2^20 for the BatchNorm partial rows of a forward leaves
    a factor 4 to the bound; the fused epilogue multiplies by |xhat| <= 8 (q = 1/2), so its budget is 2^17 for products and addend each."""
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = _geom(case)
    outs = N * Ho * Wo if _is_fwd(mode) else N * H * W
    budget = 2.0 ** 17 if "bn_" in mode else 2.0 ** 20
    return min(1.0, (budget / (outs * _terms(case, mode))) ** 0.5), min(1.0, 2.0 ** 17 / outs)


def _draw(g, shape, cls, density=1.0):
    o = types.SimpleNamespace()
    if cls == "random":
        o.full = torch.randn(shape, generator=g)
        o.hi = o.lo = None
        return o
    if cls == "split":
        o.hi = torch.tensor([-3.0, -2.0, 2.0, 3.0])[torch.randint(0, 4, shape, generator=g)]
        o.lo = torch.randint(-1, 2, shape, generator=g).float() * 2.0 ** -8
    elif cls == "int":
        o.hi, o.lo = torch.randint(-3, 4, shape, generator=g).float(), torch.zeros(shape)
    else:
        o.hi = (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * (torch.rand(shape, generator=g) < density).float()
        o.lo = torch.zeros(shape)
    o.full = o.hi + o.lo                                          # exact in fp32: 10 significant bits
    return o


def _op(case, fwd, a, w_ohwi, k=None, p=None):
    """float64: the forward convolution of a [N,H,W,Cin], or the data gradient of a = dy [N,Ho,Wo,Cout]; weights [Cout][k][k][Cin]."""
    N, H, W, Cin, Cout, k0, s, p0 = case
    k, p = (k0 if k is None else k), (p0 if p is None else p)
    w = w_ohwi.double().permute(0, 3, 1, 2).contiguous()
    if fwd:
        return nhwc(F.conv2d(nchw(a).double(), w, stride=s, padding=p))
    return nhwc(torch.nn.grad.conv2d_input((N, Cin, H, W), w, nchw(a).double(), stride=s, padding=p))


def _kept(case, fwd, a, w, k=None, p=None):
    """(result, mass) of the plane products the kernels keep: a * w_hi + a_hi * w_lo, and the same of the absolute values."""
    ref = _op(case, fwd, a.full, w.hi, k, p)
    mass = _op(case, fwd, a.hi.abs() + a.lo.abs(), w.hi.abs(), k, p)
    if bool(w.lo.any()):
        ref, mass = ref + _op(case, fwd, a.hi, w.lo, k, p), mass + _op(case, fwd, a.hi.abs(), w.lo.abs(), k, p)
    return ref, mass


@functools.lru_cache(maxsize=None)
def problem(case, mode, cls, seam=False):
    """Operands (CPU), float64 results and masses of one (case, mode) in one operand class."""
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = _geom(case)
    fwd = _is_fwd(mode)
    g = torch.Generator().manual_seed(_seed(case, {"split": 11, "int": 12, "sparse": 13, "random": 14}[cls] + 100 * sum(map(ord, mode))))
    o = types.SimpleNamespace(cls=cls, q={"split": 2.0 ** -8}.get(cls, 1.0), fwd=fwd, exact=cls != "random")
    d, d_add = _density(case, mode) if cls == "sparse" else (1.0, 1.0)
    o.density = (d, d_add)
    a_shape = (N, H, W, Cin) if fwd else (N, Ho, Wo, Cout)
    out_ch = Cout if fwd else Cin
    o.a, o.w = _draw(g, a_shape, cls, d), _draw(g, (Cout, k, k, Cin), cls, d)
    if cls == "random":
        o.w.full = o.w.full * (2.0 / (k * k * (Cin if fwd else Cout))) ** 0.5
        if seam:
            o.a.full[0] *= 1e4
        o.ref, o.mass = _op(case, fwd, o.a.full, o.w.full), None
    else:
        o.ref, o.mass = _kept(case, fwd, o.a, o.w)
    o.a2 = o.w2 = o.addend = o.bias = None
    if mode.startswith("pair"):
        o.a2, o.w2 = _draw(g, a_shape, cls, d), _draw(g, (Cout, 1, 1, Cin), cls, d)
        if cls == "random":
            o.w2.full = o.w2.full * (2.0 / Cout) ** 0.5
            o.ref = o.ref + _op(case, False, o.a2.full, o.w2.full, 1, 0)
        else:
            r2, m2 = _kept(case, False, o.a2, o.w2, 1, 0)
            o.ref, o.mass = o.ref + r2, o.mass + m2
    if "bias" in mode:
        o.bias = torch.randn(out_ch, generator=g) if cls == "random" else torch.randint(-3, 4, (out_ch,), generator=g).float()
        o.ref = o.ref + o.bias.double()
        o.mass = None if o.mass is None else o.mass + o.bias.abs().double()
    if "relu" in mode:
        o.ref = o.ref.clamp_min(0)
    wants_add = mode.endswith("_add") or "bn_" in mode        # the fused epilogue runs with AND without the addend: o.ref stays without
    if wants_add:
        o.addend = _draw(g, o.ref.shape, "int" if cls == "split" else cls, d_add).full
        o.ref_add = o.ref + o.addend.double()
        o.mass_add = None if o.mass is None else o.mass + o.addend.abs().double()
    if "bn_" in mode and o.exact:
        C = out_ch
        pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (C,), generator=g)]
        o.bn_y = torch.randint(-3, 4, o.ref.shape, generator=g).float()
        o.bnp = torch.stack([pick([-2.0, -1.0, 1.0, 2.0]), pick([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5]), pick([-1.0, 0.0, 1.0]), pick([0.5, 1.0, 2.0])])
        o.res = torch.randint(-3, 4, o.ref.shape, generator=g).float() if mode.endswith("_hi") else None
        o.pre = o.bn_y.double() * o.bnp[0].double() + o.bnp[1].double() + (o.res.double() if o.res is not None else 0.0)
        o.act = o.pre.clamp_min(0).float()                                     # relu(bn(bn_y) [+ residual]): at most 5 significant bits
        o.mask = (o.pre > 0).double()
        o.xhat = (o.bn_y.double() - o.bnp[2].double()) * o.bnp[3].double()
    return o


def bn_results(o, with_add):
    """float64 (dz, sum dz, sum dz * xhat, mass of sum dz, mass of sum dz * xhat) of the exact fused epilogue."""
    raw, mass = (o.ref_add, o.mass_add) if with_add else (o.ref, o.mass)
    dz = raw * o.mask
    return dz, dz.sum((0, 1, 2)), (dz * o.xhat).sum((0, 1, 2)), (mass * o.mask).sum((0, 1, 2)), (mass * o.mask * o.xhat.abs()).sum((0, 1, 2))


def assert_conditions(o, mode):
    """The exactness conditions of a problem, in float64 on the CPU (called before every launch, and for every case by the host test)."""
    assert o.exact
    lim = LIM * o.q
    for m in (o.mass, getattr(o, "mass_add", None)):
        if m is not None:
            assert float(m.max()) <= lim, f"exactness condition: sum |a||w| = {float(m.max()):g} > 2^22 q = {lim:g}"
    if "bn_" in mode:
        assert float(o.pre.abs().min()) >= 0.5, "a masked pre-activation sits at the threshold"
        assert bool((o.act.bfloat16().float() == o.act).all()), "the stored activation is not exact in its hi plane"
        if o.cls == "sparse":
            for with_add in (False, True):
                _, _, _, m0, m1 = bn_results(o, with_add)
                assert float(m0.max()) <= LIM and float(m1.max()) <= LIM / 2, f"partial-row condition: {float(m0.max()):g}, {float(m1.max()):g}"
    if "stats" in mode and o.cls == "sparse":
        assert float(o.mass.sum((0, 1, 2)).max()) <= LIM, "partial-row condition: sum |y|"
        assert float((o.ref * o.ref).sum((0, 1, 2)).max()) <= LIM, "partial-row condition: sum y^2"
        assert float(o.mass.max()) <= 2.0 ** 12, "y^2 of one element must stay an exact integer"


def assert_exact(what, got, ref, q):
    """Bit-equality with the float64 result; on failure say how many entries differ, by how many quanta, and where."""
    got = got.double().cpu()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    if torch.equal(got, ref):
        return
    d = (got - ref) / q
    bad = d.nonzero()
    first = ", ".join(f"{tuple(int(v) for v in ix)}: {float(d[tuple(ix)]):+g} q" for ix in bad[:6])
    whole = bool((d == d.round()).all())
    raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} entries differ, largest {float(d.abs().max()):g} q"
                         f"{'' if whole else ' (NOT all multiples of q: the exactness premise fails)'}; first: {first}")


# ---------------------------------------------------------------- device side
def _dev(o, case):
    """Device operands of a problem: activation planes, weight planes in the launch's layout (OHWI forward, IHWO data gradient)."""
    d = types.SimpleNamespace()
    lay = (lambda w: w) if o.fwd else (lambda w: w.permute(3, 1, 2, 0).contiguous())
    if o.exact:
        d.a, d.w = _device_operands(X3, o.a.full, lay(o.w.full), (o.a.hi, o.a.lo, lay(o.w.hi), lay(o.w.lo)))
        d.a2, d.w2 = _device_operands(X3, o.a2.full, lay(o.w2.full), (o.a2.hi, o.a2.lo, lay(o.w2.hi), lay(o.w2.lo))) if o.a2 is not None else (None, None)
    else:
        d.a, d.w = _device_operands(X3, o.a.full, lay(o.w.full))
        d.a2, d.w2 = _device_operands(X3, o.a2.full, lay(o.w2.full)) if o.a2 is not None else (None, None)
    d.addend = o.addend.cuda() if o.addend is not None else None
    d.bias = o.bias.cuda() if o.bias is not None else None
    return d


def _launch(case, mode, d, with_add=None, bn=None):
    """One launch through the wrappers of artiboost_amd.kernels -> (output, rows tensor or None)."""
    from artiboost_amd import kernels as K
    N, H, W, Cin, Cout, k, s, p = case
    if _is_fwd(mode):
        r = K.conv2d_fwd_x3(d.a, d.w, s, p, bias=d.bias, want_stats="stats" in mode, relu="relu" in mode)
        return r if "stats" in mode else (r, None)
    addend = d.addend if (mode.endswith("_add") if with_add is None else with_add) else None
    if mode.startswith("pair"):
        r = K.conv2d_dgrad_x3_pair(d.a, d.w, d.a2, d.w2, (H, W), p, addend=addend, bn=bn)
        return r if bn is not None else (r, None)
    if bn is not None:
        return K.conv2d_dgrad_x3(d.a, d.w, (H, W), s, p, addend=addend, bn=bn)
    if "stats" in mode:
        return K.conv2d_dgrad_x3(d.a, d.w, (H, W), s, p, want_stats=True)
    return K.conv2d_dgrad_x3(d.a, d.w, (H, W), s, p, addend=addend), None


def _twice(case, mode, d, **kw):
    out, rows = _launch(case, mode, d, **kw)
    out2, rows2 = _launch(case, mode, d, **kw)
    assert torch.equal(out, out2), "a second call differs"
    assert (rows is None) == (rows2 is None) and (rows is None or torch.equal(rows, rows2)), "a second call's partial rows differ"
    return out, rows


def _ratio(what, got, ref, per_image=False):
    """err / bound at close(..., X3_TOL), printed; asserted by close()."""
    got, worst = got.double().cpu(), 0.0
    for sl in ([slice(i, i + 1) for i in range(ref.shape[0])] if per_image else [slice(None)]):
        r = float((got[sl] - ref[sl]).abs().max()) / (X3_TOL * (float(ref[sl].abs().max()) + 1e-30))
        worst = max(worst, r)
        close(got[sl], ref[sl])
    print(f"fwd_dgrad {what}: random class err / bound {worst:.3e}")
    return worst


def _stat_check(what, rows, out64):
    """BatchNorm partial rows of the random class at the tolerances of tests/test_gpu_conv_x3.py."""
    import numpy as np
    st = rows.double().sum(0).cpu()
    yy = out64.reshape(-1, out64.shape[-1])
    np.testing.assert_allclose(st[:, 0].numpy(), yy.sum(0).numpy(), rtol=1e-4, atol=1e-4 * float(yy.abs().sum(0).max()), err_msg=what)
    np.testing.assert_allclose(st[:, 1].numpy(), (yy * yy).sum(0).numpy(), rtol=1e-4, err_msg=what)


def _check_plain(case, mode, form, rows, seam, what):
    """forward / data gradient / pair, with or without addend, bias, ReLU, statistics."""
    out_ch = case[4] if _is_fwd(mode) else case[3]
    for cls in [exact_class(case, mode)] + (["sparse"] if "stats" in mode else []) + ["random"]:
        o = problem(case, mode, cls, seam)
        if o.exact:
            assert_conditions(o, mode)
        d = _dev(o, case)
        out, part = _twice(case, mode, d)
        ref = o.ref_add if mode.endswith("_add") else o.ref
        if "stats" in mode:
            assert part is not None and tuple(part.shape) == (rows, out_ch, 2), f"{what}: partial rows {tuple(part.shape)}, the table has {rows}"
        if o.exact:
            print(f"fwd_dgrad {what}: class '{cls}' mass {float((o.mass_add if mode.endswith('_add') else o.mass).max()) / o.q:.0f} q of {2 ** 22}"
                  + (f", density {o.density[0]:.3f}" if cls == "sparse" else ""))
            assert_exact(f"{what} [{cls}]", out, ref, o.q)
            if cls == "sparse":
                sums = part.double().sum(0).cpu()
                assert_exact(f"{what} [sparse] sum y", sums[:, 0], o.ref.sum((0, 1, 2)), 1.0)
                assert_exact(f"{what} [sparse] sum y^2", sums[:, 1], (o.ref * o.ref).sum((0, 1, 2)), 1.0)
        else:
            _ratio(what, out, ref, per_image=seam)
            if "stats" in mode:
                _stat_check(what, part, out.double().cpu())


def _check_bn(case, mode, form, rows, seam, what):
    """Data gradient (or paired data gradient) with the fused BatchNorm-backward epilogue; mask recomputed from bn_y or from the hi plane of the
    stored activation; with and without the addend where the entry point takes one (3x3 / s1 only)."""
    import numpy as np
    from artiboost_amd import kernels as K
    N, H, W, Cin, Cout, k, s, p = case
    hi = mode.endswith("_hi")
    adds = (False, True) if (k, s, p) == (3, 1, 1) and not mode.startswith("pair") else (False,)
    for cls in (exact_class(case, mode), "sparse"):
        o = problem(case, mode, cls)
        assert_conditions(o, mode)
        d = _dev(o, case)
        bn_y, bnp = o.bn_y.cuda(), o.bnp.cuda()
        act = K.split(o.act.cuda()) if hi else None
        if hi:
            assert torch.equal(act[0].float().cpu(), o.act) and not bool(act[1].any()), "split() of the stored activation is not (act, 0)"
        for with_add in adds:
            dz, part = _twice(case, mode, d, with_add=with_add, bn=(bn_y, act, bnp))
            assert part is not None and tuple(part.shape) == (rows, Cin, 2), f"{what}: part {None if part is None else tuple(part.shape)}, table {rows}"
            ref_dz, s0, s1, m0, m1 = bn_results(o, with_add)
            assert_exact(f"{what} [{cls}, addend {with_add}] dz", dz, ref_dz, o.q)
            if cls == "sparse":
                print(f"fwd_dgrad {what}: sparse density {o.density[0]:.3f}, masses {float(m0.max()):.0f} / {float(m1.max()):.0f} of {2 ** 22} / {2 ** 21}")
                sums = part.double().sum(0).cpu()
                assert_exact(f"{what} [sparse, addend {with_add}] sum dz", sums[:, 0], s0, 1.0)
                assert_exact(f"{what} [sparse, addend {with_add}] sum dz * xhat", sums[:, 1], s1, 0.5)
    # ---- random class: the existing test's construction and tolerances
    o = problem(case, mode, "random", seam)
    d = _dev(o, case)
    g = torch.Generator().manual_seed(_seed(case, 77))
    ybn = (torch.randn(o.ref.shape, generator=g) * 2 + 0.3).cuda()
    gamma, beta = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.3
    bnp = K.bn_finalize(K.col_stats(ybn), N * H * W, gamma.cuda(), beta.cuda(), torch.zeros(Cin).cuda(), torch.ones(Cin).cuda())
    res = torch.randn(o.ref.shape, generator=g).cuda() if hi else None
    act = K.bn_apply_x3(ybn, bnp, res=res, relu=True, want_f32=True)
    mask = (act.cpu() > 0).double()
    xhat = (ybn.double().cpu() - bnp[2].double().cpu()) * bnp[3].double().cpu()
    for with_add in adds:
        dz, part = _twice(case, mode, d, with_add=with_add, bn=(ybn, act if hi else None, bnp))
        assert part is not None and tuple(part.shape) == (rows, Cin, 2)
        ref_dz = (o.ref_add if with_add else o.ref) * mask
        _ratio(f"{what} addend {with_add}", dz, ref_dz)
        sums, scale = part.double().sum(0).cpu(), float(ref_dz.abs().sum((0, 1, 2)).max())
        np.testing.assert_allclose(sums[:, 0].numpy(), ref_dz.sum((0, 1, 2)).numpy(), rtol=1e-4, atol=3e-5 * scale)
        np.testing.assert_allclose(sums[:, 1].numpy(), (ref_dz * xhat).sum((0, 1, 2)).numpy(), rtol=1e-4, atol=1e-4 * scale)
        # the BatchNorm backward built on (dz, part) == the one that runs its own reduction pass over the raw gradient
        dg1, db1, dg2, db2 = (torch.zeros(Cin).cuda() for _ in range(4))
        dy1 = K.bn_bwd_x3(dz, None, ybn, bnp, dg1, db1, part=part, premasked=True)
        raw_mode = "pair_add" if mode.startswith("pair") else "dgrad_add"
        raw, _ = _launch(case, raw_mode, d, with_add=with_add)
        dy2 = K.bn_bwd_x3(raw, act if hi else None, ybn, bnp, dg2, db2, relu=True if hi else "recompute")
        close((dy1[0].float() + dy1[1].float()).cpu(), (dy2[0].float() + dy2[1].float()).double().cpu(), tol=2e-5)
        np.testing.assert_allclose(dg1.cpu().numpy(), dg2.cpu().numpy(), rtol=2e-4, atol=1e-4 * float(dg2.abs().max()))
        np.testing.assert_allclose(db1.cpu().numpy(), db2.cpu().numpy(), rtol=2e-4, atol=1e-4 * float(db2.abs().max()))


def _check(section, case, mode, form, rows, seam):
    from artiboost_amd import _lib as L
    what = f"s{section} {mode} {form} {case}"
    assert route(case, mode) == (form, rows), f"{what}: the restated pickers give {route(case, mode)}"
    got = library_rows(L.cdll(), case, mode)
    print(f"fwd_dgrad {what}: library rows {got}, table {rows}")
    assert got == rows, f"{what}: the library reports {got} rows, the table has {rows}"
    (_check_bn if "bn_" in mode else _check_plain)(case, mode, form, rows, seam, what)


# ---------------------------------------------------------------- 1. conv3x3_kernel, geometries 1-8
@pytest.mark.parametrize("case,mode,form,rows,seam", _params(1))
def test_conv3x3_forms(case, mode, form, rows, seam):
    _check(1, case, mode, form, rows, seam)


# ---------------------------------------------------------------- 2. conv3x3r.hip
@pytest.mark.parametrize("case,mode,form,rows,seam", _params(2))
def test_conv3x3r_forms(case, mode, form, rows, seam):
    _check(2, case, mode, form, rows, seam)


# ---------------------------------------------------------------- 3. the stride-2 families
@pytest.mark.parametrize("case,mode,form,rows,seam", _params(3))
def test_stride2_forms(case, mode, form, rows, seam):
    _check(3, case, mode, form, rows, seam)


# ---------------------------------------------------------------- 4. conv_gemm2_kernel tile forms and gemm_rw
@pytest.mark.parametrize("case,mode,form,rows,seam", _params(4))
def test_gemm2_and_gemm_rw_forms(case, mode, form, rows, seam):
    _check(4, case, mode, form, rows, seam)


@pytest.mark.parametrize("case,C,D", SAM, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gemm_rw_logits_through_the_fused_softargmax_entry(case, C, D):
    """ab_conv1x1_sam_fwd_x3 writes the logits of the same register-resident GEMM: bit-equal to float64 on the exact class (the soft-argmax
    partials stay on tests/test_gpu_conv_x3.py::test_final_layer_gemm_rw_and_fused_softargmax)."""
    from artiboost_amd import kernels as K
    N, H, W, Cin, Cout, k, s, p = case
    assert Cout == C * 32
    o = problem(case, "fwd_bias", exact_class(case, "fwd_bias"))
    assert_conditions(o, "fwd_bias")
    d = _dev(o, case)
    assert K.conv1x1_sam_fwd_x3_ok(d.a, d.w, C, D, 32)
    logits, part = K.conv1x1_sam_fwd_x3(d.a, d.w, d.bias, C, D)
    assert_exact(f"sam logits {case}", logits, o.ref, o.q)
    assert tuple(part.shape) == (N, H * W // 64, C, 8)
    assert torch.equal(K.conv1x1_sam_fwd_x3(d.a, d.w, d.bias, C, D)[0], logits), "a second call differs"


# ---------------------------------------------------------------- 5. a slice of a larger buffer, guarded tail, once per kernel family
GUARD = [
    pytest.param((2, 12, 20, 64, 40, 3, 1, 1), "fwd_stats", id="conv3x3-fwd"),
    pytest.param((2, 12, 20, 40, 64, 3, 1, 1), "dgrad_add", id="conv3x3-dgrad"),
    pytest.param((2, 12, 20, 40, 64, 3, 1, 1), "bn_hi", id="conv3x3-bn"),
    pytest.param((1, 64, 128, 64, 64, 3, 1, 1), "fwd_stats", id="conv3x3r-fwd"),
    pytest.param((1, 64, 128, 64, 64, 3, 1, 1), "bn_hi", id="conv3x3r-bn"),
    pytest.param((2, 16, 16, 128, 64, 3, 2, 1), "fwd_stats", id="convp-fwd"),
    pytest.param((2, 16, 16, 64, 64, 3, 2, 1), "pair", id="convp-pair"),
    pytest.param((2, 16, 16, 64, 64, 3, 2, 1), "pair_bn_hi", id="convp-pair-bn"),
    pytest.param((2, 16, 16, 64, 64, 4, 2, 1), "fwd_stats", id="conv2x2-fwd"),
    pytest.param((4, 16, 16, 64, 32, 4, 2, 1), "dgrad_stats", id="conv2x2-tfwd"),
    pytest.param((2, 9, 5, 64, 40, 1, 1, 0), "fwd_bias_stats", id="gemm2"),
    pytest.param((3, 14, 10, 64, 128, 3, 2, 1), "dgrad_stats", id="gemm2-nclass4"),
    pytest.param((2, 9, 5, 128, 64, 1, 1, 0), "bn_recompute", id="gemm2-bn"),
    pytest.param((1, 8, 16, 192, 96, 1, 1, 0), "fwd_bias", id="gemm_rw"),
]
TAIL, PRE = 4096, 1040


def _guarded(shape):
    """A float32 view of `shape` inside a byte buffer of 0xA5, 1040 bytes in, with 4 KiB behind it."""
    n = 4
    for v in shape:
        n *= v
    buf = torch.full((PRE + n + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[PRE:PRE + n].view(torch.float32).view(shape), n


@pytest.mark.parametrize("case,mode", GUARD)
def test_outputs_in_a_slice_of_a_larger_buffer_leave_the_guard_unchanged(case, mode):
    """The library entry points on an output (and partial rows) that are slices of larger buffers: exact results, and neither the bytes in
    front nor the 4 KiB behind either slice change."""
    from artiboost_amd import _lib as L
    from artiboost_amd import kernels as K
    N, H, W, Cin, Cout, k, s, p = case
    lib = L.lib()
    form, rows = route(case, mode)
    o = problem(case, mode, "sparse" if ("stats" in mode or "bn_" in mode) else exact_class(case, mode))
    assert_conditions(o, mode)
    d = _dev(o, case)
    out_ch = Cout if o.fwd else Cin
    obuf, out, on = _guarded(tuple(o.ref.shape))
    has_rows = "stats" in mode or "bn_" in mode
    pbuf, part, pn = _guarded((rows, out_ch, 2)) if has_rows else (None, None, 0)
    ah, al, wh, wl = d.a[0], d.a[1], d.w[0], d.w[1]
    dims = (L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(k), L.i(k))
    if o.fwd:
        L.check(lib.ab_conv2d_fwd_x3(L.ptr(ah), L.ptr(al), L.ptr(wh), L.ptr(wl), L.ptr(out), *dims, L.i(s), L.i(p), L.ptr(d.bias), L.ptr(part),
                                     L.i(0), L.stream()), "ab_conv2d_fwd_x3")
        ref, sums = o.ref, ((o.ref.sum((0, 1, 2)), (o.ref * o.ref).sum((0, 1, 2))) if has_rows else None)
    elif "bn_" in mode:
        act = K.split(o.act.cuda())[0] if mode.endswith("_hi") else None
        bn_y, bnp = o.bn_y.cuda(), o.bnp.cuda()
        if mode.startswith("pair"):
            L.check(lib.ab_conv2d_dgrad_x3_pair_bn(L.ptr(ah), L.ptr(al), L.ptr(wh), L.ptr(wl), L.ptr(d.a2[0]), L.ptr(d.a2[1]), L.ptr(d.w2[0]), L.ptr(d.w2[1]),
                                                   L.ptr(out), *dims, L.i(p), L.ptr(bn_y), L.ptr(act), L.ptr(bnp), L.ptr(part), L.stream()),
                    "ab_conv2d_dgrad_x3_pair_bn")
            with_add = False
        else:
            with_add = (k, s, p) == (3, 1, 1)
            L.check(lib.ab_conv2d_dgrad_x3_bn(L.ptr(ah), L.ptr(al), L.ptr(wh), L.ptr(wl), L.ptr(out), *dims, L.i(s), L.i(p),
                                              L.ptr(d.addend if with_add else None), L.ptr(bn_y), L.ptr(act), L.ptr(bnp), L.ptr(part), L.stream()),
                    "ab_conv2d_dgrad_x3_bn")
        ref, s0, s1, _, _ = bn_results(o, with_add)
        sums = (s0, s1)
    elif mode.startswith("pair"):
        L.check(lib.ab_conv2d_dgrad_x3_pair(L.ptr(ah), L.ptr(al), L.ptr(wh), L.ptr(wl), L.ptr(d.a2[0]), L.ptr(d.a2[1]), L.ptr(d.w2[0]), L.ptr(d.w2[1]),
                                            L.ptr(out), *dims, L.i(p), L.ptr(None), L.stream()), "ab_conv2d_dgrad_x3_pair")
        ref, sums = o.ref, None
    else:
        addend = d.addend if mode.endswith("_add") else None
        L.check(lib.ab_conv2d_dgrad_x3(L.ptr(ah), L.ptr(al), L.ptr(wh), L.ptr(wl), L.ptr(out), *dims, L.i(s), L.i(p), L.ptr(addend), L.ptr(part),
                                       L.stream()), "ab_conv2d_dgrad_x3")
        ref = o.ref_add if addend is not None else o.ref
        sums = (o.ref.sum((0, 1, 2)), (o.ref * o.ref).sum((0, 1, 2))) if has_rows else None
    torch.cuda.synchronize()
    for name, buf, n in (("output", obuf, on), ("partial rows", pbuf, pn)):
        if buf is not None:
            assert bool((buf[:PRE] == 0xA5).all()), f"{form}: wrote in front of its {name}"
            assert bool((buf[PRE + n:] == 0xA5).all()), f"{form}: wrote behind its {name}"
    assert_exact(f"guarded {mode} {form} {case}", out, ref, o.q)
    if sums is not None:
        got = part.double().sum(0).cpu()
        assert_exact(f"guarded {mode} {form} rows[:, 0]", got[:, 0], sums[0], 1.0)
        assert_exact(f"guarded {mode} {form} rows[:, 1]", got[:, 1], sums[1], 0.5 if "bn_" in mode else 1.0)
